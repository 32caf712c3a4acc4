"""k_conv_h2s_ph on the GPU: the Upsample convolutions (nearest x2 + 3x3) of the default mode as four 2x2-tap phase convolutions of the source, against
the float64 convolution of the upsampled input, with the fp32 direct kernel's result on the same operands alongside.  Bounds: those of
test_conv3x3_fp16x2_products_match_float64 (tests/test_unet_gpu.py).  Shapes are (N, source H, source W, Cin, Cout); one float64 reference per case,
shared and never written to."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import norm_cases as nc
from tests.test_conv_upsample_phases_cpu import K_H2S, K_H2S_PH, plan

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _scratch(shape, gn_query=False):
    from humanliff_amd import _lib
    N, H, W, C, Cout = shape
    q = getattr(_lib.lib(), "hl_conv2d_gn_scratch_bytes" if gn_query else "hl_conv2d_scratch_bytes")
    need = max(q(m, N, H, W, C, Cout, 3, 1, 1, 0) for m in (_lib.HL_CONV_FP32, _lib.HL_CONV_FP32_DIRECT))
    return torch.empty(need // 4, device=dev)


def _run(mode, shape, x, w, b, r=None):
    from humanliff_amd import _lib
    N, H, W, C, Cout = shape
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    rd = r.to(dev) if r is not None else None
    out = torch.zeros((N, 2 * H, 2 * W, Cout), device=dev)
    scratch = _scratch(shape)
    _lib.check(_lib.lib().hl_conv2d_nhwc_mode(mode, _lib.ptr(xd), N, H, W, C, _lib.ptr(wd), _lib.ptr(bd), Cout, 3, 1, 1, None, None, 0, _lib.ptr(rd), _lib.ptr(out),
                                              _lib.ptr(scratch), scratch.numel() * 4, _lib.stream_ptr()), "hl_conv2d_nhwc_mode")
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def case(shape, kind="random"):
    """x (N, H, W, C), w, b, r (the residual) and ref = the float64 convolution of the nearest-x2 input, NHWC, without the residual.
    kind 'cancel': columns 1 and 2 of every 3x3 kernel are opposite up to 1e-4 noise, and rows 1 and 2 alike - the summed taps nearly vanish."""
    N, H, W, C, Cout = shape
    g = torch.Generator().manual_seed(N + C + Cout + H + (7 if kind == "cancel" else 0))
    x = torch.randn((N, H, W, C), generator=g) * 1.5
    w = torch.randn((Cout, C, 3, 3), generator=g) / (9 * C) ** 0.5
    if kind == "cancel":
        w[:, :, :, 1] = -w[:, :, :, 2] + 1e-4 * torch.randn((Cout, C, 3), generator=g)
        w[:, :, 1, :] = -w[:, :, 2, :] + 1e-4 * torch.randn((Cout, C, 3), generator=g)
    b = torch.randn(Cout, generator=g)
    r = torch.randn((N, 2 * H, 2 * W, Cout), generator=g)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    xi = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest")
    ref = F.conv2d(xi, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=w, b=b, r=r, ref=ref)


def _check_against_float64(shape, kind, res):
    from humanliff_amd import _lib
    c = case(shape, kind)
    C = shape[3]
    ref = c["ref"] + c["r"].double() if res else c["ref"]
    r = c["r"] if res else None
    out = _run(_lib.HL_CONV_FP32, shape, c["x"], c["w"], c["b"], r).double()
    out32 = _run(_lib.HL_CONV_FP32_DIRECT, shape, c["x"], c["w"], c["b"], r).double()
    scale = float(ref.abs().mean())
    e2, e32 = float((out - ref).abs().max()), float((out32 - ref).abs().max())
    l2, l32 = float((out - ref).norm() / ref.norm()), float((out32 - ref).norm() / ref.norm())
    print(f"ups 3x3 {shape} {kind} res={res}: default max-abs {e2:.2e} rel-L2 {l2:.2e}; fp32 direct {e32:.2e} / {l32:.2e} (output mean-abs {scale:.2f})")
    assert e2 < 6e-6 * max(1.0, scale) * (9 * C / 384) ** 0.5, (e2, scale)
    assert l2 < 1.6e-6 and l2 < 4 * l32 + 2e-7, (l2, l32)
    return out, out32


@pytest.mark.parametrize("shape,kind,res,splits", [
    ((1, 40, 80, 96, 384), "random", False, 1),      # 80x160 output: 100 workgroups' worth (the unsplit threshold), three chunks (both stage parities, an odd count),
    ((1, 40, 80, 96, 384), "random", True, 1),       # two channel blocks, a non-square image; with the residual read through the same output-pixel map
    ((1, 40, 80, 32, 384), "random", False, 1),      # one chunk: prologue and epilogue only
    ((4, 8, 16, 160, 192), "random", False, 2),      # one source tile per image: every workgroup touches all four borders; five chunks in slabs of 3 + 2
    ((1, 40, 80, 64, 384), "cancel", False, 1),      # two chunks, summed taps that nearly cancel
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upsample_phases_match_float64(shape, kind, res, splits):
    assert plan(*shape) == (K_H2S_PH, splits)
    out, out32 = _check_against_float64(shape, kind, res)
    assert not torch.equal(out, out32)                      # the default mode really took another kernel


def test_nearly_cancelling_taps_on_the_two_chunk_shape():
    """(2, 16, 32, 64, 192) with W[., 1] = -W[., 2] + 1e-4 noise, rows alike.  16 workgroups' worth and two chunks leave split-K no second slab of two chunks,
    so the planner never gave this layer to k_conv_h2s and does not give it to the phases (the 1 x 40 x 80 x 64 case above runs them on such weights);
    the bound against float64 holds on the kernel it takes all the same."""
    shape = (2, 16, 32, 64, 192)
    assert plan(*shape)[0] not in (K_H2S, K_H2S_PH)
    _check_against_float64(shape, "cancel", False)


@pytest.mark.parametrize("shape,kernel", [((2, 8, 8, 64, 192), None), ((8, 8, 8, 128, 192), K_H2S)], ids=["2x8x8x64x192", "8x8x8x128x192"])
def test_source_width_8_keeps_the_nine_taps(shape, kernel):
    """a source 8 pixels wide has no whole 8x16 tile: the nine-tap path, same bound (the second shape has enough chunks to reach k_conv_h2s itself)"""
    k = plan(*shape)[0]
    assert k != K_H2S_PH and (kernel is None or k == kernel)
    _check_against_float64(shape, "random", False)


def test_upsample_phases_are_scale_invariant():
    """weights x 2^a and input x 2^b (the bias x 2^(a + b)): the result x 2^-(a + b) is the unscaled one, bit for bit"""
    from humanliff_amd import _lib
    shape = (1, 40, 80, 96, 384)
    assert plan(*shape) == (K_H2S_PH, 1)
    c = case(shape)
    base = _run(_lib.HL_CONV_FP32, shape, c["x"], c["w"], c["b"])
    for a in (0, -6, -12, 6):
        for bx in (0, 5, -5):
            s = 2.0 ** (a + bx)
            out = _run(_lib.HL_CONV_FP32, shape, c["x"] * 2.0 ** bx, c["w"] * 2.0 ** a, c["b"] * s)
            assert torch.equal(out / s, base), (a, bx, float((out / s - base).abs().max()))


@pytest.mark.parametrize("shape,splits", [((4, 8, 16, 160, 192), 2), ((1, 40, 80, 96, 384), 1)], ids=["4x8x16x160x192", "1x40x80x96x384"])
def test_upsample_phases_emit_the_groupnorm_totals(shape, splits):
    """hl_conv2d_nhwc_gn: the next GroupNorm's affine from the totals of the launch (the epilogue's, or the split-K finish's) against float64
    GroupNorm32 of the stored tensor, at the bar of tests/norm_cases.py; the stored tensor is the plain call's."""
    from humanliff_amd import _lib
    L = _lib.lib()
    assert plan(*shape) == (K_H2S_PH, splits)
    N, H, W, C, Cout = shape
    c = case(shape)
    g = nc._gen("ups_phases", shape)
    gamma, beta = torch.randn(Cout, generator=g) * 0.2 + 1, torch.randn(Cout, generator=g) * 0.2
    xd, wd, bd, gd_, be_ = (t.to(dev) for t in (c["x"], c["w"], c["b"], gamma, beta))
    out = torch.empty((N, 2 * H, 2 * W, Cout), device=dev)
    nA, nB = torch.empty((N, Cout), device=dev), torch.empty((N, Cout), device=dev)
    scratch = _scratch(shape, gn_query=True)
    used = ctypes.c_int(-1)
    _lib.check(L.hl_conv2d_nhwc_gn(_lib.HL_CONV_FP32, _lib.ptr(xd), N, H, W, C, _lib.ptr(wd), _lib.ptr(bd), Cout, 3, 1, 1, None, None, 0, None, _lib.ptr(out),
                                   _lib.ptr(gd_), _lib.ptr(be_), _lib.ptr(nA), _lib.ptr(nB), ctypes.byref(used), _lib.ptr(scratch), scratch.numel() * 4,
                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert used.value > 0, used.value
    assert torch.equal(out.cpu(), _run(_lib.HL_CONV_FP32, shape, c["x"], c["w"], c["b"]))
    y = out.cpu().permute(0, 3, 1, 2).contiguous()
    want = F.group_norm(y.double(), 32, gamma.double(), beta.double(), 1e-5)
    e_ref = nc.err(F.group_norm(y, 32, gamma, beta, 1e-5), want)
    rec = y.double() * nA.cpu().double()[:, :, None, None] + nB.cpu().double()[:, :, None, None]
    e = nc.err(rec, want)
    print(f"hl_conv2d_nhwc_gn ups {shape}: E {e:.2e}  E_ref {e_ref:.2e}  bar {nc.bar(e_ref):.2e}")
    assert e <= nc.bar(e_ref)
