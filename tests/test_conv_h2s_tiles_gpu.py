"""k_conv_h2s (3x3 fp16x2 convolution, 8x16-pixel tiles) with its 1 x 4 wave layout of 16x16x32 tiles: every kind of launch the dispatcher sends
to it, against a float64 convolution of the fp32 operands.  The bound is the one of test_conv_fp16x2_products_are_scale_invariant: rel-L2 of the fp16x2
result <= 1.3 x that of the fp32 direct kernel + 5e-8.  Every case also runs twice and must give the same bits."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

# (N, H, W, C, Cout, ups, gn, silu, res): input size H x W (the output is 2H x 2W under ups)
CASES = {
    "256px": (1, 256, 256, 96, 192, 0, False, 0, False),
    "128px": (2, 128, 128, 192, 192, 0, False, 0, True),
    "64px": (4, 64, 64, 192, 384, 0, False, 0, False),
    "32px_splitk": (4, 32, 32, 384, 384, 0, False, 0, True),
    "16px_splitk": (8, 16, 16, 384, 384, 0, False, 0, False),
    "upsample": (4, 64, 64, 192, 192, 1, False, 0, True),
    "upsample_splitk": (2, 32, 32, 384, 192, 1, False, 0, False),
    "gn_silu": (2, 128, 128, 192, 192, 0, True, 1, True),
    "gn_affine": (4, 64, 64, 384, 192, 0, True, 0, False),
}


def _operands(N, H, W, C, Cout, gn, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g) * 1.5
    w = torch.randn((Cout, C, 3, 3), generator=g) / (9 * C) ** 0.5
    w = w * torch.exp2(torch.randint(-6, 1, (Cout, 1, 1, 1), generator=g).float())
    b = torch.randn(Cout, generator=g) * 0.1
    cA, cB = (torch.rand((N, C), generator=g) + 0.5, torch.randn((N, C), generator=g) * 0.1) if gn else (None, None)
    return x, w, b, cA, cB


def _reference(x, w, b, ups, cA, cB, silu, res):
    xin = x.double()
    if cA is not None:
        xin = xin * cA.double()[:, None, None, :] + cB.double()[:, None, None, :]
        if silu:
            xin = xin * torch.sigmoid(xin)
    xin = xin.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    torch.set_num_threads(min(32, torch.get_num_threads()))
    y = F.conv2d(xin, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return y + res.double() if res is not None else y


def _scratch(N, H, W, C, Cout, ups):
    """One buffer for every call of a test: the largest hl_conv2d_nhwc_gn asks for over both modes, with and without a GroupNorm in front
    (the room of the plain call sits behind its prefix)."""
    from humanliff_amd import _lib
    need = max(_lib.lib().hl_conv2d_gn_scratch_bytes(m, N, H, W, C, Cout, 3, 1, ups, gn)
               for m in (_lib.HL_CONV_FP32, _lib.HL_CONV_FP32_DIRECT) for gn in (0, 1))
    return torch.empty(need // 4, device=dev)


def _run(L, _lib, mode, x, w, b, Cout, ups, cA, cB, silu, res, scratch):
    N, H, W, C = x.shape
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    out = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev)
    _lib.check(L.hl_conv2d_nhwc_mode(mode, _lib.ptr(x), N, H, W, C, _lib.ptr(w), _lib.ptr(b), Cout, 3, 1, ups,
                                     _lib.ptr(cA) if cA is not None else None, _lib.ptr(cB) if cB is not None else None, silu,
                                     _lib.ptr(res) if res is not None else None, _lib.ptr(out), _lib.ptr(scratch), scratch.numel() * 4,
                                     _lib.stream_ptr()), "hl_conv2d_nhwc_mode")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_conv_h2s_tiles_match_float64(case):
    from humanliff_amd import _lib
    L = _lib.lib()
    N, H, W, C, Cout, ups, gn, silu, with_res = CASES[case]
    x, w, b, cA, cB = _operands(N, H, W, C, Cout, gn, seed=N + H + C + Cout + ups)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    res = torch.randn((N, Ho, Wo, Cout), generator=torch.Generator().manual_seed(7)) if with_res else None
    ref = _reference(x, w, b, ups, cA, cB, silu, res)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    cAd, cBd = (cA.to(dev), cB.to(dev)) if gn else (None, None)
    rd = res.to(dev) if with_res else None
    scratch = _scratch(N, H, W, C, Cout, ups)
    out = _run(L, _lib, _lib.HL_CONV_FP32, xd, wd, bd, Cout, ups, cAd, cBd, silu, rd, scratch)
    again = _run(L, _lib, _lib.HL_CONV_FP32, xd, wd, bd, Cout, ups, cAd, cBd, silu, rd, scratch)
    out32 = _run(L, _lib, _lib.HL_CONV_FP32_DIRECT, xd, wd, bd, Cout, ups, cAd, cBd, silu, rd, scratch)
    assert torch.equal(out, again)                       # run-to-run bit identity
    out, out32 = out.cpu().double(), out32.cpu().double()
    assert torch.isfinite(out).all()
    assert not torch.equal(out, out32)                   # the default mode took the fp16x2 kernel, not the fp32 direct one
    l2, l32 = float((out - ref).norm() / ref.norm()), float((out32 - ref).norm() / ref.norm())
    print(f"{case}: rel-L2 {l2:.3e} (fp32 direct {l32:.3e})")
    assert l2 <= 1.3 * l32 + 5e-8, (l2, l32)


@pytest.mark.parametrize("N,H,W,C,Cout,res", [(2, 128, 128, 192, 192, True), (4, 64, 64, 384, 384, False)])
def test_conv_h2s_tiles_group_statistics(N, H, W, C, Cout, res):
    """The epilogue's GroupNorm statistics (per tile and channel half) of the stored tensor, as the next layer's coefficients."""
    from humanliff_amd import _lib
    L = _lib.lib()
    x, w, b, cA, cB = _operands(N, H, W, C, Cout, True, seed=11 + N + C)
    g = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    r = torch.randn((N, H, W, Cout), generator=g) if res else None
    out = torch.empty((N, H, W, Cout), device=dev)
    nA, nB = torch.empty((N, Cout), device=dev), torch.empty((N, Cout), device=dev)
    scratch = _scratch(N, H, W, C, Cout, 0)
    used = ctypes.c_int(-1)
    xd, wd, bd, cAd, cBd, gd, bed = (t.to(dev) for t in (x, w, b, cA, cB, gamma, beta))
    rd = r.to(dev) if res else None
    _lib.check(L.hl_conv2d_nhwc_gn(_lib.HL_CONV_FP32, _lib.ptr(xd), N, H, W, C, _lib.ptr(wd), _lib.ptr(bd), Cout, 3, 1, 0, _lib.ptr(cAd), _lib.ptr(cBd), 1,
                                   _lib.ptr(rd) if res else None, _lib.ptr(out), _lib.ptr(gd), _lib.ptr(bed), _lib.ptr(nA), _lib.ptr(nB), ctypes.byref(used),
                                   _lib.ptr(scratch), scratch.numel() * 4, _lib.stream_ptr()), "hl_conv2d_nhwc_gn")
    torch.cuda.synchronize()
    assert used.value > 0
    y = out.cpu().double()
    ref = _reference(x, w, b, 0, cA, cB, 1, r)
    l2 = float((y - ref).norm() / ref.norm())
    assert l2 < 2e-6, l2
    yd = y.permute(0, 3, 1, 2).reshape(N, 32, -1)
    mean, var = yd.mean(dim=2), yd.var(dim=2, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    cg = Cout // 32
    wantA = (rstd[:, :, None] * gamma.double().reshape(1, 32, cg)).reshape(N, Cout)
    wantB = beta.double()[None] - (mean[:, :, None].expand(N, 32, cg).reshape(N, Cout)) * wantA
    assert (nA.cpu().double() - wantA).abs().max() < 2e-6 * wantA.abs().max()
    assert (nB.cpu().double() - wantB).abs().max() < 2e-6 * max(1.0, float(wantB.abs().max()))
