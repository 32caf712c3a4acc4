"""Backward-data of the convolutions (hl_conv2d_nhwc_bwd_data, through the C ABI) on every kernel it reaches, against float64 autograd
of the operands as that kernel rounds them (tests/conv_bwd_cases.py; tests/test_conv_bwd_cpu.py pins each case to its kernel with
hl_conv2d_bwd_data_plan), and the weight-gradient kernels on ragged geometries through _Conv.apply.

The bounds are the suite's standing ones for the same kernels in the forward direction (E = max-abs against float64, dx is O(1)):
    k_conv, k_conv_dma        E < 2e-5 max(1, |dx|max)                                            (test_conv_matches_torch)
    k_conv_wino  F(2x2)       that, and E < 8 E_direct + 1e-6                                      (test_conv_winograd_matches_torch)
    k_conv_wino4[w]  F(4x4)   E < 4e-5, rms < 8 rms_direct + 1e-7                                  (test_conv_winograd_f43_matches_torch)
    k_conv_h16 / k_conv1_h16  E < 2e-5, rel-L2 < 1e-6 (split-K: 5e-5, 2e-6) against the rounded-operand reference
                              (test_conv_h16_equals_the_convolution_of_the_rounded_operands, test_conv_h16_split_k_on_small_layers)
    k_conv_bf3 (HL_CONV_BF16) E < norm_cases.bar(E_ref) = 4 E_ref + 2e-6 against the rounded-operand reference, E_ref = fp32 CPU
                              autograd on the same rounded operands
E_direct / rms_direct: the same call under HL_CONV_FP32_DIRECT (k_conv / k_conv_dma only)."""
import pytest
import torch

from tests import conv_bwd_cases as cb
from tests import norm_cases as nc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

SENTINEL = -7.0


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _modes():
    from humanliff_amd import _lib
    return {"fp32": _lib.HL_CONV_FP32, "bf16": _lib.HL_CONV_BF16, "fp16": _lib.HL_CONV_FP16, "direct": _lib.HL_CONV_FP32_DIRECT}


def _device_operands(c):
    """dy (N,Ho,Wo,Cy) with zero pad channels [Cout, Cy), w (Cout,Cin,ks,ks), on the device."""
    dy, w = cb.operands(c)
    dyp = torch.zeros((c.N, c.Ho, c.Wo, c.Cy))
    dyp[..., :c.Cout] = nhwc(dy)
    return dyp.to(dev), w.to(dev)


def _call(c, mode, dy, w):
    """One hl_conv2d_nhwc_bwd_data into a dx that lives inside a larger buffer of SENTINELs: one image row of guard on either side, and the
    pad channels [Cin, Cx) inside it.  Asserts that the guards and the pad channels come back bit-identical (behind an upsample the pad
    channels come back zero: the 2x2 sums are stored for all Cx channels) -> dx (N, Cin, H, W) on the CPU."""
    from humanliff_amd import _lib
    L = _lib.lib()
    H, W = cb.x_hw(c)
    guard, n = W * c.Cx, c.N * H * W * c.Cx
    buf = torch.full((guard + n + guard,), SENTINEL, device=dev)
    dx = buf[guard:guard + n].view(c.N, H, W, c.Cx)
    need = L.hl_conv2d_bwd_data_scratch_bytes(mode, *cb.abi_args(c))
    assert need > 0
    scratch = torch.empty(need // 4, device=dev)
    with _lib.on(dev):
        _lib.check(L.hl_conv2d_nhwc_bwd_data(mode, _lib.ptr(dy), c.N, c.Ho, c.Wo, c.Cy, _lib.ptr(w), c.Cout, c.Cin, c.ks, c.stride, c.ups,
                                             _lib.ptr(dx), c.Cx, _lib.ptr(scratch), need, _lib.stream_ptr()), "hl_conv2d_nhwc_bwd_data")
    torch.cuda.synchronize()
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), "wrote outside dx"
    assert bool((dx[..., c.Cin:] == (0.0 if c.ups else SENTINEL)).all()), "wrote the pad channels of dx"
    got = dx[..., :c.Cin]
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any())
    return nchw(got.cpu())


def _errors(got, want):
    d = got.double() - want
    return float(d.abs().max()), float(d.pow(2).mean().sqrt()), float(d.norm() / want.norm())


@pytest.mark.parametrize("name", sorted(cb.CASES))
def test_backward_data_matches_float64_on_its_kernel(name):
    """Measured on MI355X (E, worst per family): see the backward-data table in DESIGN.md.  k_conv_bf3 under HL_CONV_BF16, which has no
    standing tight bound: bf16_bf3_split E 8.3e-7 at E_ref 1.3e-6 (bar 7.1e-6), bf16_bf3_1x1 6.1e-7 at 1.2e-6, bf16_bf3_1x1_split 8.0e-7 at 1.9e-6."""
    c = cb.CASES[name]
    modes = _modes()
    r = cb.reference(c)
    dy, w = _device_operands(c)
    got = _call(c, modes[c.mode], dy, w)
    e, rms, rel = _errors(got, r["want"])
    line = f"{name} ({c.kernel}{', split-K' if c.split else ''}): |dx|max {r['scale']:.2f}  E {e:.2e}  rms {rms:.2e}  rel-L2 {rel:.2e}  E_ref {r['e_ref']:.2e}"

    # the same call again: the same bits
    assert torch.equal(_call(c, modes[c.mode], dy, w), got)

    sixteen = cb.rounding(c) is not None
    if not sixteen:
        direct = _call(c, modes["direct"], dy, w)
        e_d, rms_d, _ = _errors(direct, r["want"])
        line += f"  E_direct {e_d:.2e}  rms_direct {rms_d:.2e}"
    else:
        _, _, rel_exact = _errors(got, r["exact"])
        line += f"  rel-L2 against the unrounded gradient {rel_exact:.2e}"
    print(line)

    if c.kernel in ("k_conv", "k_conv_dma"):
        assert e < 2e-5 * max(1.0, r["scale"]), line
    elif c.kernel == "k_conv_wino":
        assert not torch.equal(got, direct), "the Winograd kernel did not run"
        assert e < 2e-5 * max(1.0, r["scale"]) and e < 8 * e_d + 1e-6, line
    elif c.kernel in ("k_conv_wino4", "k_conv_wino4w"):
        assert not torch.equal(got, direct), "the Winograd kernel did not run"
        assert e < 4e-5 and rms < 8 * rms_d + 1e-7, line
    elif c.kernel == "k_conv_h16":
        assert (e < 5e-5 and rel < 2e-6) if c.split else (e < 2e-5 and rel < 1e-6), line
    elif c.kernel == "k_conv_bf3":
        assert e < nc.bar(r["e_ref"]), line
    else:
        raise KeyError(c.kernel)
    if not sixteen:
        assert e_d < 2e-5 * max(1.0, r["scale"]), line                 # (the twin is a direct kernel: its own bound)
    else:
        assert rel_exact > 1e-5, line                                  # 16-bit arithmetic ran (the fp32 kernels sit at 1e-7)

    # gradients in training are 1e-4 ... 1e-9: every operation on the path is a multiply, an add or a round-to-nearest conversion far from
    # under- and overflow, so a power-of-two scale of dy goes through bit for bit (fp16 operands excepted: 2^-20 dy is below fp16's range)
    if not (c.kernel == "k_conv_h16" and c.mode == "fp16"):
        s = 2.0 ** -20
        assert torch.equal(_call(c, modes[c.mode], dy * s, w), got * s), "a 2^-20 scale of dy changed the bits of dx"


def _conv_apply(g, kind, x, w, b, cot):
    """_Conv.apply forward + backward in the arithmetic `kind` -> y, dx (NCHW, CPU), dw, db (CPU)."""
    from humanliff_amd.improved_diffusion import unet_train as ut
    xd = ut._pad_c(nhwc(x), 16).to(dev).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    ut.set_train_arithmetic(kind)
    try:
        y = ut._Conv.apply(xd, wd, bd, g.stride, g.ups)
        (y * nhwc(cot).to(dev)).sum().backward()
    finally:
        ut.set_train_arithmetic(None)
    return nchw(y.detach().cpu()), nchw(xd.grad.cpu())[:, :g.Cin], wd.grad.cpu(), bd.grad.cpu()


@pytest.mark.parametrize("name", sorted(cb.WGRAD_CASES))
def test_weight_gradient_on_ragged_geometries_fp32(name):
    """k_conv_wgrad_t<1>, <2> and k_conv_wgrad_1x1 where tiles are ragged and slabs cross images, with the tolerances of
    test_conv_backward_matches_torch_autograd."""
    k = cb.wgrad_case(name)
    g = k["geom"]
    y, dx, dw, db = _conv_apply(g, "fp32", k["x"], k["w"], k["b"], k["cot"])
    sx, sw, sb = float(k["dx"].abs().max()), float(k["dw"].abs().max()), float(k["db"].abs().max())
    e_y, e_x = float((y.double() - k["y"]).abs().max()), float((dx.double() - k["dx"]).abs().max())
    e_w, e_b = float((dw.double() - k["dw"]).abs().max()), float((db.double() - k["db"]).abs().max())
    print(f"{name} fp32: forward {e_y:.2e}  dx {e_x:.2e} (max {sx:.2f})  dW {e_w / sw:.2e} of max  db {e_b / sb:.2e} of max")
    assert e_y < 3e-5
    assert e_x < 2e-5 * max(1.0, sx)
    assert e_w < 1e-5 * sw and e_b < 1e-5 * sb
    again = _conv_apply(g, "fp32", k["x"], k["w"], k["b"], k["cot"])
    assert torch.equal(again[2], dw) and torch.equal(again[3], db) and torch.equal(again[1], dx)


@pytest.mark.parametrize("name", sorted(cb.WGRAD_CASES))
def test_weight_gradient_on_ragged_geometries_bf16(name):
    """The same layers in bf16 arithmetic, with the checks of test_16bit_weight_gradient_equals_the_gradient_of_the_rounded_operands: the
    3x3 / stride-1 layer (k_conv_wgrad_h16) gives the float64 weight gradient of the operands rounded to bf16 up to fp32 summation; the
    stride-2 and 1x1 layers keep the fp32 kernels (hl_conv2d_wgrad_nhwc_ws_mode), so theirs is that of the unrounded operands; db is the
    fp32 row sum of the unrounded output gradient; bit-reproducible."""
    k = cb.wgrad_case(name)
    g = k["geom"]
    runs = [_conv_apply(g, "bf16", k["x"], k["w"], k["b"], k["cot"]) for _ in range(2)]
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])
    dw, db = runs[0][2], runs[0][3]
    dw_ref = k["dw16"] if k["dw16"] is not None else k["dw"]
    ew = float((dw.double() - dw_ref).abs().max() / dw_ref.abs().max())
    eb = float((db.double() - k["db"]).abs().max() / k["db"].abs().max())
    print(f"{name} bf16 ({'rounded' if k['dw16'] is not None else 'fp32'} operands): dW max-abs / max {ew:.2e}, db {eb:.2e}")
    assert ew < (2e-5 if k["dw16"] is not None else 1e-5) and eb < 1e-5      # (the fp32 kernels: test_conv_backward_matches_torch_autograd's bound)
    if k["dw16"] is not None:                                           # 16-bit arithmetic ran: the unrounded gradient is a rounding away
        assert float((dw.double() - k["dw"]).abs().max() / k["dw"].abs().max()) > 1e-4
