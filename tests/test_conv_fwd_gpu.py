"""The forward convolutions (hl_conv2d_nhwc_mode, and hl_conv2d_nhwc_gn for the cases that return statistics) on every kernel instantiation
the plan reaches, against float64 F.conv2d of the operands as that kernel rounds them (tests/conv_fwd_cases.py; tests/test_conv_fwd_cpu.py
pins each case to its instantiation with hl_conv2d_plan_ex).

The bounds are the suite's standing ones (E = max-abs against float64, rms and rel-L2 likewise; _direct: the same call under
HL_CONV_FP32_DIRECT, which runs k_conv / k_conv_dma and is held to its own bound wherever it is the yardstick):
    k_conv, k_conv_dma        E < 2e-5 max(1, |y|max)                                              (test_conv_matches_torch, test_conv_bwd_gpu)
    k_conv_wino  F(2x2)       that, and E < 8 E_direct + 1e-6                                        (test_conv_winograd_matches_torch)
    k_conv_wino4[w]  F(4x4)   E < 4e-5 max(1, |y|max), rms < 8 rms_direct + 1e-7                     (test_conv_winograd_f43_matches_torch)
    k_conv_bf3, three planes  the direct bound, and E < 4 E_direct + 1e-6                            (test_conv_bf16x3_emulation_matches_torch)
    k_conv_bf3, HL_CONV_BF16  E < norm_cases.bar(E_ref) against the rounded-operand reference        (test_conv_bwd_gpu)
    k_conv_h16 / k_conv1_h16  E < 2e-5, rel-L2 < 1e-6 (split-K: 5e-5, 2e-6) against the rounded-operand reference, and rel-L2 against the
                              unrounded one > 1e-5: 16-bit arithmetic ran                            (test_conv_h16_..., test_conv_bwd_gpu)
    the fp16x2 kernels        rel-L2 <= 1.3 rel-L2_direct + 5e-8, the direct bound on E, and not the direct kernel's bits
                                                                                                     (test_conv_h2s_tiles_gpu, test_conv_matches_torch)
    a GroupNorm output rounded to 16 bits ("half", or "dense" in front of k_conv_bf3 under HL_CONV_BF16): E < norm_cases.bar(E_ref) - the
                              family's tight bound is asserted next to it for k_conv_h16, whose fair case of the kind has no flip on the CPU and
                              (the affine is the same two IEEE roundings in k_gn_apply_h16) none on the GPU
    statistics                the returned coefficients against float64 statistics of the stored tensor: 2e-6 max|A|, 2e-6 max(1, |B|max)
                                                                                                     (test_conv_h2s_tiles_group_statistics)
Every case: the output sits inside a buffer of sentinels with one image row of guard on either side, which must come back bit-identical; the
scratch is exactly the queried bytes; the same call twice gives the same bits; and where the path is exact under a power-of-two scale (every
fp32 kernel, and the fp16x2 ones by design) x 2^-10 scales the output bit for bit (without bias, coefficients and residual, which break the
linearity).  Measured on MI355X: the forward table in DESIGN.md."""
import ctypes

import pytest
import torch

from tests import conv_fwd_cases as cf
from tests import norm_cases as nc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

SENTINEL = -7.0


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _device_operands(c):
    o = cf.operands(c)
    d = {k: (None if v is None else v.to(dev)) for k, v in o.items() if k not in ("x", "res")}
    d["x"] = nhwc(o["x"]).to(dev)
    d["res"] = None if o["res"] is None else nhwc(o["res"]).to(dev)
    return d


def _call(c, mode, o, stats=False):
    """One call into a y that lives inside a larger buffer of SENTINELs -> y (N, Cout, Ho, Wo) on the CPU; with stats through hl_conv2d_nhwc_gn
    -> (y, next_coefA, next_coefB, slots used)."""
    from humanliff_amd import _lib
    L = _lib.lib()
    Ho, Wo = cf.out_hw(c)
    guard, n = Wo * c.Cout, c.N * Ho * Wo * c.Cout
    buf = torch.full((guard + n + guard,), SENTINEL, device=dev)
    y = buf[guard:guard + n].view(c.N, Ho, Wo, c.Cout)
    gn = int(o["A"] is not None)
    geom = (c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.ups, gn)
    need = (L.hl_conv2d_gn_scratch_bytes if stats else L.hl_conv2d_scratch_bytes)(mode, *geom)
    assert need > 0 and need % 4 == 0
    scratch = torch.empty(need // 4, device=dev)
    p = _lib.ptr
    front = (mode, p(o["x"]), c.N, c.H, c.W, c.Cin, p(o["w"]), p(o["b"]), c.Cout, c.ks, c.stride, c.ups, p(o["A"]), p(o["B"]), c.silu if gn else 0, p(o["res"]), p(y))
    with _lib.on(dev):
        if stats:
            nA, nB = torch.full((c.N, c.Cout), SENTINEL, device=dev), torch.full((c.N, c.Cout), SENTINEL, device=dev)
            used = ctypes.c_int(-1)
            _lib.check(L.hl_conv2d_nhwc_gn(*front, p(o["gamma"]), p(o["beta"]), p(nA), p(nB), ctypes.byref(used), p(scratch), need, _lib.stream_ptr()), "hl_conv2d_nhwc_gn")
        else:
            _lib.check(L.hl_conv2d_nhwc_mode(*front, p(scratch), need, _lib.stream_ptr()), "hl_conv2d_nhwc_mode")
    torch.cuda.synchronize()
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), "wrote outside y"
    assert bool(torch.isfinite(y).all()) and not bool((y == SENTINEL).any())
    got = nchw(y.cpu())
    return (got, nA.cpu(), nB.cpu(), used.value) if stats else got


def _errors(got, want):
    d = got.double() - want
    return float(d.abs().max()), float(d.pow(2).mean().sqrt()), float(d.norm() / want.norm())


@pytest.mark.parametrize("name", sorted(cf.CASES))
def test_forward_matches_float64_on_its_kernel(name):
    from humanliff_amd import _lib
    c = cf.CASES[name]
    mode, direct_mode = cf.mode_number(c.mode), _lib.HL_CONV_FP32_DIRECT
    r = cf.reference(c)
    o = _device_operands(c)
    want_stats = c.stats is not None
    first = _call(c, mode, o, want_stats)
    again = _call(c, mode, o, want_stats)
    got = first[0] if want_stats else first
    e, rms, rel = _errors(got, r["want"])
    line = (f"{name} ({c.kernel}{'' if c.tile is None else ' tile %d' % c.tile}, {c.gn}{', split-K' if c.split else ''}, {c.arith}, {c.mode}): |y|max {r['scale']:.2f}  "
            f"E {e:.2e}  rms {rms:.2e}  rel-L2 {rel:.2e}  E_ref {r['e_ref']:.2e}")

    # the same call again: the same bits (the statistics and their coefficients too)
    assert torch.equal(again[0] if want_stats else again, got), "two runs differ"
    if want_stats:
        assert torch.equal(again[1], first[1]) and torch.equal(again[2], first[2]) and again[3] == first[3]

    sixteen = cf.rounding(c) is not None
    direct = None
    if c.kernel not in ("k_conv", "k_conv_dma") and not sixteen:          # (the direct kernels are their own yardstick)
        direct = _call(c, direct_mode, o)
        e_d, rms_d, rel_d = _errors(direct, r["want"])
        line += f"  E_direct {e_d:.2e}  rms_direct {rms_d:.2e}  rel-L2_direct {rel_d:.2e}"
    if sixteen:
        _, _, rel_exact = _errors(got, r["exact"])
        line += f"  rel-L2 against the unrounded result {rel_exact:.2e}"
    print(line)

    unit = max(1.0, r["scale"])
    if c.kernel in ("k_conv", "k_conv_dma"):
        assert e < 2e-5 * unit, line
    elif c.kernel == "k_conv_wino":
        assert not torch.equal(got, direct), "the Winograd kernel did not run"
        assert e < 2e-5 * unit and e < 8 * e_d + 1e-6, line
    elif c.kernel in ("k_conv_wino4", "k_conv_wino4w"):
        assert not torch.equal(got, direct), "the Winograd kernel did not run"
        assert e < 4e-5 * unit and rms < 8 * rms_d + 1e-7, line
    elif c.arith == "bf16x3":
        assert not torch.equal(got, direct), "the bf16x3 kernel did not run"
        assert e < 2e-5 * unit and e < 4 * e_d + 1e-6, line
    elif c.arith == "bf16w2":
        assert e < nc.bar(r["e_ref"]), line
    elif c.kernel == "k_conv_h16":
        if cf.flips(c):
            assert e < nc.bar(r["e_ref"]), line
        assert (e < 5e-5 and rel < 2e-6) if c.split else (e < 2e-5 and rel < 1e-6), line      # (the tight bound holds behind the pre-pass too)
    elif c.kernel in cf.FP16X2:
        assert not torch.equal(got, direct), "the fp16x2 kernel did not run"
        assert rel <= 1.3 * rel_d + 5e-8 and e < 2e-5 * unit, line
    else:
        raise KeyError(c.kernel)
    if direct is not None:
        assert e_d < 2e-5 * unit, line                                     # (the twin is a direct kernel: its own bound)
    if sixteen:
        assert rel_exact > 1e-5, line                                      # 16-bit arithmetic ran (the fp32 kernels sit at 1e-7)

    if want_stats:
        _, nA, nB, used = first
        plan = cf.case_plan(c)
        assert used == plan["stat_slots"] and (used > 0) == (c.stats != "none"), (used, plan)
        # whoever adds them (the epilogue, the finish, or the consumer from the tensor): the statistics of the STORED tensor
        yd = got.double().reshape(c.N, 32, -1)
        mean, var = yd.mean(dim=2), yd.var(dim=2, unbiased=False)
        cg = c.Cout // 32
        wantA = ((1.0 / torch.sqrt(var + 1e-5))[:, :, None] * cf.operands(c)["gamma"].double().reshape(1, 32, cg)).reshape(c.N, c.Cout)
        wantB = cf.operands(c)["beta"].double()[None] - mean[:, :, None].expand(c.N, 32, cg).reshape(c.N, c.Cout) * wantA
        eA, eB = float((nA.double() - wantA).abs().max()), float((nB.double() - wantB).abs().max())
        print(f"    statistics by {c.stats}, {used} slots: A {eA:.2e} of max {float(wantA.abs().max()):.2f}, B {eB:.2e} of max {float(wantB.abs().max()):.2f}")
        assert eA < 2e-6 * float(wantA.abs().max()) and eB < 2e-6 * max(1.0, float(wantB.abs().max()))

    # every operation on these paths is a multiply, an add or a round-to-nearest far from under- and overflow (the fp16x2 kernels scale their
    # planes by the image's own power of two), so a power-of-two scale of x goes through bit for bit
    if c.arith in ("fp32", "fp16x2"):
        bare = dict(o, b=None, A=None, B=None, res=None)
        base = got if (o["b"] is None and o["A"] is None and o["res"] is None and not want_stats) else _call(c, mode, bare)
        s = 2.0 ** -10
        assert torch.equal(_call(c, mode, dict(bare, x=o["x"] * s)), base * s), "a 2^-10 scale of x changed the bits of y"
