"""tests/conv_bwd_cases.py on the CPU: every backward-data case reaches the kernel it was written for (hl_conv2d_bwd_data_plan is host
arithmetic: no GPU), the cases cover every (mode, kernel size, kernel, split or not) the plan can answer on the stated grid, every case is
fair (fp32 CPU autograd on the same operands within E_REF_MAX of float64), the query refuses what the call refuses, and a stride-2
convolution of an odd size is refused before anything is launched."""
import ctypes
import itertools

import pytest
import torch

from tests import conv_bwd_cases as cb


def _mode(name):
    from humanliff_amd import _lib
    return {"fp32": _lib.HL_CONV_FP32, "bf16": _lib.HL_CONV_BF16, "fp16": _lib.HL_CONV_FP16}[name]


def _plan(mode, *args):
    """(status, kernel name, split-K slabs) of hl_conv2d_bwd_data_plan(mode, N, Ho, Wo, Cy, Cout, Cin, ks, stride, ups, Cx)."""
    from humanliff_amd import _lib
    k, s = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().hl_conv2d_bwd_data_plan(mode, *args, ctypes.byref(k), ctypes.byref(s))
    return rc, cb.KERNELS.get(k.value), s.value


@pytest.mark.parametrize("name", sorted(cb.CASES))
def test_case_reaches_the_kernel_it_was_written_for(name):
    c = cb.CASES[name]
    rc, kernel, splits = _plan(_mode(c.mode), *cb.abi_args(c))
    assert rc == 0
    assert (kernel, splits > 1) == (c.kernel, c.split), (name, kernel, splits)


def test_cases_cover_every_plan_the_grid_reaches():
    g = cb.GRID
    reached = set()
    for mode, ks, N, (H, W), Cy, Cin in itertools.product(g["modes"], g["ks"], g["N"], g["sizes"], g["channels"], g["channels"]):
        rc, kernel, splits = _plan(_mode(mode), N, H, W, Cy, Cy, Cin, ks, 1, 0, Cin)
        assert rc == 0, (mode, ks, N, H, W, Cy, Cin)
        reached.add((mode, ks, kernel, splits > 1))
    covered = {(c.mode, c.ks, c.kernel, c.split) for c in cb.CASES.values()}
    assert reached - covered == set(), "plans of the grid without a case"
    assert covered - reached == set(), "cases on plans the grid does not reach"
    universe = {(m, ks, k, sp) for m in cb.MODES for ks in (3, 1) for k in cb.MODE_KERNELS[m] for sp in (False, True) if ks == 3 or "wino" not in k}
    assert reached <= universe
    assert universe - reached == set(cb.UNREACHABLE), (sorted(universe - reached - set(cb.UNREACHABLE)), sorted(set(cb.UNREACHABLE) & reached))


@pytest.mark.parametrize("name", sorted(cb.CASES))
def test_case_is_fair(name):
    c = cb.CASES[name]
    r = cb.reference(c)
    H, W = cb.x_hw(c)
    assert tuple(r["want"].shape) == (c.N, c.Cin, H, W) and r["want"].dtype == torch.float64
    print(f"{name}: |dx|max {r['scale']:.3f}, E_ref {r['e_ref']:.2e} ({r['e_ref'] / r['scale']:.2e} of it)")
    assert 0.5 < r["scale"] < 20.0                                    # dx is O(1)
    assert r["e_ref"] < cb.E_REF_MAX * r["scale"]
    if cb.rounding(c) is not None:                                    # the rounding is visible, and it is a rounding
        rel = float((r["want"] - r["exact"]).norm() / r["exact"].norm())
        assert 1e-5 < rel < 1e-2, rel


def test_bf16_planes_are_the_two_leading_truncated_planes():
    """cb.bf16_planes2 against the split written out by hand: hi = the upper 16 bits, mid = the upper 16 bits of the (exact) rest."""
    e = lambda k: 2.0 ** -k  # noqa: E731
    #                 one plane holds it       both planes hold it (the second: 8 bits from its leading one)    cut below that, towards zero
    w = torch.tensor([1.0, -1.0, 1.0 + e(7), 1.0 + e(8), 1.0 + e(8) + e(15), 1.0 + e(8) + e(16), -(1.0 + e(8) + e(15) + e(23)), 0.0])
    want = torch.tensor([1.0, -1.0, 1.0 + e(7), 1.0 + e(8), 1.0 + e(8) + e(15), 1.0 + e(8), -(1.0 + e(8) + e(15)), 0.0])
    assert torch.equal(cb.bf16_planes2(w), want)
    # a run of zero bits after the first plane moves the second plane down: 1 + 2^-12 + 2^-19 keeps all three bits (mid = 2^-12 (1 + 2^-7))
    assert torch.equal(cb.bf16_planes2(torch.tensor([1.0 + e(12) + e(19)])), torch.tensor([1.0 + e(12) + e(19)]))
    g = torch.Generator().manual_seed(3)
    w = torch.randn(4096, generator=g) * 0.05
    p2 = cb.bf16_planes2(w)
    assert bool((p2.abs() <= w.abs()).all()) and bool(((w - p2).abs() < w.abs() * 2.0 ** -15).all()) and not torch.equal(p2, w)


def test_plan_query_refuses_what_the_call_refuses():
    from humanliff_amd import _lib
    L = _lib.lib()
    good = dict(mode=_lib.HL_CONV_FP32, N=2, Ho=8, Wo=8, Cy=64, Cout=64, Cin=64, ks=3, stride=1, ups=0, Cx=64)
    order = ("N", "Ho", "Wo", "Cy", "Cout", "Cin", "ks", "stride", "ups", "Cx")

    def both(**kw):
        a = dict(good, **kw)
        rc, _, _ = _plan(a["mode"], *(a[k] for k in order))
        need = L.hl_conv2d_bwd_data_scratch_bytes(a["mode"], *(a[k] for k in order))
        return rc, need
    assert both()[0] == 0 and both()[1] > 0
    assert both(stride=2)[0] == 0 and both(ups=1)[0] == 0 and both(Cin=27, Cx=32)[0] == 0 and both(Cout=27)[0] == 0
    # the refusals of hl_conv2d_nhwc_bwd_data, one argument each (the call itself cannot run here: it checks these before its pointers)
    bad = [dict(mode=_lib.HL_CONV_BF16X3), dict(mode=_lib.HL_CONV_FP32_MFMA), dict(mode=99), dict(Cy=72, Cout=72), dict(Cout=80), dict(Cin=80),
           dict(ks=5), dict(ks=2), dict(stride=3), dict(stride=0), dict(stride=2, ups=1), dict(stride=2, ks=1), dict(ups=1, Cin=27, Cx=27), dict(ups=1, Ho=7), dict(ups=1, Wo=9),
           dict(N=0), dict(Ho=0), dict(Wo=-8), dict(Cin=0, Cx=0), dict(Cy=0, Cout=0)]
    for kw in bad:
        rc, _ = both(**kw)
        assert rc == -1, kw
        assert b"hl_conv2d_bwd_data_plan" in L.hl_last_error(), kw
    k = ctypes.c_int(0)
    assert L.hl_conv2d_bwd_data_plan(good["mode"], *(good[n] for n in order), None, ctypes.byref(k)) == -1
    # the size query says 0 for exactly those: the call, its size and its plan read one statement of the arguments
    for kw in bad:
        assert both(**kw) == (-1, 0), kw


def test_stride2_convolution_of_an_odd_size_is_refused_before_any_launch():
    """hl_conv2d_nhwc_bwd_data stores the whole zero-stuffed (2Ho, 2Wo) grid: for odd H that is one row more than dx has.  _Conv refuses the
    forward, so no backward of such a layer exists.  (CPU tensors: the refusal comes before the library is asked for anything.)"""
    from humanliff_amd.improved_diffusion import unet_train as ut
    w, b = torch.zeros((16, 16, 3, 3)), torch.zeros(16)
    for shape in ((1, 5, 6, 16), (1, 6, 5, 16), (2, 7, 9, 16)):
        with pytest.raises(ValueError, match=str(shape).replace("(", r"\(").replace(")", r"\)")):
            ut._Conv.apply(torch.zeros(shape), w, b, 2, 0)
