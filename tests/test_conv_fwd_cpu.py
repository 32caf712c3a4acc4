"""tests/conv_fwd_cases.py on the CPU: every forward case launches the kernel instantiation it was written for (hl_conv2d_plan_ex is host
arithmetic: no GPU), the cases cover every instantiation the plan can answer on the stated grid under the seven modes, the instantiations the
grid cannot reach are exactly UNREACHABLE, every case the GPU test runs is fair (the fp32 CPU restatement within E_REF_MAX of float64), and
the size and plan queries refuse what the call refuses."""
import ctypes
import itertools

import pytest
import torch

from tests import conv_fwd_cases as cf


_plan = cf.plan_ex
_case_plan = cf.case_plan


@pytest.mark.parametrize("name", sorted(cf.ALL_CASES))
def test_case_launches_the_instantiation_it_was_written_for(name):
    from humanliff_amd import _lib
    L = _lib.lib()
    c = cf.ALL_CASES[name]
    p = _case_plan(c)
    assert p is not None, L.hl_last_error()
    assert cf.plan_key(c.mode, c.ks, c.stride, c.ups, cf.with_gn(c), c.silu, p) == cf.key(c), (name, p)
    assert cf.STATS_BY[p["stats_by"]] == (c.stats or "none"), (name, p)
    assert (p["stat_slots"] > 0) == (c.stats in ("epilogue", "finish")) and (p["kt_per"] > 0)
    if c.stats is not None:
        assert c.Cout % 32 == 0                                  # (a GroupNorm32 follows)
    # the short query agrees, and both size queries answer
    k, s = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.hl_conv2d_plan(cf.mode_number(c.mode), *cf.abi_args(c), ctypes.byref(k), ctypes.byref(s)) == 0
    assert (k.value, s.value) == (p["kernel"], p["splits"])
    assert L.hl_conv2d_scratch_bytes(cf.mode_number(c.mode), *cf.abi_args(c)) > 0
    assert L.hl_conv2d_gn_scratch_bytes(cf.mode_number(c.mode), *cf.abi_args(c)) > L.hl_conv2d_scratch_bytes(cf.mode_number(c.mode), *cf.abi_args(c))


def test_cases_cover_every_instantiation_the_grid_reaches():
    g = cf.GRID
    reached = set()
    for mode, kind, N, (H, W), Cin, Cout, (gn, silu) in itertools.product(g["modes"], g["kinds"], g["N"], g["sizes"], g["cin"], g["cout"], g["gn"]):
        ks, stride, ups = cf.KINDS[kind]
        if gn and ups:
            continue                                             # (refused: test_queries_refuse_what_the_call_refuses)
        p = _plan(mode, N, H, W, Cin, Cout, ks, stride, ups, gn, silu)
        assert p is not None, (mode, kind, N, H, W, Cin, Cout, gn, silu)
        reached.add(cf.plan_key(mode, ks, stride, ups, gn, silu, p))
    on_grid = {cf.key(c) for c in cf.ALL_CASES.values() if (c.ks, c.stride, c.ups) in [cf.KINDS[k] for k in g["kinds"]]}
    assert reached - on_grid == set(), "instantiations of the grid without a case"
    assert on_grid - reached == set(), "cases on instantiations the grid does not reach"
    assert reached <= cf.UNIVERSE, sorted(reached - cf.UNIVERSE, key=str)
    assert cf.UNIVERSE - reached == set(cf.UNREACHABLE), (sorted(cf.UNIVERSE - reached - set(cf.UNREACHABLE), key=str), sorted(set(cf.UNREACHABLE) & reached, key=str))


def test_every_number_of_the_plan_is_in_a_case_or_unreachable():
    keys = {cf.key(c) for c in cf.ALL_CASES.values()} | set(cf.UNREACHABLE)
    assert {k[0] for k in keys} == set(cf.KERNELS.values())                                     # every ConvKernel (k_conv1_h16 shares k_conv_h16's number)
    assert {k[1] for k in keys if k[0] == "k_conv"} == {0, 1, 2}                                # the three cfgs
    for kernel in ("k_conv_dma", "k_conv_bf3"):
        assert {k[1] for k in keys if k[0] == kernel} == {4, 8}                                 # both tile8 values
    assert {k[5] for k in keys} >= {v for v in cf.PRE.values() if v}                            # every ConvPrePass
    assert {c.stats for c in cf.ALL_CASES.values()} == {None, "none", "epilogue", "finish"}     # both ConvStatsBy values, and a launch that leaves them to the consumer
    # ... and what is DROPPED takes no kernel, pre-pass or arithmetic out of the GPU run
    run = {cf.key(c) for c in cf.CASES.values()}
    assert {k[0] for k in run} == set(cf.KERNELS.values()) and {k[5] for k in run} == {"none", "affine", "affine_silu", "dense", "blocked", "half"}
    assert {(k[0], k[7]) for k in run} == {(k[0], k[7]) for k in keys - set(cf.UNREACHABLE)}
    assert {c.stats for c in cf.CASES.values()} == {None, "none", "epilogue", "finish"}
    for family in set(cf.KERNELS.values()) - {"k_conv", "k_conv_bf3"}:                           # (k_conv and the bf16 planes leave the statistics to the consumer)
        assert any(c.stats in ("epilogue", "finish") for c in cf.CASES.values() if c.kernel == family), family


@pytest.mark.parametrize("name", sorted(cf.ALL_CASES))
def test_case_is_fair(name):
    c = cf.ALL_CASES[name]
    r = cf.reference(c)
    Ho, Wo = cf.out_hw(c)
    assert tuple(r["want"].shape) == (c.N, c.Cout, Ho, Wo) and r["want"].dtype == torch.float64 and r["ref32"].dtype == torch.float32
    print(f"{name}: |y|max {r['scale']:.3f}, E_ref {r['e_ref']:.2e} ({r['e_ref'] / r['scale']:.2e} of it)")
    assert 0.5 < r["scale"] < 30.0                                    # y is O(1)
    if name in cf.DROPPED:                                            # dropped for this, and only the cases that round a GroupNorm output to 16 bits can be
        assert cf.flips(c) and not cf.is_fair(c), "the case is fair: take it out of DROPPED"
        return
    assert r["e_ref"] <= cf.E_REF_MAX * r["scale"]
    if cf.rounding(c) is not None:                                    # the rounding is visible, and it is a rounding
        rel = float((r["want"] - r["exact"]).norm() / r["exact"].norm())
        assert 1e-5 < rel < 1e-2, rel


# (mode, N, H, W, Cin, Cout, ks, stride, ups, with_gn, silu): what conv2d_single refuses
_GOOD = dict(mode="fp32", N=2, H=8, W=8, Cin=64, Cout=64, ks=3, stride=1, ups=0, gn=0, silu=0)
_REFUSED = [dict(ups=1, gn=1), dict(ups=1, gn=1, silu=1), dict(stride=2, ups=1), dict(silu=1), dict(stride=2, ups=1, gn=1), dict(ks=1, stride=2, ups=1),
            dict(mode="direct", N=1, H=16, W=16, Cin=32, Cout=32, ups=1, gn=1),            # 516608 bytes before the queries shared the call's check
            dict(mode="direct", N=1, H=16, W=16, Cin=32, Cout=32, stride=2, ups=1),        # 287232
            dict(stride=0), dict(stride=3), dict(ks=2), dict(ks=5), dict(Cin=24), dict(Cin=0), dict(Cout=0), dict(N=0), dict(H=0), dict(W=-1)]
_ACCEPTED = [dict(), dict(gn=1), dict(gn=1, silu=1), dict(stride=2), dict(ups=1), dict(stride=2, gn=1, silu=1), dict(ks=1), dict(ks=1, stride=2), dict(ks=1, ups=1),
             dict(ks=1, stride=2, gn=1), dict(H=7, W=9, stride=2), dict(Cout=27), dict(Cin=16)]


def _queries(kw):
    from humanliff_amd import _lib
    L = _lib.lib()
    a = dict(_GOOD, **kw)
    geom = (a["N"], a["H"], a["W"], a["Cin"], a["Cout"], a["ks"], a["stride"], a["ups"])
    k, s = ctypes.c_int(-1), ctypes.c_int(-1)
    m = cf.mode_number(a["mode"])
    short = L.hl_conv2d_plan(m, *geom, a["gn"], ctypes.byref(k), ctypes.byref(s))
    return (L.hl_conv2d_scratch_bytes(m, *geom, a["gn"]), L.hl_conv2d_gn_scratch_bytes(m, *geom, a["gn"]), short,
            _plan(a["mode"], *geom, a["gn"], a["silu"]))


@pytest.mark.parametrize("kw", _REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_queries_refuse_what_the_call_refuses(kw):
    from humanliff_amd import _lib
    L = _lib.lib()
    size, size_gn, short, ex = _queries(kw)
    assert ex is None and b"hl_conv2d_plan_ex" in L.hl_last_error()
    if set(kw) != {"silu"}:                                      # (the size queries and the short plan query have no silu to refuse)
        assert (size, size_gn, short) == (0, 0, -1), kw
    # the call itself: refused on its arguments before it looks at a pointer (none is given: nothing is launched)
    a = dict(_GOOD, **kw)
    one = ctypes.c_float(0)
    coef = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p) if a["gn"] else None
    rc = L.hl_conv2d_nhwc_mode(cf.mode_number(a["mode"]), None, a["N"], a["H"], a["W"], a["Cin"], None, None, a["Cout"], a["ks"], a["stride"], a["ups"],
                               coef, coef, a["silu"], None, None, None, 0, None)
    assert rc == -1 and b"hl_conv2d_nhwc: " in L.hl_last_error() and b"scratch too small" not in L.hl_last_error(), L.hl_last_error()


@pytest.mark.parametrize("kw", _ACCEPTED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "plain")
def test_queries_answer_what_the_call_accepts(kw):
    """... 1x1 with stride 2 or behind the upsample included: k_conv / k_conv_dma / k_conv_bf3 index the input for any ks, and the plan sends
    such a layer nowhere else."""
    from humanliff_amd import _lib
    L = _lib.lib()
    size, size_gn, short, ex = _queries(kw)
    assert size > 0 and size_gn > size and short == 0 and ex is not None, kw
    a = dict(_GOOD, **kw)
    if a["ks"] == 1 and (a["stride"] == 2 or a["ups"]):
        for mode, Cin, Cout, N, hw in itertools.product(cf.MODES, (48, 96, 768), (64, 192, 768), (1, 4), (16, 64)):
            p = _plan(mode, N, hw, hw, Cin, Cout, 1, a["stride"], a["ups"], a["gn"], 0)
            assert cf.KERNELS[p["kernel"]] in ("k_conv", "k_conv_dma", "k_conv_bf3"), (mode, Cin, Cout, N, hw, p)
    # the call gets as far as its scratch check
    rc = L.hl_conv2d_nhwc_mode(cf.mode_number(a["mode"]), None, a["N"], a["H"], a["W"], a["Cin"], None, None, a["Cout"], a["ks"], a["stride"], a["ups"],
                               None, None, 0, None, None, None, 0, None)
    if not a["gn"]:
        assert rc == -1 and b"scratch too small" in L.hl_last_error(), L.hl_last_error()


def test_plan_ex_reports_the_statistics_only_when_asked():
    """want_stats is what hl_conv2d_nhwc_gn sets: without it no launch adds statistics, with it the kernel and the slabs stay the same."""
    for c in (cf.ALL_CASES["dma4_3x3"], cf.ALL_CASES["h2s_3x3_split"]):
        a = (c.mode, c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.ups, int(cf.with_gn(c)), c.silu)
        off, on = _plan(*a, 0), _plan(*a, 1)
        assert off["stats_by"] == 0 and off["stat_slots"] == 0 and on["stats_by"] > 0 and on["stat_slots"] > 0
        assert {k: v for k, v in off.items() if k not in ("stats_by", "stat_slots")} == {k: v for k, v in on.items() if k not in ("stats_by", "stat_slots")}
    from humanliff_amd import _lib
    assert _lib.lib().hl_conv2d_plan_ex(0, 2, 8, 8, 64, 64, 3, 1, 0, 0, 0, 0, None) == -1
