"""The renderer's gradient reductions against float64 at their edges, each called alone through the C ABI:

  hl_render_weight_grads         (k_wgrad, k_wgrad_finish)                          all 14 MLP parameter gradients
  hl_render_plane_grads          (k_df_transpose, k_plane_scatter)                  the transposed tri-plane lookup, points on rays
  hl_render_plane_grads_points   (k_df_transpose, k_block_bbox, k_plane_scatter_pts) the same for given points

Inputs: tests/render_reduction_cases.py; the right answers: tests/render_reduction_restatement.py (pinned in test_render_reductions_cpu.py).
Both stages state an exactness property - order-free 64-bit fixed point in the scatter, exact three-way bf16 splits in the weight
gradient - so the exact families demand EQUALITY with float64: one dropped, doubled or misplaced contribution fails them, where the
training-step tests' bar (2e-4 of the tensor's maximum) would not notice.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import render_reduction_cases as rc
from tests import render_reduction_restatement as rr

pytestmark = pytest.mark.gpu


def _L():
    from humanliff_amd import _lib
    return _lib


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _scratch(n_bytes):
    return torch.empty(n_bytes // 4 + 1, dtype=torch.float32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------- weight gradients

def _weight_grads(delta, act, n_cols, init=None, expect_rc=0, stride=None, null=None):
    """hl_render_weight_grads on device matrices -> {name: float64 CPU tensor of what the call ADDED}; `init` = the tensors' contents before."""
    _lib = _L()
    L = _lib.lib()
    a, d = C.c_int(), C.c_int()
    L.hl_render_train_rows(C.byref(a), C.byref(d))
    assert (a.value, d.value) == (rr.ACT_ROWS, rr.DEL_ROWS) == (act.shape[0], delta.shape[0])
    stride = delta.shape[1] if stride is None else stride
    assert delta.is_contiguous() and act.is_contiguous() and act.shape[1] == delta.shape[1]
    shapes = rr.grad_shapes()
    init = {n: torch.zeros(s) for n, s in shapes.items()} if init is None else init
    grads = {n: init[n].clone().cuda() for n in rr.GRAD_NAMES}
    ptrs = [None if n == null else C.c_void_p(grads[n].data_ptr()) for n in rr.GRAD_NAMES]
    gp = _lib.RenderMlpParams(*ptrs)
    scratch = _scratch(L.hl_render_weight_grads_scratch_bytes(max(n_cols, 32)))
    rcode = L.hl_render_weight_grads(_lib.ptr(delta), stride, _lib.ptr(act), stride, n_cols, C.byref(gp), _lib.ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (rcode == 0) == (expect_rc == 0), (rcode, L.hl_last_error())
    return {n: grads[n].cpu().double() - init[n].double() for n in rr.GRAD_NAMES}, {n: grads[n].cpu() for n in rr.GRAD_NAMES}


@pytest.mark.parametrize("n_cols", sorted(rc.W_EXACT))
def test_weight_grads_of_small_integers_equal_float64(n_cols):
    """Integers in [-8, 8], integer initial gradients: every partial sum in every order is an integer below 2^24 (asserted on the very
    matrices), so the result must EQUAL float64.  Columns past n_cols and the rows of no operand hold 1e30 and must not leak."""
    big = n_cols == rc.W_EXACT_BIG
    delta, act, init = rc.w_exact(n_cols, device="cuda" if big else "cpu")
    assert rc.w_exact_bound(delta, act, n_cols) < 2 ** 24
    want = rr.weight_grads(delta, act, n_cols)              # float64 matmul; the 270 304-column case on the device
    added, final = _weight_grads(delta.cuda(), act.cuda(), n_cols, init)
    for name in rr.GRAD_NAMES:
        w = want[name].cpu()
        assert bool(torch.isfinite(final[name]).all()), name
        bad = (added[name] != w).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} of {w.numel()} elements differ, first at {bad[0].tolist()}: " \
                                 f"added {added[name][tuple(bad[0])].item()} want {w[tuple(bad[0])].item()}"


@pytest.mark.parametrize("mantissa_in_delta", [True, False], ids=["mantissa_in_delta", "mantissa_in_activation"])
def test_weight_grads_single_products_equal_float64(mantissa_in_delta):
    """One (delta row, activation row) pair per column, every weight element of all seven layers once: each is ONE product of a 24-bit
    mantissa and a power of two, which three bf16 planes and the three partial products that involve the power of two carry exactly.
    Catches a lost plane, a row mislabelled in the ragged tiles (27, 155, 64, 1, 3 rows) and the heads' swapped operands.  A bias is a sum of
    at most 155 such values: within nnz x 2^-24 of its sum of magnitudes in any order (adding a zero is exact)."""
    delta, act, drow, arow = rc.w_probe(mantissa_in_delta)
    n = delta.shape[1]
    want = rr.weight_grads(delta, act, n)
    added, _ = _weight_grads(delta.cuda(), act.cuda(), n)
    for name, (d0, d1), _a in rr.WEIGHT_JOBS:
        w, g = want[f"{name}_w"], added[f"{name}_w"]
        bad = (g != w).nonzero()
        assert bad.numel() == 0, f"{name}_w: {bad.shape[0]} of {w.numel()} differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])].item()!r} want {w[tuple(bad[0])].item()!r}"
        d = delta[d0:d1].double()
        bar = (d != 0).sum(1).double() * 2.0 ** -24 * d.abs().sum(1)
        assert bool(((added[f"{name}_b"] - want[f"{name}_b"]).abs() <= bar).all()), f"{name}_b"


@pytest.mark.parametrize("n_cols", rc.W_RANDOM)
def test_weight_grads_of_scaled_normals_against_sequential_float32(n_cols):
    """Normal entries, rows scaled by 2^uniform(-20, 20).  Measure: max over elements of |got - float64| / sum_p |a_p b_p|.  The bar is 8 x the same
    measure of the float32 products accumulated one after the other in float32 on the CPU (six partial products per term with a rounding
    each, three dropped terms of at most 2^-24 |a b|).
    Measured on MI355X: 2.39e-7 against 2.29e-7 at 1056 columns (ratio 1.05), 6.58e-8 against 2.51e-7 at 5152 (ratio 0.26); with the third
    bf16 plane truncated away the ratios are 18.7 and 7.7."""
    delta, act = rc.w_random(n_cols)
    want = rr.weight_grads(delta, act, n_cols)
    scale = rr.weight_abs_sums(delta, act, n_cols)
    seq = rc.sequential_fp32_error(delta, act, n_cols)
    added, _ = _weight_grads(delta.cuda(), act.cuda(), n_cols)
    worst, where = 0.0, None
    for name in rr.GRAD_NAMES:
        assert bool(torch.isfinite(added[name]).all()), name
        e = float(((added[name] - want[name]).abs() / scale[name]).max())
        if e > worst:
            worst, where = e, name
    print(f"\nW-random {n_cols} columns: kernel {worst:.3e} ({where}), sequential float32 {seq:.3e} of sum |a b|: ratio {worst / seq:.2f} (bar 8)")
    assert worst <= 8 * seq          # measured ratios: 1.05 (1056 columns), 0.26 (5152)


def test_weight_grads_refuses_bad_arguments():
    """Host checks: nothing is launched, the gradient tensors keep their contents."""
    delta, act, init = rc.w_exact(1056)
    delta, act = delta.cuda(), act.cuda()
    for kw in (dict(n_cols=1040), dict(n_cols=1056, stride=1024), dict(n_cols=1056, null="views_b"), dict(n_cols=1056, null="pts0_w")):
        n_cols = kw.pop("n_cols")
        added, _ = _weight_grads(delta, act, n_cols, init, expect_rc=1, **kw)
        assert all(bool((v == 0).all()) for v in added.values()), kw


# ------------------------------------------------------------------------------------------------------------------ plane gradients

def _plane_common(case, extra_stride):
    delta = _dev(rc.delta_matrix(case, extra_stride))
    out = torch.full((27, case.H, case.W), float("nan"), dtype=torch.float32, device="cuda")
    return delta, out, _dev(case.bounds)


def _plane_rays(case, extra_stride=0, expect_rc=0, stride=None, Ni=None):
    """hl_render_plane_grads -> (27,H,W) float32 numpy; the output is prefilled with NaN, every call gets its own delta matrix."""
    from humanliff_amd.NeRF.renderer import tile_rows
    _lib = _L()
    L = _lib.lib()
    delta, out, bounds = _plane_common(case, extra_stride)
    ro, rd, nr, fr = _dev(case.rays_o), _dev(case.rays_d), _dev(case.near), _dev(case.far)
    zc = None if case.zc is None else _dev(case.zc)
    zn = _dev(case.zn) if case.zn_rows else tile_rows(_dev(case.zn)).contiguous()
    scratch = _scratch(L.hl_render_plane_grads_scratch_bytes(case.R))
    p = _lib.ptr
    rcode = L.hl_render_plane_grads(case.H, case.W, p(bounds), p(ro), p(rd), p(nr), p(fr), p(zc), p(zn), case.zn_rows, case.R, case.N,
                                    case.Ni if Ni is None else Ni, p(delta), delta.shape[1] if stride is None else stride, p(out), p(scratch),
                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (rcode == 0) == (expect_rc == 0), (rcode, L.hl_last_error())
    return out.cpu().numpy()


def _plane_points(case, pts, extra_stride=0, expect_rc=0, stride=None, Ni=None):
    """hl_render_plane_grads_points on the given points of the two passes ((R,N,3), (R,Ni,3) float32)."""
    _lib = _L()
    L = _lib.lib()
    delta, out, bounds = _plane_common(case, extra_stride)
    pc, pn = _dev(rc.tile_points(pts[0])), _dev(rc.tile_points(pts[1]))
    scratch = _scratch(L.hl_render_plane_grads_points_scratch_bytes(case.R, case.N, case.Ni))
    p = _lib.ptr
    rcode = L.hl_render_plane_grads_points(case.H, case.W, p(bounds), p(pc), p(pn), case.R, case.N, case.Ni if Ni is None else Ni, p(delta),
                                           delta.shape[1] if stride is None else stride, p(out), p(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (rcode == 0) == (expect_rc == 0), (rcode, L.hl_last_error())
    return out.cpu().numpy()


def _call(which, case, pts, **kw):
    return _plane_rays(case, **kw) if which == "rays" else _plane_points(case, pts, **kw)


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    c, y, x = bad[0]
    return f"{bad.shape[0]} texels differ, first: channel {c} (image {c // 3}) texel ({y}, {x}) got {got[c, y, x]!r} want {want[c, y, x]!r}"


@pytest.mark.parametrize("which", ["rays", "points"])
def test_plane_grads_of_dyadic_points_equal_float64(which):
    """Axis-aligned rays with dyadic origins, directions and depths at 32x32 in [-1,1]^3, integer deltas: every weight is a multiple of
    1/16 and every sum exact in fixed point and in float32, so the output must EQUAL the restatement (which equals float64 autograd
    through plane_features: test_render_reductions_cpu.py).  Points at texel centres, half a texel outside each edge, more than a texel
    outside, on both sides of and across the 16-texel tile seams in x, y and both, 4 096 points on one texel.  Texels nothing touches
    come back 0 from a NaN-filled output."""
    case, pts, ref = rc.p_reference("exact")
    got = _call(which, case, pts, extra_stride=96 if which == "points" else 0)
    assert not np.isnan(got).any(), "texels left unwritten (or NaN)"
    want = ref["want"]
    assert np.array_equal(got.astype(np.float64), want), _first_difference(got.astype(np.float64), want)
    assert np.all(got[np.repeat(ref["taps"], 3, 0) == 0] == 0)


@pytest.mark.parametrize("rn", rc.P_RANDOM_RAYS, ids=lambda v: "R%d-N%d-Ni%d" % v)
@pytest.mark.parametrize("hw", rc.P_RANDOM_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("which", ["rays", "points"])
def test_plane_grads_of_random_rays_within_the_contract(which, hw, rn):
    """Random rays through a non-unit box from 2 and 8 box widths away (the points call: the same points bent off their rays); coarse
    depths NULL or stratified rows, new depths rows or tile-major; deltas +-2^uniform(-20, 0).  Per texel
        |got - want| <= 2^-24 |want| + taps(texel) x 2^-43 x max |delta|
    - float32's rounding of the sum plus the header's fixed-point unit per contribution.  Nothing else is allowed: a sample culled by the
    depth interval or a block's bounding box, or a tap lost at a tile seam, is a whole contribution."""
    case, pts, ref = rc.p_reference(which, hw, rn)
    got = _call(which, case, pts, extra_stride=0 if which == "points" else 64).astype(np.float64)
    assert not np.isnan(got).any(), "texels left unwritten (or NaN)"
    bar = rc.p_random_bar(case, ref)
    err = np.abs(got - ref["want"])
    touched = bar > 0
    frac = float((err[touched] / bar[touched]).max()) if touched.any() else 0.0
    print(f"\nP-random {which} {hw} {rn}: {int(ref['taps'].sum())} taps, largest error {frac:.4f} of its bar")
    assert np.all(got[~touched] == 0)
    assert np.all(err <= bar), _first_difference(np.where(err <= bar, ref["want"], got), ref["want"])


_PROPERTY_CASES = [((24, 40), (600, 130, 70)), ((40, 40), (70, 65, 3))]


@pytest.mark.parametrize("hw, rn", _PROPERTY_CASES, ids=["600rays", "70rays"])
def test_plane_grads_bits_do_not_depend_on_run_order_or_entry_point(hw, rn):
    """Fixed point is order-free: a second run, the rays permuted together with their delta columns, and hl_render_plane_grads_points fed the
    float32 points o + d z all give the same BITS; any difference is a culling error.  All-zero deltas give zeros, not NaN."""
    case, pts, _ = rc.p_reference("rays", hw, rn)
    first = _plane_rays(case)
    assert np.array_equal(first.view(np.uint32), _plane_rays(case, extra_stride=32).view(np.uint32)), "two runs differ"
    perm = np.random.default_rng(9).permutation(case.R)
    again = _plane_rays(case.permuted(perm))
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), "permuted rays: " + _first_difference(again, first)
    by_points = _plane_points(case, pts)
    assert np.array_equal(first.view(np.uint32), by_points.view(np.uint32)), "points entry: " + _first_difference(by_points, first)
    by_points = _plane_points(case.permuted(perm), tuple(p[perm] for p in pts))
    assert np.array_equal(first.view(np.uint32), by_points.view(np.uint32)), "points entry, permuted: " + _first_difference(by_points, first)
    zero = case.with_deltas(np.zeros_like(case.delta_c), np.zeros_like(case.delta_n))
    for got in (_plane_rays(zero), _plane_points(zero, pts)):
        assert np.array_equal(got, np.zeros_like(got))


@pytest.mark.parametrize("which", ["rays", "points"])
def test_plane_grads_refuse_bad_arguments(which):
    """Host checks: a delta stride below the padded column count, n_importance = 0.  Nothing is launched: the output keeps its NaN fill."""
    case, pts, _ = rc.p_reference("rays", (40, 40), (70, 65, 3))
    cols = 3 * 32 * (case.N + case.Ni)
    for kw in (dict(stride=cols - 32), dict(stride=case.R * (case.N + case.Ni)), dict(Ni=0)):
        got = _call(which, case, pts, expect_rc=1, **kw)
        assert np.isnan(got).all(), kw
