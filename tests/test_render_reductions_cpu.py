"""tests/render_reduction_restatement.py pinned without a GPU, and the conditions tests/render_reduction_cases.py promises to
tests/test_render_reductions_gpu.py: the plane restatement equals float64 autograd through oracle.render_oracle.plane_features (exactly on
dyadic inputs; to 1e-5 of a texel's sum of |contributions| on dense random points: float32 coordinates; to 1e-12 on the GPU tests' own random
inputs when its statements run in float64: there a texel may rest on one tap of vanishing weight), the weight restatement equals torch.einsum in
float64, the exact families are exact (integer sums below 2^24, float32 == float64 texel coordinates), the probe columns are what they claim."""
import numpy as np
import pytest
import torch

from tests import render_reduction_cases as rc
from tests import render_reduction_restatement as rr


# ---------------------------------------------------------------------------------------------------------------- weight gradients

def test_weight_restatement_is_einsum_over_the_headers_row_ranges():
    from humanliff_amd import _lib
    import ctypes
    a, d = ctypes.c_int(), ctypes.c_int()
    _lib.lib().hl_render_train_rows(ctypes.byref(a), ctypes.byref(d))
    assert (a.value, d.value) == (rr.ACT_ROWS, rr.DEL_ROWS)
    delta, act = rc.w_random(1056)
    got = rr.weight_grads(delta, act, 1056)
    D, A = delta[:, :1056].double(), act[:, :1056].double()
    want = {"pts0_w": (D[0:128], A[0:27]), "pts1_w": (D[128:256], A[155:283]), "pts2_w": (D[256:384], A[0:155]), "feat_w": (D[384:512], A[283:411]),
            "views_w": (D[512:576], A[411:566]), "alpha_w": (D[576:577], A[283:411]), "rgb_w": (D[577:580], A[566:630])}
    assert set(got) == set(rr.GRAD_NAMES) and list(got) == list(rr.GRAD_NAMES)
    for name, (dd, aa) in want.items():
        w = torch.einsum("ip,np->in", dd, aa)
        assert got[name].shape == rr.grad_shapes()[name] == tuple(w.shape)
        scale = torch.einsum("ip,np->in", dd.abs(), aa.abs())
        assert float(((got[name] - w).abs() / scale).max()) < 1e-13, name
        b = name[:-1] + "b"
        assert got[b].shape == rr.grad_shapes()[b]
        assert float(((got[b] - dd.sum(1)).abs() / dd.abs().sum(1)).max()) < 1e-13, b
    assert sum(int(np.prod(s)) for s in rr.grad_shapes().values()) == 66884        # the MLP's parameter count


@pytest.mark.parametrize("n_cols", sorted(rc.W_EXACT))
def test_w_exact_sums_are_integers_below_2_24(n_cols):
    delta, act, init = rc.w_exact(n_cols)
    stride = rc.W_EXACT[n_cols]
    assert delta.shape == (rr.DEL_ROWS, stride) and act.shape == (rr.ACT_ROWS, stride) and stride >= n_cols
    used_d, used_a = delta[:rr.DF_ROW0, :n_cols], act[:, :n_cols]
    for m in (used_d, used_a):
        assert float(m.abs().max()) == 8.0 and bool((m == m.round()).all())
    assert bool((delta[rr.DF_ROW0:] == rc.BIG).all()) and bool((delta[:, n_cols:] == rc.BIG).all()) and bool((act[:, n_cols:] == rc.BIG).all())
    for name, v in init.items():
        assert v.shape == rr.grad_shapes()[name] and bool((v != 0).all()) and bool((v == v.round()).all())
    bound = rc.w_exact_bound(delta, act, n_cols)
    print(f"n_cols {n_cols}: bound of every partial sum {bound:.0f} = 2^{np.log2(bound):.2f}")
    assert bound < 2 ** 24
    if n_cols <= 5152:                                                   # the bound bounds: the actual largest sum of |products|
        s = rr.weight_abs_sums(delta, act, n_cols)
        assert max(float(v.max()) for v in s.values()) + 8 <= bound


def test_w_exact_strides_cover_both_layouts():
    assert sorted(rc.W_EXACT) == [32, 1024, 1056, 3072, 5152, 270304]
    assert {s - n for n, s in rc.W_EXACT.items()} == {0, 96}


@pytest.mark.parametrize("mantissa_in_delta", [True, False])
def test_w_probe_columns_hold_one_distinct_pair(mantissa_in_delta):
    delta, act, drow, arow = rc.w_probe(mantissa_in_delta)
    n = delta.shape[1]
    assert n == 66304 == 66884 - 580 and n % 32 == 0
    assert len(set(zip(drow.tolist(), arow.tolist()))) == n                              # distinct pairs: every weight element once
    cols = np.arange(n)
    d, a = delta.numpy(), act.numpy()
    assert np.count_nonzero(d) == n and np.count_nonzero(a) == n
    assert np.all(d[drow, cols] != 0) and np.all(a[arow, cols] != 0)                     # one non-zero per column in each matrix
    full, pow2 = (d[drow, cols], a[arow, cols]) if mantissa_in_delta else (a[arow, cols], d[drow, cols])
    mant, _ = np.frexp(pow2.astype(np.float64))
    assert np.all(np.abs(mant) == 0.5) and np.all(np.abs(pow2) >= 2.0 ** -20) and np.all(np.abs(pow2) <= 2.0 ** 20)
    bits = full.view(np.uint32)
    assert np.all(bits & 1 == 1)                                                         # 24 significant bits: the third bf16 plane is needed
    # every pair lies in exactly one job, so the float64 answer is the single product, and float32 holds it
    want = rr.weight_grads(delta, act, n)
    k = 0
    for name, (d0, d1), (a0, a1) in rr.WEIGHT_JOBS:
        w = want[f"{name}_w"].numpy()
        cnt = (d1 - d0) * (a1 - a0)
        inj = (drow >= d0) & (drow < d1)
        assert inj.sum() == cnt and np.all((arow[inj] >= a0) & (arow[inj] < a1))
        prod = d[drow[inj], cols[inj]].astype(np.float64) * a[arow[inj], cols[inj]].astype(np.float64)
        assert np.array_equal(w[drow[inj] - d0, arow[inj] - a0], prod) and np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
        assert np.all(w != 0)
        k += cnt
    assert k == n
    # rows 26 | 27 and 154 | 155 of the ragged tiles and both heads are among the pairs
    pairs = set(zip(drow.tolist(), arow.tolist()))
    assert {(0, 26), (256, 154), (512 + 63, 411 + 154), (576, 283), (576, 410), (577, 566), (579, 629)} <= pairs
    assert (0, 27) not in pairs and (256, 155) not in pairs


def test_sequential_fp32_error_is_a_float32_error():
    delta, act = rc.w_random(1056)
    e = rc.sequential_fp32_error(delta, act, 1056)
    print(f"sequential float32 accumulation, 1056 columns: {e:.3e} of sum |a b| = {e * 2 ** 24:.2f} x 2^-24")
    assert 2.0 ** -26 < e < 64 * 2.0 ** -24
    scale = delta[:rr.DF_ROW0, :1056].abs().max(1).values
    assert float(scale.max() / scale.min()) > 2.0 ** 30                                  # the rows' scales really span the range


# ------------------------------------------------------------------------------------------------------------------ plane gradients

def test_p_exact_is_dyadic_and_contains_its_edge_points():
    case, pts, ref = rc.p_reference("exact")
    H = W = rc.P_EXACT_HW
    assert (case.H, case.W) == (H, W) and np.array_equal(case.bounds, [[-1, -1, -1], [1, 1, 1]])
    P, D = case.flat(pts)
    # the float32 points are the exact points: float64 o + d z from float64 inputs agrees
    zc, zn = case.depths()
    p64 = np.concatenate([(case.rays_o.astype(np.float64)[:, None] + case.rays_d.astype(np.float64)[:, None] * z.astype(np.float64)[..., None]).reshape(-1, 3)
                          for z in (zc, zn)])
    assert np.array_equal(P.astype(np.float64), p64)
    ix32, iy32 = rr.texel_coords(P, case.bounds, H, W, np.float32)
    ix64, iy64 = rr.texel_coords(P, case.bounds, H, W, np.float64)
    assert np.array_equal(ix32.astype(np.float64), ix64) and np.array_equal(iy32.astype(np.float64), iy64)
    assert np.array_equal(ix64 * 4, np.round(ix64 * 4)) and np.array_equal(iy64 * 4, np.round(iy64 * 4))      # multiples of 1/4
    assert np.array_equal(ix64[1] - ix64[0], np.full(P.shape[0], 0.5))                                          # the group shift is half a texel
    assert np.array_equal(D, np.round(D)) and np.abs(D).max() == 8
    for q in range(9):
        x, y = ix64[q], iy64[q]
        inside = (y > 0) & (y < H - 1)
        assert np.any((x == np.round(x)) & (y == np.round(y)) & (x >= 0) & (x <= W - 1) & inside), q               # texel centres
        assert np.any((x == -0.5) & inside) and np.any((x == W - 0.5) & inside), q                                  # one column of taps outside
        assert np.any((y == -0.5) & (x > 0) & (x < W - 1)) and np.any((y == H - 0.5) & (x > 0) & (x < W - 1)), q
        assert np.any(x < -1) and np.any(x > W) and np.any(y < -1) and np.any(y > H), q                             # no tap at all
        for lo, hi in ((14, 15), (15, 16), (16, 17)):                                                                # left of, across, right of the seam
            inx, iny = (x > lo) & (x < hi), (y > lo) & (y < hi)
            assert np.any(inx & inside) and np.any(iny & (x > 0) & (x < W - 1)), (q, lo)
        assert np.any((x > 15) & (x < 16) & (y > 15) & (y < 16)), q                                                  # across both seams at once
    one = (ix64[0] == 7) & (iy64[0] == 20)
    assert one.sum() >= 4096 and ref["taps"][0, 20, 7] >= 4096                                                       # 4 096 points on one texel
    # every sum a multiple of 1/16 that float32 holds, whatever the order
    assert np.array_equal(ref["want"] * 16, np.round(ref["want"] * 16)) and ref["abs"].max() < 2 ** 19
    assert np.any(ref["taps"] == 0)                                                                                  # texels nothing touches


def test_plane_restatement_equals_float64_autograd_on_the_dyadic_case():
    case, pts, ref = rc.p_reference("exact")
    auto = rr.plane_grads_autograd(*case.flat(pts), case.bounds, case.H, case.W)
    assert np.array_equal(ref["want"], auto)
    assert np.all(ref["want"][np.repeat(ref["taps"], 3, 0) == 0] == 0)


_PIN = [("rays", (40, 40), (33, 64, 64)), ("rays", (24, 40), (70, 65, 3)), ("rays", (24, 40), (1, 1, 1)), ("points", (40, 40), (70, 65, 3)),
        ("points", (256, 256), (33, 64, 64))]


@pytest.mark.parametrize("kind, hw, rn", _PIN)
def test_plane_restatement_in_float64_is_float64_autograd(kind, hw, rn):
    """The restatement's statements, run in float64 on the GPU tests' own random inputs, are the transpose of plane_features to rounding.
    (In float32 they differ from it by the coordinates' rounding, 2^-24 x the plane size in texels: printed; on these sparse inputs a texel
    can hold one tap of weight 1e-3, which that moves by 1e-2 of itself, so no 1e-5 bar applies here - see the dense test below.)"""
    case, pts, ref = rc.p_reference(kind, hw, rn)
    P, D = case.flat(pts)
    auto = rr.plane_grads_autograd(P, D, case.bounds, case.H, case.W)
    r64 = rr.plane_grads(P, D, case.bounds, case.H, case.W, np.float64)
    assert r64["taps"].sum() > 0
    touched = r64["abs"] > 0
    err = np.abs(r64["want"] - auto)[touched] / r64["abs"][touched]
    assert err.max() < 1e-12 and np.all(auto[~touched] == 0)
    both = touched & (ref["abs"] > 0)
    e32 = np.abs(ref["want"] - auto)[both] / ref["abs"][both]
    print(f"{kind} {hw} {rn}: float64 statements vs autograd {err.max():.1e}; float32 coordinates: median {np.median(e32):.1e}, max {e32.max():.1e} of sum |contributions|")


@pytest.mark.parametrize("H, W", [(8, 8), (6, 10)])
def test_plane_restatement_is_float64_autograd_to_float32_coordinates(H, W):
    """Random points: within 1e-5 of every texel's sum of |contributions| of float64 autograd; float32 coordinates account for the gap."""
    pts, delta, bounds = rc.p_dense_points(H, W)
    ref = rr.plane_grads(pts, delta, bounds, H, W)
    auto = rr.plane_grads_autograd(pts, delta, bounds, H, W)
    assert ref["taps"].min() >= 100
    err = np.abs(ref["want"] - auto) / ref["abs"]
    print(f"dense random points at {H}x{W}: restatement vs float64 autograd {err.max():.2e} of sum |contributions|")
    assert err.max() < 1e-5


@pytest.mark.parametrize("hw, rn", rc.P_RANDOM)
def test_p_random_cases_are_what_they_claim(hw, rn):
    case = rc.p_random(hw, rn)
    assert (case.H, case.W, case.R, case.N, case.Ni) == (*hw, *rn)
    assert not np.array_equal(case.bounds, [[-1, -1, -1], [1, 1, 1]])
    null_zc, zn_rows = rc.p_random_variant(hw, rn)
    assert (case.zc is None) == null_zc and bool(case.zn_rows) == zn_rows
    b = case.bounds.astype(np.float64)
    width = (b[1] - b[0]).max()
    gap = np.linalg.norm(case.rays_o - b.mean(0), axis=1) / width
    assert np.all((np.abs(gap - 2) < 1.0) | (np.abs(gap - 8) < 1.0)) and (case.R == 1 or (np.any(gap < 3) and np.any(gap > 7)))
    for d in (case.delta_c, case.delta_n):
        assert np.all(np.abs(d) <= 1) and np.all(np.abs(d) >= 2.0 ** -20)
    # the points reach the planes: the case is not empty, and a one-sample pass puts its sample inside the box
    P, _ = case.flat()
    n = 2 * (P - b[0]) / (b[1] - b[0]) - 1
    assert np.any(np.all(np.abs(n) < 1, axis=1))
    if case.N == 1:
        assert np.all(np.abs(n[:case.R]) < 1)


def test_p_random_variants_cover_every_combination():
    seen = {rc.p_random_variant(hw, rn) for hw, rn in rc.P_RANDOM}
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    for rn in rc.P_RANDOM_RAYS:
        assert len({rc.p_random_variant(hw, rn) for hw in rc.P_RANDOM_HW}) == 3
    for hw in rc.P_RANDOM_HW:
        assert len({rc.p_random_variant(hw, rn) for rn in rc.P_RANDOM_RAYS}) == 4


def test_p_random_points_leave_their_rays():
    case, pts = rc.p_random_points((40, 40), (70, 65, 3))
    straight = case.points()
    ext = case.bounds[1] - case.bounds[0]
    for a, b in zip(pts, straight):
        assert a.dtype == np.float32 and a.shape == b.shape
        off = np.abs(a - b) / ext
        assert off.max() < 0.06 and off.mean() > 0.005


def test_tile_layouts():
    rows = np.arange(70 * 3 * 2, dtype=np.float32).reshape(70, 3, 2)
    t = rc.tile_columns(rows)
    assert t.shape == (2, 3 * 3 * 32)
    for r, s, k in ((0, 0, 0), (31, 2, 1), (32, 0, 0), (69, 1, 1)):
        assert t[k, ((r // 32) * 3 + s) * 32 + r % 32] == rows[r, s, k]
    assert np.all(t[:, (2 * 3 + 0) * 32 + 6:(2 * 3 + 0) * 32 + 32] == 0)                  # padding rays: zero
    from humanliff_amd.NeRF.renderer import tile_rows
    z = torch.arange(70 * 3, dtype=torch.float32).view(70, 3)
    assert np.array_equal(tile_rows(z).numpy()[:2 * 3 * 32 + 6], rc.tile_columns(z.numpy()[:, :, None])[0][:2 * 3 * 32 + 6])
    p = rc.tile_points(np.ones((33, 2, 3), np.float32))
    assert p.shape == (2, 2, 32, 4) and np.all(p[0, :, :, :3] == 1) and np.all(np.isnan(p[..., 3])) and np.all(np.isnan(p[1, :, 1:]))


def test_linspace_depths_of_one_sample_is_near():
    z = rr.linspace_depths([2.0, 3.0], [4.0, 9.0], 1)
    assert np.array_equal(z, [[2.0], [3.0]])
    z = rr.linspace_depths([2.0], [4.0], 5)
    assert np.array_equal(z, [[2.0, 2.5, 3.0, 3.5, 4.0]])
    for n in (1, 2, 3, 64, 65, 130):                                      # torch's own values to the last bit or the one next to it
        t = torch.linspace(0.0, 1.0, n, dtype=torch.float32).numpy()
        mine = rr.linspace01(n)
        assert mine.dtype == np.float32 and mine[0] == 0 and (n == 1 or mine[-1] == 1)
        assert np.abs(mine - t).max() <= 2.0 ** -24
