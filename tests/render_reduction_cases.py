"""Seeded inputs of tests/test_render_reductions_{cpu,gpu}.py: the delta / activation matrices of hl_render_weight_grads and the rays, points
and feature deltas of hl_render_plane_grads*.  Every builder is deterministic in its arguments; the conditions a family rests on (integer
sums below 2^24, dyadic coordinates, distinct probe pairs) are asserted by the CPU test, not assumed by the GPU test.

Families ("The renderer's gradient reductions, each alone"):
  w_exact   small integers: every partial sum in every order is an integer below 2^24, so float32 accumulation is exact
  w_probe   one (delta row, activation row) pair per column: every weight element is ONE product of a 24-bit mantissa and a power of two
  w_random  normal entries with per-row scales 2^uniform(-20, 20)
  p_exact   axis-aligned rays with dyadic origins, directions and depths in the box [-1,1]^3 at 32x32: every texel coordinate a multiple of 1/4
  p_random  random rays through a non-unit box
"""
import functools

import numpy as np
import torch

from tests import render_reduction_restatement as rr

BIG = 1.0e30                     # fills whatever the calls must not read: a product of two of them is inf

# ---------------------------------------------------------------------------------------------------------------- weight gradients

# n_cols -> row stride.  Range size 1024 up to 262 144 columns (at most 256 ranges): 32 = one step; 1056 = a second range of one step; 3072 = three
# ranges (k_wgrad_finish's remainder loop only); 5152 = six ranges (one group of four + remainder); 270 304 = range size 1056, 256 ranges, the last short
W_EXACT = {32: 32, 1024: 1024 + 96, 1056: 1056, 3072: 3072 + 96, 5152: 5152, 270304: 270304 + 96}
W_EXACT_BIG = 270304
W_RANDOM = (1056, 5152)


def _fill_unread(delta, act, n_cols):
    delta[:, n_cols:] = BIG
    act[:, n_cols:] = BIG
    delta[rr.DF_ROW0:] = BIG     # rows outside the fourteen operands (every activation row belongs to one)


def w_exact(n_cols, device="cpu"):
    """-> delta (634, stride), act (630, stride), init {name: tensor}: integers in [-8, 8]; initial gradients non-zero integers."""
    stride = W_EXACT[n_cols]
    g = torch.Generator(device=device).manual_seed(1000 + n_cols)
    delta = torch.randint(-8, 9, (rr.DEL_ROWS, stride), generator=g, device=device, dtype=torch.int8).float()
    act = torch.randint(-8, 9, (rr.ACT_ROWS, stride), generator=g, device=device, dtype=torch.int8).float()
    _fill_unread(delta, act, n_cols)
    gi = torch.Generator().manual_seed(2000 + n_cols)
    init = {}
    for name, shape in rr.grad_shapes().items():
        v = torch.randint(1, 9, shape, generator=gi).float()
        init[name] = v * (torch.randint(0, 2, shape, generator=gi).float() * 2 - 1)
    return delta, act, init


def w_exact_bound(delta, act, n_cols):
    """An upper bound of sum_p |delta[i][p] act[n][p]| over every pair of rows (Cauchy-Schwarz: the largest row norms), so of every partial sum
    in every order, plus the largest initial gradient.  Below 2^24 every such sum is an integer float32 holds exactly."""
    dn = delta[:rr.DF_ROW0, :n_cols].pow(2).sum(1, dtype=torch.float64).max().sqrt()
    an = act[:, :n_cols].pow(2).sum(1, dtype=torch.float64).max().sqrt()
    bias = delta[:rr.DF_ROW0, :n_cols].abs().sum(1, dtype=torch.float64).max()
    return float(max(dn * an, bias)) + 8.0


def probe_pairs():
    """Every (delta row, activation row) pair that is a weight element, in the order of WEIGHT_JOBS: 66 304 pairs = 2 072 steps of 32 columns."""
    d, a = [], []
    for _, (d0, d1), (a0, a1) in rr.WEIGHT_JOBS:
        dd, aa = np.meshgrid(np.arange(d0, d1), np.arange(a0, a1), indexing="ij")
        d.append(dd.ravel())
        a.append(aa.ravel())
    return np.concatenate(d), np.concatenate(a)


def w_probe(mantissa_in_delta, seed=0):
    """-> delta, act (rows x 66 304), drow, arow (the pair of each column).  Column p holds delta[drow[p]][p] and act[arow[p]][p] and nothing else.
    One operand is +-m 2^e with m an odd 24-bit integer (bit 23 set: all three bf16 planes are needed), the other +-2^k, k in [-20, 20]."""
    rng = np.random.default_rng(3000 + seed + (1 if mantissa_in_delta else 0))
    drow, arow = probe_pairs()
    n = drow.size
    assert n % 32 == 0
    perm = rng.permutation(n)                # pairs of one job spread over all point ranges
    drow, arow = drow[perm], arow[perm]
    m = (rng.integers(1 << 23, 1 << 24, n) | 1).astype(np.float64)
    full = (m * np.exp2(rng.integers(-8, 9, n) - 23.0) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    pow2 = (np.exp2(rng.integers(-20, 21, n).astype(np.float64)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    delta = np.zeros((rr.DEL_ROWS, n), np.float32)
    act = np.zeros((rr.ACT_ROWS, n), np.float32)
    cols = np.arange(n)
    delta[drow, cols] = full if mantissa_in_delta else pow2
    act[arow, cols] = pow2 if mantissa_in_delta else full
    return torch.from_numpy(delta), torch.from_numpy(act), drow, arow


def w_random(n_cols):
    """-> delta, act: normal entries, each row scaled by 2^uniform(-20, 20); stride n_cols + 96, unread parts BIG."""
    g = torch.Generator().manual_seed(4000 + n_cols)
    stride = n_cols + 96
    delta = torch.randn(rr.DEL_ROWS, stride, generator=g) * torch.exp2(torch.rand(rr.DEL_ROWS, 1, generator=g) * 40 - 20)
    act = torch.randn(rr.ACT_ROWS, stride, generator=g) * torch.exp2(torch.rand(rr.ACT_ROWS, 1, generator=g) * 40 - 20)
    _fill_unread(delta, act, n_cols)
    return delta.contiguous(), act.contiguous()


def sequential_fp32_error(delta, act, n_cols):
    """max over all 14 tensors' elements of |s32 - s64| / sum_p |a_p b_p|, s32 = the float32 products a_p b_p accumulated one after the
    other in float32 (np.cumsum): the yardstick of the W-random bar."""
    d_all = delta[:, :n_cols].numpy()
    a_all = act[:, :n_cols].numpy()
    worst = 0.0
    for _, (d0, d1), (a0, a1) in rr.WEIGHT_JOBS:
        a = a_all[a0:a1]
        for i in range(d0, d1):
            prod = d_all[i][None, :] * a                                        # float32 products
            s32 = np.cumsum(prod, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
            p64 = d_all[i].astype(np.float64)[None, :] * a.astype(np.float64)
            worst = max(worst, float(np.max(np.abs(s32 - p64.sum(1)) / np.abs(p64).sum(1))))
        d = d_all[d0:d1]
        s32 = np.cumsum(d, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        worst = max(worst, float(np.max(np.abs(s32 - d.astype(np.float64).sum(1)) / np.abs(d).astype(np.float64).sum(1))))
    return worst


# ------------------------------------------------------------------------------------------------------------------ plane gradients

class PlaneCase:
    """One call of hl_render_plane_grads: rays, depths and the feature deltas of both passes (rows: ray r, sample s).
    zc None = NULL coarse depths (linspace between near and far); zn_rows: new depths passed as rows or tile-major."""

    def __init__(self, H, W, bounds, rays_o, rays_d, near, far, zc, zn, zn_rows, delta_c, delta_n):
        self.H, self.W = H, W
        self.bounds = np.asarray(bounds, np.float32).reshape(2, 3)
        self.rays_o, self.rays_d = np.asarray(rays_o, np.float32), np.asarray(rays_d, np.float32)
        self.near, self.far = np.asarray(near, np.float32), np.asarray(far, np.float32)
        self.zn = np.asarray(zn, np.float32)
        self.zc = None if zc is None else np.asarray(zc, np.float32)
        self.zn_rows = zn_rows
        self.delta_c, self.delta_n = np.asarray(delta_c, np.float32), np.asarray(delta_n, np.float32)     # (R,N,27), (R,Ni,27)
        self.R, self.N, self.Ni = self.rays_o.shape[0], self.delta_c.shape[1], self.delta_n.shape[1]
        assert self.zn.shape == (self.R, self.Ni) and (self.zc is None or self.zc.shape == (self.R, self.N))

    def depths(self):
        zc = rr.linspace_depths(self.near, self.far, self.N) if self.zc is None else self.zc
        return zc, self.zn

    def points(self):
        """The float32 sample points of the two passes, (R,N,3) and (R,Ni,3)."""
        zc, zn = self.depths()
        return rr.ray_points(self.rays_o, self.rays_d, zc), rr.ray_points(self.rays_o, self.rays_d, zn)

    def flat(self, pts=None):
        """All sample points and their deltas as (M,3), (M,27)."""
        pc, pn = self.points() if pts is None else pts
        return (np.concatenate([pc.reshape(-1, 3), pn.reshape(-1, 3)]),
                np.concatenate([self.delta_c.reshape(-1, 27), self.delta_n.reshape(-1, 27)]))

    def permuted(self, perm):
        zc = None if self.zc is None else self.zc[perm]
        return PlaneCase(self.H, self.W, self.bounds, self.rays_o[perm], self.rays_d[perm], self.near[perm], self.far[perm], zc, self.zn[perm],
                         self.zn_rows, self.delta_c[perm], self.delta_n[perm])

    def with_deltas(self, delta_c, delta_n):
        return PlaneCase(self.H, self.W, self.bounds, self.rays_o, self.rays_d, self.near, self.far, self.zc, self.zn, self.zn_rows, delta_c, delta_n)


def tile_columns(rows):
    """(R, S, K) per-ray values -> (K, ceil(R/32) * S * 32): the tile-major column order [ceil(R/32)][S][32] of one pass, padding rays zero."""
    R, S, K = rows.shape
    tiles = (R + 31) // 32
    buf = np.zeros((tiles * 32, S, K), rows.dtype)
    buf[:R] = rows
    return np.ascontiguousarray(buf.reshape(tiles, 32, S, K).transpose(3, 0, 2, 1)).reshape(K, tiles * S * 32)


def delta_matrix(case, extra_stride=0):
    """The delta matrix of a plane case (634 rows): rows [580,607) hold the feature deltas, columns coarse pass then new depths, padding
    rays zero; every other row and the columns past the padded count are BIG (rows [607,634) are the call's own scratch)."""
    cols = np.concatenate([tile_columns(case.delta_c), tile_columns(case.delta_n)], axis=1)
    m = np.full((rr.DEL_ROWS, cols.shape[1] + extra_stride), BIG, np.float32)
    m[rr.DF_ROW0:rr.DF_ROW0 + 27, :cols.shape[1]] = cols
    return m


def tile_points(pts):
    """(R, S, 3) -> float4 array [ceil(R/32)][S][32][4]; the fourth component and the padding rays are NaN (nothing may read them)."""
    R, S, _ = pts.shape
    tiles = (R + 31) // 32
    buf = np.full((tiles * 32, S, 4), np.nan, np.float32)
    buf[:R, :, :3] = pts
    return np.ascontiguousarray(buf.reshape(tiles, 32, S, 4).transpose(0, 2, 1, 3))


# P-exact: normalised coordinate v -> texel coordinate 16 v + 15.5 (group shift: + 0.5).  Multiples of 1/64 give multiples of 1/4.
P_EXACT_HW = 32
_SPECIAL = [
    -50 / 64, 9 / 32,                                        # texel centres of the unshifted group (ix = 3, 20): weights 1 and 0
    -1.0, 1.0,                                               # ix = -0.5 and W - 0.5: one column of taps outside
    -1.25, 1.25, -69 / 64,                                   # ix = -4.5, 35.5, -1.75: more than one texel outside, no tap
    -3 / 64, -1 / 64, 0.0, 1 / 64, 1 / 32, 3 / 64,           # ix = 14.75 .. 16.25: both sides of the seam 15|16 and across it
    -33 / 32, 31 / 32,                                       # shifted group at ix = -0.5 and W - 0.5
    -5 / 64,                                                 # ix = 14.25: the shifted group left of the seam
]
P_EXACT_ONE_TEXEL = (-17 / 32, 9 / 32)                       # (x, y) of 64 rays x 64 samples along z: 4 096 points on texel (7, 20) of plane 0, group 0


def p_exact():
    rng = np.random.default_rng(5000)
    N, Ni = 40, 24
    grid = lambda n: rng.integers(-70, 71, n) / 64.0
    vo = np.array(_SPECIAL[:13] + [-23 / 64])                # ray origins: 14 x 14 per axis
    vc = np.concatenate([_SPECIAL, grid(N - len(_SPECIAL))])
    vn = np.concatenate([_SPECIAL, grid(Ni - len(_SPECIAL))])
    o, d, zc, zn = [], [], [], []
    for axis in range(3):
        others = [k for k in range(3) if k != axis]
        for a in vo:
            for b in vo:
                # p[axis] = o + d z walks the coordinate list; three dyadic parametrisations of the same walk
                speed, start = [(1.0, -1.5), (2.0, -1.5), (-0.5, 1.5)][len(o) % 3]
                oo, dd = np.zeros(3), np.zeros(3)
                oo[others[0]], oo[others[1]], oo[axis], dd[axis] = a, b, start, speed
                o.append(oo)
                d.append(dd)
                zc.append((rng.permutation(vc) - start) / speed)
                zn.append((rng.permutation(vn) - start) / speed)
    for _ in range(64):
        o.append(np.array([P_EXACT_ONE_TEXEL[0], P_EXACT_ONE_TEXEL[1], -1.5]))
        d.append(np.array([0.0, 0.0, 1.0]))
        zc.append(rng.permutation(vc) + 1.5)
        zn.append(rng.permutation(vn) + 1.5)
    R = len(o)
    dc = rng.integers(-8, 9, (R, N, 27)).astype(np.float32)
    dn = rng.integers(-8, 9, (R, Ni, 27)).astype(np.float32)
    bounds = [[-1, -1, -1], [1, 1, 1]]
    return PlaneCase(P_EXACT_HW, P_EXACT_HW, bounds, np.array(o), np.array(d), np.zeros(R), np.full(R, 3.0), np.array(zc), np.array(zn), 1, dc, dn)


P_RANDOM_HW = ((40, 40), (24, 40), (256, 256))                       # ragged tiles, non-square, production size
P_RANDOM_RAYS = ((1, 1, 1), (33, 64, 64), (70, 65, 3), (600, 130, 70))   # minimum, ragged ray tile, ragged 64-sample blocks, second 512-ray sweep
P_RANDOM_BOUNDS = [[-0.7, -1.1, -0.4], [0.9, 0.8, 1.3]]
P_RANDOM = tuple((hw, rn) for hw in P_RANDOM_HW for rn in P_RANDOM_RAYS)


def p_random_variant(hw, rn):
    """(coarse depths NULL?, new depths as rows?) of a case: the four combinations go round the twelve cases."""
    i = P_RANDOM.index((hw, rn))
    i = i + i // 4                                                   # shift per plane size: every ray shape meets three of the four
    return bool(i & 1), bool(i & 2)


def p_random(hw, rn, jitter=0.0):
    """Random rays through the box from origins 2 and 8 box widths away.  `jitter` > 0 is for the points call only: see p_random_points."""
    (H, W), (R, N, Ni) = hw, rn
    null_zc, zn_rows = p_random_variant(hw, rn)
    rng = np.random.default_rng(6000 + 100 * P_RANDOM_HW.index(hw) + P_RANDOM_RAYS.index(rn))
    b = np.array(P_RANDOM_BOUNDS)
    centre, ext = b.mean(0), b[1] - b[0]
    width = float(ext.max())
    target = centre + (rng.random((R, 3)) - 0.5) * ext * (1.1 if R > 1 else 0.5)   # a few rays graze or miss the box; a lone ray hits it
    dirn = rng.normal(size=(R, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    dist = np.where(np.arange(R) % 2 == 0, 2.0, 8.0) * width
    o = target - dirn * dist[:, None]
    # depths from in front of the box to behind it; a pass of ONE sample stays close to the target so that the case is not empty
    reach = (0.6 if N > 1 else 0.05) * float(np.linalg.norm(ext))
    near, far = dist - reach, dist + reach
    zc = None if null_zc else near[:, None] + (far - near)[:, None] * (np.arange(N)[None] + rng.random((R, N))) / N
    zn = np.sort(near[:, None] + (far - near)[:, None] * rng.random((R, Ni)), axis=1)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)
    dc = sgn((R, N, 27)) * np.exp2(rng.uniform(-20, 0, (R, N, 27)))
    dn = sgn((R, Ni, 27)) * np.exp2(rng.uniform(-20, 0, (R, Ni, 27)))
    return PlaneCase(H, W, b, o, dirn, near, far, zc, zn, 1 if zn_rows else 0, dc, dn)


def p_random_points(hw, rn):
    """Points for hl_render_plane_grads_points that are NOT on straight rays: the ray case's points bent by a smooth displacement of up to
    3 % of the box per axis plus a 0.3 % scatter (a stand-in for the body deformation), float32."""
    case = p_random(hw, rn)
    rng = np.random.default_rng(7000 + 100 * P_RANDOM_HW.index(hw) + P_RANDOM_RAYS.index(rn))
    ext = (case.bounds[1] - case.bounds[0]).astype(np.float64)
    out = []
    for pts in case.points():
        p = pts.astype(np.float64)
        bend = 0.03 * ext * np.sin(7.0 * p[..., [1, 2, 0]] / ext)
        out.append((p + bend + 0.003 * ext * rng.normal(size=p.shape)).astype(np.float32))
    return case, tuple(out)


def p_dense_points(H, W, n=30000):
    """n points uniform in 1.2 x the box with deltas +-2^uniform(-20, 0): hundreds of contributions on every texel, so that no texel's sum
    rests on one tap with a vanishing weight - the situation in which a restatement with float32 coordinates can be held to 1e-5 of a
    texel's sum of |contributions| (a lone tap of weight w differs from its float64 value by about 2^-24 W / w of itself)."""
    rng = np.random.default_rng(8000 + H * 1000 + W)
    b = np.array(P_RANDOM_BOUNDS)
    pts = b.mean(0) + (rng.random((n, 3)) - 0.5) * (b[1] - b[0]) * 1.2
    delta = rng.choice([-1.0, 1.0], (n, 27)) * np.exp2(rng.uniform(-20, 0, (n, 27)))
    return pts.astype(np.float32), delta.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def p_reference(kind, hw=None, rn=None):
    """(case, points of both passes, restatement) of 'exact', 'rays' or 'points' inputs, computed once and shared; treat as read-only."""
    if kind == "exact":
        case = p_exact()
        pts = case.points()
    elif kind == "rays":
        case = p_random(hw, rn)
        pts = case.points()
    else:
        case, pts = p_random_points(hw, rn)
    ref = rr.plane_grads(*case.flat(pts), case.bounds, case.H, case.W)
    return case, pts, ref


def p_random_bar(case, ref):
    """|got - want| <= 2^-24 |want| + taps x 2^-43 x vmax per texel: float32's rounding of the sum and the fixed-point unit of a contribution."""
    vmax = max(float(np.abs(case.delta_c).max()), float(np.abs(case.delta_n).max()))
    return 2.0 ** -24 * np.abs(ref["want"]) + np.repeat(ref["taps"], 3, axis=0).astype(np.float64) * 2.0 ** -43 * vmax
