"""CPU restatement (numpy) of the mesh extraction in humanliff_amd/NeRF/geometry.py, for the tests only.

It states the contract of DESIGN.md (mesh extraction) a second time, in plain array code:
  * edt: exact separable Euclidean distance transform (brute-force lower envelope per axis), checked against scipy;
  * smooth_constrained: signed distance, band, bounds, the 13-point operator as A x = Q^T Q x, damped projected Jacobi;
  * case_table: marching-cubes cases from a GEOMETRIC face walk (segment direction from a cross product with the outward
    normal), independent of the combinatorial walk of scripts/gen_mc_table.py that produced the baked table;
  * marching_cubes: vertices per crossing lattice edge ordered by key, triangles by cube then table order.
Product code never imports this module.
"""
import numpy as np

INF = 1 << 40


def edt(b):
    """scipy.ndimage.distance_transform_edt(b): distance of every True voxel to the nearest False voxel (0 on False voxels)."""
    f = np.where(b, INF, 0).astype(np.int64)
    for axis in range(f.ndim):
        f = np.moveaxis(f, axis, -1)
        n = f.shape[-1]
        q = np.arange(n, dtype=np.int64)
        out = np.full(f.shape, INF, dtype=np.int64)
        for p in range(n):
            np.minimum(out, f[..., p:p + 1] + (q - p) ** 2, out=out)
        f = np.moveaxis(out, -1, axis)
    return np.sqrt(f.astype(np.float64))


def signed_distance(v, edt_fn=edt):
    b = np.asarray(v) > 0
    if b.all() or not b.any():
        raise ValueError("the volume has no sign change")
    return np.where(b, edt_fn(b) - 0.5, -edt_fn(~b) + 0.5)


def smooth_constrained(v, band_radius=4, max_iters=250, rel_tol=1e-6, edt_fn=edt):
    """Returns (smoothed fp64 volume, sweeps run, band size)."""
    d = signed_distance(v, edt_fn)
    band = np.abs(d) <= band_radius
    nb = int(band.sum())
    var = np.full(d.shape, -1, dtype=np.int64)
    var[band] = np.arange(nb)
    coords = np.argwhere(band)
    nbr = []                                    # nbr[a][s]: variable index of the neighbour (-1: none), s = 0 for -1, 1 for +1
    for a in range(3):
        row = []
        for s in (-1, 1):
            c = coords.copy()
            c[:, a] += s
            ok = (c[:, a] >= 0) & (c[:, a] < d.shape[a])
            idx = np.full(nb, -1, dtype=np.int64)
            idx[ok] = var[c[ok, 0], c[ok, 1], c[ok, 2]]
            row.append(idx)
        nbr.append(row)
    m = [(nbr[a][0] >= 0).astype(np.float64) + (nbr[a][1] >= 0) for a in range(3)]
    diag = sum(m[a] * m[a] + m[a] for a in range(3))

    def grad(x):
        return [sum(np.where(n >= 0, x[n] - x, 0.0) for n in nbr[a]) for a in range(3)]

    def apply_a(x):
        g = grad(x)
        return sum(-m[a] * g[a] + sum(np.where(n >= 0, g[a][n], 0.0) for n in nbr[a]) for a in range(3))

    def energy(x):
        return 0.5 * float(x @ apply_a(x))

    x = d[band].copy()
    lower = np.where(x > 0, x, -np.inf)
    upper = np.where(x < 0, x, np.inf)
    lower[np.isfinite(lower) & (np.abs(lower) < 1)] = 0.0
    upper[np.isfinite(upper) & (np.abs(upper) < 1)] = 0.0
    w = 0.5
    e_prev = energy(x)
    it = 0
    while it < max_iters:
        y = -(apply_a(x) - diag * x) / diag
        x = w * y + (1 - w) * x
        x = np.minimum(np.maximum(x, lower), upper)
        it += 1
        if it % 10 == 0:
            e = energy(x)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = (e_prev - e) / e_prev if e_prev != 0 else float("nan")
            if ratio < 1 - (1 - rel_tol) ** 10:
                break
            e_prev = e
    out = d.copy()
    out[band] = x
    return out, it, nb


# ---- marching cubes ---------------------------------------------------------------------------------------------------
CORNERS = np.array([(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)])
EDGE_AXIS = np.array([e // 4 for e in range(12)])
EDGE_OFF = np.zeros((12, 3), dtype=np.int64)     # lower corner of edge e relative to the cube's lower corner
for _e in range(12):
    _others = [k for k in range(3) if k != _e // 4]
    EDGE_OFF[_e, _others[0]] = _e & 1
    EDGE_OFF[_e, _others[1]] = (_e >> 1) & 1


def _edge_corners(e):
    lo = EDGE_OFF[e]
    hi = lo.copy()
    hi[EDGE_AXIS[e]] += 1
    idx = lambda p: int(p[0] + 2 * p[1] + 4 * p[2])
    return idx(lo), idx(hi)


def _case(cfg):
    above = [(cfg >> c) & 1 for c in range(8)]
    mid = {e: EDGE_OFF[e] + 0.5 * np.eye(3)[EDGE_AXIS[e]] for e in range(12)}
    nxt = {}
    for axis in range(3):
        for side in (0, 1):
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            es = [e for e in range(12) if EDGE_AXIS[e] != axis and EDGE_OFF[e][axis] == side]
            cross = [e for e in es if above[_edge_corners(e)[0]] != above[_edge_corners(e)[1]]]
            if not cross:
                continue
            up = [c for c in cs if above[c]]
            if len(cross) == 2:
                pairs = [(cross[0], cross[1], up[0])]
            else:                                      # ambiguous face: cut off each above corner on its own
                pairs = [tuple([e for e in cross if c in _edge_corners(e)]) + (c,) for c in up]
            for e1, e2, c in pairs:
                dvec = mid[e2] - mid[e1]
                r = CORNERS[c] - 0.5 * (mid[e1] + mid[e2])
                if np.dot(np.cross(dvec, r), n) < 0:
                    e1, e2 = e2, e1
                nxt[e1] = e2
    tris, done = [], set()
    for e0 in sorted(nxt):
        if e0 in done:
            continue
        poly = [e0]
        while nxt[poly[-1]] != e0:
            poly.append(nxt[poly[-1]])
        done.update(poly)
        tris += [(poly[0], poly[i], poly[i + 1]) for i in range(1, len(poly) - 1)]
    return tris


def case_table():
    return [_case(c) for c in range(256)]


_TABLE = None


def marching_cubes(v, iso):
    """Returns (vertices float64 (V,3) in index coordinates, triangles int64 (T,3))."""
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    v = np.asarray(v, dtype=np.float64)
    nx, ny, nz = v.shape
    above = v > iso
    keys, pos = [], []
    for a in range(3):
        sl_lo = [slice(None)] * 3
        sl_hi = [slice(None)] * 3
        sl_lo[a] = slice(0, v.shape[a] - 1)
        sl_hi[a] = slice(1, None)
        crossing = above[tuple(sl_lo)] != above[tuple(sl_hi)]
        p = np.argwhere(crossing)
        fa = v[tuple(sl_lo)][crossing]
        fb = v[tuple(sl_hi)][crossing]
        t = (iso - fa) / (fb - fa)
        q = p.astype(np.float64)
        q[:, a] = q[:, a] + t * 1.0
        keys.append(((p[:, 0] * ny + p[:, 1]) * nz + p[:, 2]) * 3 + a)
        pos.append(q)
    keys = np.concatenate(keys)
    pos = np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    keys, verts = keys[order], pos[order]
    if nx < 2 or ny < 2 or nz < 2:
        return verts.reshape(-1, 3), np.zeros((0, 3), dtype=np.int64)
    cfg = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = CORNERS[c]
        cfg |= above[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntri = np.array([len(t) for t in _TABLE])
    mt = max(ntri)
    tab = np.full((256, mt, 3), -1, dtype=np.int64)
    for c in range(256):
        if _TABLE[c]:
            tab[c, :len(_TABLE[c])] = _TABLE[c]
    cube = np.argwhere(ntri[cfg] > 0)              # C order = cube linear order
    cc = cfg[cube[:, 0], cube[:, 1], cube[:, 2]]
    rep = ntri[cc]
    cube = np.repeat(cube, rep, axis=0)
    slot = np.concatenate([np.arange(r) for r in rep]) if len(rep) else np.zeros(0, dtype=np.int64)
    edges = tab[np.repeat(cc, rep), slot]          # (T, 3)
    lower = cube[:, None, :] + EDGE_OFF[edges]
    k = ((lower[..., 0] * ny + lower[..., 1]) * nz + lower[..., 2]) * 3 + EDGE_AXIS[edges]
    tris = np.searchsorted(keys, k)
    assert np.array_equal(keys[tris], k)
    return verts, tris.astype(np.int64).reshape(-1, 3)
