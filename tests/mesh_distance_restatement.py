"""The rules of DESIGN.md "Measuring mesh distance" once more, in numpy float64 and in the stated order of operations.

Everything is relative to an origin o, the componentwise minimum of the target's finite vertices: p = v - o.
    dot(a, b) = (ax bx + ay by) + az bz,   cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx)
    seg(p, a, e): l = dot(e, e), t = dot(p - a, e), t = t / l if l > 0 else 0, t clamped to [0, 1] (a zero keeps a + sign),
                  x = a + t e, r = p - x, d2 = dot(r, r)
    closest(p, a, b, c): seg over (a, b - a), (b, c - b), (c, a - c); then n = cross(b - a, c - a), nn = dot(n, n) and, only where nn > 0 and
                  finite, v = dot(cross(p - a, c - a), n) / nn, w = dot(cross(b - a, p - a), n) / nn and, only where v >= 0, w >= 0 and
                  v + w <= 1, x = a + (v (b - a) + w (c - a)).  The smallest d2 wins, the first of ab, bc, ca, interior in a tie.
                  Barycentrics: ab (1 - t, t, 0), bc (0, 1 - t, t), ca (t, 0, 1 - t), interior ((1 - v) - w, v, w).
    Between triangles the smallest (d2, index) wins.  A triangle with an index outside [0, N) or a non-finite corner takes no part.
The sampler: a_i = rint((sqrt(nn_i) / 2) / u), u = L^2 / 2^30 with L the longest side of the bounds; P its exclusive prefix; sample s of S:
    k = floor(((s + 0.5) / S) A_fix), the largest i with P[i] <= k, m = seed 2^32 + s + 1 (mod 2^64),
    u1 = ((m 0xC13FA9A902A6328F mod 2^64) >> 11) 2^-53, u2 likewise with 0x91E10DA5C79E7B1D; u1 + u2 > 1: both become 1 - u;
    point = a + (u1 (b - a) + u2 (c - a)) + o, barycentrics ((1 - u1) - u2, u1, u2), normal = n / sqrt(nn).
"""
import numpy as np

from mesh_simplify_restatement import ELLIPSOID_CENTRE, ellipsoid, sheet  # noqa: F401  (the meshes the tests use)

STATUS_INDEX, STATUS_CORNER, STATUS_QUERY = 1, 2, 4
WIDE_CELLS = 4096
SLACK = 2.0 ** -20
R2_A, R2_B = 0xC13FA9A902A6328F, 0x91E10DA5C79E7B1D


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def seg(p, a, e):
    """-> (d2, t, x), broadcasting."""
    l = dot(e, e)
    t = dot(p - a, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l > 0.0, t / np.where(l > 0.0, l, 1.0), 0.0)
    t = np.where(t > 0.0, t, 0.0)
    t = np.where(t < 1.0, t, 1.0)
    x = a + t[..., None] * e
    r = p - x
    return dot(r, r), t, x


def closest(p, a, b, c):
    """p, a, b, c broadcastable (..., 3), relative to the origin -> (d2, winner 0..3, x, barycentrics)."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac = b - a, c - a
    d0, t0, x0 = seg(p, a, ab)
    d1, t1, x1 = seg(p, b, c - b)
    d2, t2, x2 = seg(p, c, a - c)
    n = cross(ab, ac)
    nn = dot(n, n)
    ap = p - a
    ok = (nn > 0.0) & np.isfinite(nn)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        snn = np.where(ok, nn, 1.0)
        v = dot(cross(ap, ac), n) / snn
        w = dot(cross(ab, ap), n) / snn
        inside = ok & (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
        x3 = a + (v[..., None] * ab + w[..., None] * ac)
        r3 = p - x3
        d3 = np.where(inside, dot(r3, r3), np.inf)
    best, win = d0.copy(), np.zeros(d0.shape, dtype=np.int64)
    for k, d in ((1, d1), (2, d2), (3, d3)):
        better = d < best
        best, win = np.where(better, d, best), np.where(better, k, win)
    zero = np.zeros_like(t0)
    barys = [np.stack([1.0 - t0, t0, zero], axis=-1), np.stack([zero, 1.0 - t1, t1], axis=-1), np.stack([t2, zero, 1.0 - t2], axis=-1),
             np.stack([(1.0 - v) - w, v, w], axis=-1)]
    x, bary = x0, barys[0]
    for k, (xk, bk) in enumerate(((x1, barys[1]), (x2, barys[2]), (x3, barys[3])), 1):
        x, bary = np.where((win == k)[..., None], xk, x), np.where((win == k)[..., None], bk, bary)
    return best, win, x, bary


def target(vertices, triangles):
    """-> dict: origin, hi (the bounds relative to nothing), corners (T,3,3) relative to the origin (zeros where invalid), valid (T,), status."""
    v = np.asarray(vertices, dtype=np.float64)
    tri = np.asarray(triangles).astype(np.int64)
    fin = np.isfinite(v).all(axis=1)
    origin, hi = v[fin].min(axis=0), v[fin].max(axis=0)
    inrange = ((tri >= 0) & (tri < len(v))).all(axis=1)
    safe = np.where(inrange[:, None], tri, 0)
    corner_ok = fin[safe].all(axis=1)
    valid = inrange & corner_ok
    status = (0 if inrange.all() else STATUS_INDEX) | (0 if (corner_ok | ~inrange).all() else STATUS_CORNER)
    with np.errstate(invalid="ignore"):
        corners = np.where(valid[:, None, None], v[safe] - origin[None, None], 0.0)
    return {"origin": origin, "hi": hi, "corners": corners, "valid": valid, "status": status, "N": len(v), "T": len(tri)}


def sqdist_matrix(points, tg, chunk=256):
    """d2 of every query to every triangle (Q,T); +inf for a dropped triangle."""
    p = np.asarray(points, dtype=np.float64) - tg["origin"][None]
    cn = tg["corners"]
    out = np.empty((len(p), len(cn)))
    for s in range(0, len(p), chunk):
        d2 = closest(p[s:s + chunk, None], cn[None, :, 0], cn[None, :, 1], cn[None, :, 2])[0]
        out[s:s + chunk] = np.where(tg["valid"][None], d2, np.inf)
    return out


def hit(points, tg, tri):
    """The full answer of every query against the triangle `tri` names for it -> (d2, x + o, barycentrics)."""
    p = np.asarray(points, dtype=np.float64) - tg["origin"][None]
    cn = tg["corners"][tri]
    d2, _, x, bary = closest(p, cn[:, 0], cn[:, 1], cn[:, 2])
    return d2, x + tg["origin"][None], bary


def brute(points, vertices, triangles, normals=None):
    """Every triangle for every query -> dict: sqdist, triangle, barycentric, point, normal_dot, matrix (Q,T), target."""
    tg = target(vertices, triangles)
    m = sqdist_matrix(points, tg)
    tri = np.argmin(m, axis=1)                      # (the first minimum: the smallest index)
    d2, x, bary = hit(points, tg, tri)
    assert np.array_equal(d2, m[np.arange(len(tri)), tri])
    out = {"sqdist": d2, "triangle": tri, "barycentric": bary, "point": x, "matrix": m, "target": tg, "normal_dot": None}
    if normals is not None:
        out["normal_dot"] = normal_dot(normals, tg, tri)
    return out


def normal_dot(normals, tg, tri):
    nq = np.asarray(normals, dtype=np.float64)
    cn = tg["corners"][tri]
    n = cross(cn[:, 1] - cn[:, 0], cn[:, 2] - cn[:, 0])
    length = np.sqrt(dot(n, n))
    ok = (length > 0.0) & np.isfinite(length) & np.isfinite(nq).all(axis=1) & (nq != 0.0).any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = n / np.where(ok, length, 1.0)[:, None]
        return np.where(ok, dot(nq, u), np.nan)


# ---- the grid walk --------------------------------------------------------------------------------------------------------------
def build_grid(tg, h):
    """-> dict: g (3,), cells {key: [triangle ids]}, wide [ids in order]."""
    g = np.floor((tg["hi"] - tg["origin"]) / h).astype(np.int64) + 1
    cells, wide = {}, []
    for t in np.nonzero(tg["valid"])[0]:
        cn = tg["corners"][t]
        lo = np.minimum(np.maximum(np.floor(cn.min(axis=0) / h), 0.0), g - 1.0).astype(np.int64)
        hi = np.minimum(np.maximum(np.floor(cn.max(axis=0) / h), 0.0), g - 1.0).astype(np.int64)
        if int(np.prod(hi - lo + 1)) > WIDE_CELLS:
            wide.append(int(t))
            continue
        for cz in range(lo[2], hi[2] + 1):
            for cy in range(lo[1], hi[1] + 1):
                for cx in range(lo[0], hi[0] + 1):
                    cells.setdefault((cz * g[1] + cy) * g[0] + cx, []).append(int(t))
    return {"g": g, "cells": cells, "wide": wide, "h": float(h)}


def grid_walk(points, tg, grid, max_distance=np.inf):
    """The ring search of section 2 -> (sqdist (Q,), triangle (Q,), the largest ring any query reached)."""
    g, h, cells = grid["g"], grid["h"], grid["cells"]
    cn = tg["corners"]
    pts = np.asarray(points, dtype=np.float64) - tg["origin"][None]
    out_d, out_t, rings = np.empty(len(pts)), np.empty(len(pts), dtype=np.int64), 0
    for qi, p in enumerate(pts):
        c = np.minimum(np.maximum(np.floor(p / h), 0.0), g - 1.0).astype(np.int64)
        best = [np.inf, np.iinfo(np.int64).max]

        def test(ids):
            if not ids:
                return
            ids = np.asarray(ids)
            d2 = closest(p[None], cn[ids, 0], cn[ids, 1], cn[ids, 2])[0]
            for d, t in zip(d2, ids):
                if d < best[0] or (d == best[0] and t < best[1]):
                    best[0], best[1] = float(d), int(t)

        test(grid["wide"])
        r = 0
        while True:
            for cz in range(max(c[2] - r, 0), min(c[2] + r, g[2] - 1) + 1):
                for cy in range(max(c[1] - r, 0), min(c[1] + r, g[1] - 1) + 1):
                    face = abs(cz - c[2]) == r or abs(cy - c[1]) == r
                    xs = range(max(c[0] - r, 0), min(c[0] + r, g[0] - 1) + 1) if face else [x for x in {c[0] - r, c[0] + r} if 0 <= x < g[0]]
                    for cx in xs:
                        test(cells.get((cz * g[1] + cy) * g[0] + cx))
            s = np.inf
            for a in range(3):
                if c[a] - r > 0:
                    s = min(s, p[a] - float(c[a] - r) * h)
                if c[a] + r < g[a] - 1:
                    s = min(s, float(c[a] + r + 1) * h - p[a])
            if s == np.inf:
                break
            sm = max(s - h * SLACK, 0.0)
            if best[0] <= sm * sm or sm >= max_distance:
                break
            r += 1
        rings = max(rings, r)
        if best[1] == np.iinfo(np.int64).max or np.sqrt(best[0]) > max_distance:
            out_d[qi], out_t[qi] = np.inf, -1
        else:
            out_d[qi], out_t[qi] = best
    return out_d, out_t, rings


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def areas(tg):
    """-> (a int64 (T,), the exclusive prefix P int64 (T,), A_fix, the unit u)."""
    L = float((tg["hi"] - tg["origin"]).max())
    u = (L * L) / 1073741824.0
    cn = tg["corners"]
    n = cross(cn[:, 1] - cn[:, 0], cn[:, 2] - cn[:, 0])
    q = (np.sqrt(dot(n, n)) / 2.0) / u
    a = np.where(tg["valid"] & (q >= 0.0) & (q < 2147483648.0), np.rint(np.where(np.isfinite(q), q, 0.0)), 0.0).astype(np.int64)
    P = np.concatenate([[0], np.cumsum(a)[:-1]]).astype(np.int64)
    return a, P, int(a.sum()), u


def sample(tg, S, seed=0):
    """-> dict: points, triangle, barycentric, normals, area (a_i), total."""
    a, P, total, _ = areas(tg)
    s = np.arange(S, dtype=np.int64)
    k = np.floor(((s.astype(np.float64) + 0.5) / float(S)) * float(total)).astype(np.uint64).astype(np.int64)
    k = np.minimum(k, total - 1)
    tri = np.searchsorted(P, k, side="right") - 1
    m = (np.uint64(seed) << np.uint64(32)) + s.astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        u1 = ((m * np.uint64(R2_A)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        u2 = ((m * np.uint64(R2_B)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    flip = u1 + u2 > 1.0
    u1, u2 = np.where(flip, 1.0 - u1, u1), np.where(flip, 1.0 - u2, u2)
    cn = tg["corners"][tri]
    ab, ac = cn[:, 1] - cn[:, 0], cn[:, 2] - cn[:, 0]
    x = cn[:, 0] + (u1[:, None] * ab + u2[:, None] * ac)
    n = cross(ab, ac)
    return {"points": x + tg["origin"][None], "triangle": tri, "barycentric": np.stack([(1.0 - u1) - u2, u1, u2], axis=1),
            "normals": n / np.sqrt(dot(n, n))[:, None], "area": a, "total": total}


# ---- the scores -----------------------------------------------------------------------------------------------------------------
def side(distance, sqdist, normal_dot_, thresholds):
    """One side's numbers from per-query arrays, non-finite distances left out -> dict as mesh_distance's a_to_b."""
    ok = np.isfinite(distance)
    d, d2 = distance[ok], sqdist[ok]
    n = int(ok.sum())
    out = {"count": n, "mean": float(d.sum() / n), "mean_sq": float(d2.sum() / n), "rms": float(np.sqrt(d2.sum() / n)), "max": float(d.max()),
           "within": [float((d <= t).sum()) / n for t in thresholds], "normal_consistency": None}
    if normal_dot_ is not None:
        nd = normal_dot_[ok]
        nd = nd[np.isfinite(nd)]
        out["normal_consistency"] = float(nd.sum() / len(nd)) if len(nd) else None
    return out
