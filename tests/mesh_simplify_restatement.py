"""The rule of DESIGN.md "Simplifying the mesh" once more, in numpy float64 and in the stated order, plus the meshes the tests use.

Cell units: q = (v - origin) / cell per axis, ci = floor(q), centre = ci + 0.5, key = (cz gy + cy) gx + cx, cluster id = rank of the key
among the occupied keys.  Fixed point: fix(x) = rint(2^30 x) (ties to even, as llrint), 0 for a non-finite x; all sums are int64.

Per cluster, ACC_FIELDS: count; sum fix(q - centre); sum fix(n); sum of the colours; and for every triangle with all indices in range
and all corners in cells, once per distinct cluster k among its corners, at the first corner that lies in k:
    p_j = q_j - centre_k (j = 0, 1, 2),  e1 = p_1 - p_0,  e2 = p_2 - p_0,
    n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x),  l = sqrt((nx nx + ny ny) + nz nz)   (l == 0 or non-finite: nothing)
    u = n / l,  d = -((ux px + uy py) + uz pz) with p the corner in k,  w = min(l / 2, 1)
    xx xy xz yy yz zz += fix((w u_i) u_j),  xd yd zd += fix((w u_i) d),  dd += fix((w d) d)

Representative: m = (sum / 2^30) / count; A, b = sums / 2^30; t = (Axx + Ayy) + Azz; t == 0: p = m; otherwise eps = (1e-3 t) / 3,
    M = A + eps I,  r_i = ((A_i0 m0 + A_i1 m1) + A_i2 m2) + b_i,
    c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
    c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01,
    det = (M00 c00 + M01 c01) + M02 c02     (not positive and finite: p = m)
    p0 = m0 - ((c00 r0 + c01 r1) + c02 r2) / det,  p1 = m1 - ((c01 r0 + c11 r1) + c12 r2) / det,  p2 = m2 - ((c02 r0 + c12 r1) + c22 r2) / det
    p clamped to [-0.5, 0.5];  vertex = origin + ((centre + p) cell);  normal = s / sqrt((sx sx + sy sy) + sz sz), zero stays zero;
    colour = (2 sum + count) // (2 count).
Triangles: cluster ids; two equal: dropped; rotated so that the smallest id leads; key c0 << 42 | c1 << 21 | c2; the smallest input index
of every key survives; survivors in input order; clusters no survivor references are dropped and the rest renumbered in order.
"""
import numpy as np

ACC_FIELDS = ("count", "px", "py", "pz", "nx", "ny", "nz", "r", "g", "b", "xx", "xy", "xz", "yy", "yz", "zz", "xd", "yd", "zd", "dd")
FIX = 1073741824.0
LAMBDA = 1e-3
STATUS_VERTEX, STATUS_INDEX = 1, 2


def fix(x):
    x = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(x)
    return np.where(ok, np.rint(FIX * np.where(ok, x, 0.0)), 0.0).astype(np.int64)


def _three(x):
    v = np.asarray(x, dtype=np.float64)
    return np.full(3, float(v)) if v.shape == () else v.reshape(3).copy()


def clusters(vertices, cell, origin=None):
    """-> dict: q (N,3), ci int64 (N,3), valid (N,), ids int64 (N,) (-1: no cell), ckey int64 (C,), g int64 (3,), origin, cell."""
    v = np.asarray(vertices, dtype=np.float64)
    cell = _three(cell)
    valid = np.isfinite(v).all(axis=1)
    if origin is not None:
        origin = _three(origin)
        with np.errstate(invalid="ignore"):
            valid &= (v >= origin[None]).all(axis=1)
    if not valid.any():
        return None
    lo, hi = v[valid].min(axis=0), v[valid].max(axis=0)
    if origin is None:
        origin = lo.copy()
    g = np.floor((hi - origin) / cell).astype(np.int64) + 1
    with np.errstate(invalid="ignore"):
        q = (v - origin[None]) / cell[None]
        valid &= (q >= 0.0).all(axis=1)
    ci = np.where(valid[:, None], np.floor(np.where(valid[:, None], q, 0.0)), 0.0).astype(np.int64)
    key = (ci[:, 2] * g[1] + ci[:, 1]) * g[0] + ci[:, 0]
    ckey = np.unique(key[valid])
    ids = np.where(valid, np.searchsorted(ckey, key), -1).astype(np.int64)
    return {"q": q, "ci": ci, "valid": valid, "ids": ids, "ckey": ckey, "g": g, "origin": origin, "cell": cell}


def accumulate(cl, triangles, normals=None, colors=None):
    """-> (acc int64 (C,20), status): the integer accumulators of every cluster."""
    q, ci, ids = cl["q"], cl["ci"], cl["ids"]
    N, C = len(ids), len(cl["ckey"])
    acc = np.zeros((C, len(ACC_FIELDS)), dtype=np.int64)
    status = 0 if cl["valid"].all() else STATUS_VERTEX
    mem = np.nonzero(ids >= 0)[0]
    np.add.at(acc[:, 0], ids[mem], 1)
    rel = q[mem] - (ci[mem].astype(np.float64) + 0.5)
    for c in range(3):
        np.add.at(acc[:, 1 + c], ids[mem], fix(rel[:, c]))
        if normals is not None:
            np.add.at(acc[:, 4 + c], ids[mem], fix(np.asarray(normals, dtype=np.float64)[mem, c]))
        if colors is not None:
            np.add.at(acc[:, 7 + c], ids[mem], np.asarray(colors)[mem, c].astype(np.int64))
    tri = np.asarray(triangles).astype(np.int64)
    inrange = ((tri >= 0) & (tri < N)).all(axis=1)
    if not inrange.all():
        status |= STATUS_INDEX
    tri = tri[inrange]
    tid = ids[tri]
    tri, tid = tri[(tid >= 0).all(axis=1)], tid[(tid >= 0).all(axis=1)]
    for k in range(3):
        first = np.ones(len(tri), dtype=bool)
        for j in range(k):
            first &= tid[:, k] != tid[:, j]
        tk, dst = tri[first], tid[first, k]
        centre = ci[tk[:, k]].astype(np.float64) + 0.5
        p = [q[tk[:, j]] - centre for j in range(3)]
        e1, e2 = p[1] - p[0], p[2] - p[0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (l > 0.0) & np.isfinite(l)
        n, l, pk, dst = n[ok], l[ok], p[k][ok], dst[ok]
        u = n / l[:, None]
        d = -((u[:, 0] * pk[:, 0] + u[:, 1] * pk[:, 1]) + u[:, 2] * pk[:, 2])
        w = np.minimum(l / 2.0, 1.0)
        wu, wd = w[:, None] * u, w * d
        terms = [wu[:, 0] * u[:, 0], wu[:, 0] * u[:, 1], wu[:, 0] * u[:, 2], wu[:, 1] * u[:, 1], wu[:, 1] * u[:, 2], wu[:, 2] * u[:, 2],
                 wu[:, 0] * d, wu[:, 1] * d, wu[:, 2] * d, wd * d]
        for f, term in enumerate(terms):
            np.add.at(acc[:, 10 + f], dst, fix(term))
    return acc, status


def contributions(cl, triangles):
    """How many fixed-point terms went into each accumulator: int64 (C,20) - the bound on a difference of one unit per llrint tie."""
    ids = cl["ids"]
    C = len(cl["ckey"])
    out = np.zeros((C, len(ACC_FIELDS)), dtype=np.int64)
    members = np.bincount(ids[ids >= 0], minlength=C)
    out[:, 1:7] = members[:, None]
    tri = np.asarray(triangles).astype(np.int64)
    tri = tri[((tri >= 0) & (tri < len(ids))).all(axis=1)]
    tid = ids[tri]
    tid = tid[(tid >= 0).all(axis=1)]
    touch = np.zeros(C, dtype=np.int64)
    for k in range(3):
        first = np.ones(len(tid), dtype=bool)
        for j in range(k):
            first &= tid[:, k] != tid[:, j]
        np.add.at(touch, tid[first, k], 1)
    out[:, 10:] = touch[:, None]
    return out


def representatives(acc, ckey, g, origin, cell, with_normals=True, with_colors=True):
    """The representative of every cluster from integer sums -> (p (C,3) in cell units about the centre, vertices (C,3) world,
    normals (C,3) or None, colors uint8 (C,3) or None, the largest condition number among the systems solved)."""
    acc = np.asarray(acc, dtype=np.int64)
    count = acc[:, 0]
    cnt = count.astype(np.float64)
    m = (acc[:, 1:4].astype(np.float64) / FIX) / cnt[:, None]
    Axx, Axy, Axz, Ayy, Ayz, Azz = (acc[:, 10 + f].astype(np.float64) / FIX for f in range(6))
    b = acc[:, 16:19].astype(np.float64) / FIX
    t = (Axx + Ayy) + Azz
    eps = (LAMBDA * t) / 3.0
    M00, M11, M22, M01, M02, M12 = Axx + eps, Ayy + eps, Azz + eps, Axy, Axz, Ayz
    r0 = ((Axx * m[:, 0] + Axy * m[:, 1]) + Axz * m[:, 2]) + b[:, 0]
    r1 = ((Axy * m[:, 0] + Ayy * m[:, 1]) + Ayz * m[:, 2]) + b[:, 1]
    r2 = ((Axz * m[:, 0] + Ayz * m[:, 1]) + Azz * m[:, 2]) + b[:, 2]
    c00, c01, c02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
    c11, c12, c22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
    det = (M00 * c00 + M01 * c01) + M02 * c02
    solve = (t != 0.0) & (det > 0.0) & np.isfinite(det)
    sd = np.where(solve, det, 1.0)
    x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / sd, ((c01 * r0 + c11 * r1) + c12 * r2) / sd, ((c02 * r0 + c12 * r1) + c22 * r2) / sd], axis=1)
    p = np.where(solve[:, None], m - x, m)
    p = np.minimum(np.maximum(p, -0.5), 0.5)
    key = np.asarray(ckey, dtype=np.int64)
    ci = np.stack([key % g[0], (key // g[0]) % g[1], key // (g[0] * g[1])], axis=1)
    vertices = origin[None] + ((ci.astype(np.float64) + 0.5) + p) * cell[None]
    normals = colors = None
    if with_normals:
        s = acc[:, 4:7].astype(np.float64) / FIX
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0.0) & np.isfinite(length)
        normals = np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0)
    if with_colors:
        colors = ((2 * acc[:, 7:10] + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    some = t != 0.0
    cond = 1.0
    if some.any():                                  # the condition number of the systems solved: at most (t + eps) / eps = 3 / lambda + 1
        M = np.stack([np.stack([M00, M01, M02], axis=1), np.stack([M01, M11, M12], axis=1), np.stack([M02, M12, M22], axis=1)], axis=1)[some]
        ev = np.linalg.eigvalsh(M)
        cond = float((ev[:, 2] / ev[:, 0]).max())
    return p, vertices, normals, colors, cond


def oriented_keys(cl, triangles):
    """-> (input indices of the triangles with three different clusters, their rotated ids int64 (K,3), their packed keys)."""
    ids = cl["ids"]
    tri = np.asarray(triangles).astype(np.int64)
    inrange = ((tri >= 0) & (tri < len(ids))).all(axis=1)
    tid = np.where(inrange[:, None], ids[np.where(inrange[:, None], tri, 0)], -1)
    keep = (tid >= 0).all(axis=1) & (tid[:, 0] != tid[:, 1]) & (tid[:, 1] != tid[:, 2]) & (tid[:, 0] != tid[:, 2])
    index = np.nonzero(keep)[0]
    tid = tid[keep]
    lead = np.argmin(tid, axis=1)
    rot = np.stack([tid[np.arange(len(tid)), (lead + j) % 3] for j in range(3)], axis=1)
    return index, rot, (rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2]


def simplify(vertices, triangles, cell, origin=None, normals=None, colors=None):
    """The whole rule -> dict: vertices, triangles, normals, colors, vertex_map as simplify_mesh returns them, plus ids (N,), ckey, acc,
    status, g, origin, cell, p (cell units, every cluster), used (C,) bool, survivors (input indices), cond."""
    N = len(vertices)
    cl = clusters(vertices, cell, origin)
    if cl is None:
        return None
    acc, status = accumulate(cl, triangles, normals, colors)
    index, rot, keys = oriented_keys(cl, triangles)
    _, first = np.unique(keys, return_index=True)            # (the first occurrence: the smallest input index)
    first = np.sort(first)
    survivors, rot = index[first], rot[first]
    C = len(cl["ckey"])
    used = np.zeros(C, dtype=bool)
    used[rot.reshape(-1)] = True
    newidx = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    p, verts, nrm, col, cond = representatives(acc, cl["ckey"], cl["g"], cl["origin"], cl["cell"], normals is not None, colors is not None)
    ids = cl["ids"]
    return {"vertices": verts[used], "triangles": newidx[rot].reshape(-1, 3), "normals": None if nrm is None else nrm[used],
            "colors": None if col is None else col[used], "vertex_map": np.where(ids >= 0, newidx[np.maximum(ids, 0)], -1).astype(np.int64),
            "ids": ids, "ckey": cl["ckey"], "acc": acc, "status": status, "g": cl["g"], "origin": cl["origin"], "cell": cl["cell"], "p": p,
            "used": used, "survivors": survivors, "cond": cond, "N": N}


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
ELLIPSOID_SEMI = (0.25, 0.9, 0.18)
ELLIPSOID_CENTRE = (0.1, -0.05, 2.0)


def ellipsoid(n_lat, n_lon, semi=ELLIPSOID_SEMI, centre=ELLIPSOID_CENTRE):
    """A lat-long ellipsoid with pole fans, outward triangles: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) triangles; the poles
    on the second axis.  -> (vertices, triangles, unit normals of the ellipsoid at the vertices)."""
    semi, centre = np.asarray(semi, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2.0 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.broadcast_to(np.cos(th)[:, None], (n_lat - 1, n_lon)), np.sin(th)[:, None] * np.sin(ph)[None]],
                    axis=2).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]])
    v = centre[None] + unit * semi[None]
    nrm = unit / semi[None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    south = len(v) - 1
    at = lambda i, j: 1 + i * n_lon + j % n_lon  # noqa: E731
    tris = []
    for j in range(n_lon):
        tris.append((0, at(0, j + 1), at(0, j)))
        for i in range(n_lat - 2):
            tris.append((at(i, j), at(i, j + 1), at(i + 1, j)))
            tris.append((at(i, j + 1), at(i + 1, j + 1), at(i + 1, j)))
        tris.append((south, at(n_lat - 2, j), at(n_lat - 2, j + 1)))
    tris = np.asarray(tris, dtype=np.int64)
    # outward: the flat normal of every triangle points away from the centre
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3.0 - centre[None]) > 0).all()
    return v, tris, nrm


def ellipsoid_level(vertices, semi=ELLIPSOID_SEMI, centre=ELLIPSOID_CENTRE):
    """The ellipsoid's implicit function sqrt(sum ((v - c) / s)^2): 1 on the surface."""
    return np.sqrt((((np.asarray(vertices) - np.asarray(centre)[None]) / np.asarray(semi)[None]) ** 2).sum(axis=1))


def sheet(n=24, spacing=0.01, jitter=0.3, seed=0, offset=(0.0, 0.0, 0.0)):
    """An n x n sheet of quads (two triangles each, normals towards +z) over the xy plane, bent (z = a smooth bump) and jittered by
    `jitter` spacings in every coordinate: (n + 1)^2 vertices, 2 n^2 triangles.  -> (vertices, triangles, normals, colors)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i.reshape(-1).astype(np.float64), j.reshape(-1).astype(np.float64)
    z = 3.0 * np.sin(x / n * 2.0) * np.cos(y / n * 3.0)
    v = (np.stack([x, y, z], axis=1) + jitter * (rng.random((len(x), 3)) * 2.0 - 1.0)) * spacing + np.asarray(offset, dtype=np.float64)[None]
    at = lambda a, b: a * (n + 1) + b  # noqa: E731
    tris = []
    for a in range(n):
        for b in range(n):
            tris.append((at(a, b), at(a + 1, b), at(a + 1, b + 1)))
            tris.append((at(a, b), at(a + 1, b + 1), at(a, b + 1)))
    nrm = rng.normal(size=v.shape) * 0.3 + np.asarray([0.0, 0.0, 1.0])[None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = rng.integers(0, 256, size=v.shape, dtype=np.uint8)
    return v, np.asarray(tris, dtype=np.int64), nrm, col
