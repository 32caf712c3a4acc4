"""The mesh rasteriser restated in numpy (DESIGN.md "Rasterising the mesh"; csrc/hl_mesh_raster.hip), for the tests.

Coverage is exact integer arithmetic (int64 on 1/256-pixel coordinates, as the kernel); depth, weights and attributes are computed in
`dtype`: float32 follows the kernel's stated order rounding for rounding (the yardstick), float64 is the truth.  Inputs that the kernel
reads as fp32 (vertices, normals, the records' z) are widened exactly.  Everything is vectorised per triangle over its box; the scenes
of the tests take seconds."""
import numpy as np

F32, F64 = np.float32, np.float64
GUARD = float(1 << 19)          # pixels
SUB = 256                       # sub-pixel steps per pixel


def owned(dx, dy):
    """The one-sided rule of an edge of direction (dx, dy): true for exactly one of d and -d (d != 0)."""
    return (dy < 0) | ((dy == 0) & (dx > 0))


def camera_centre(R, T):
    R, T = np.asarray(R, F64), np.asarray(T, F64).reshape(3)
    return np.array([-((R[0, c] * T[0] + R[1, c] * T[1]) + R[2, c] * T[2]) for c in range(3)])


def project(v, K, R, T, dtype=F64, znear=1e-3):
    """v (N,3) -> X, Y int64 (1/256 pixel), z float32, invalid bool.  dtype float64 is the kernel's arithmetic."""
    v = np.asarray(v, F32).astype(dtype)
    K, R, T = np.asarray(K, dtype), np.asarray(R, dtype), np.asarray(T, dtype).reshape(3)
    with np.errstate(all="ignore"):
        cam = [((R[r, 0] * v[:, 0] + R[r, 1] * v[:, 1]) + R[r, 2] * v[:, 2]) + T[r] for r in range(3)]
        p = [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]
        sx, sy = p[0] / p[2], p[1] / p[2]
        ok = np.isfinite(cam[0]) & np.isfinite(cam[1]) & np.isfinite(cam[2]) & (cam[2] > znear) & (np.abs(sx) <= GUARD) & (np.abs(sy) <= GUARD)
        X = np.where(ok, np.rint(np.where(ok, sx, 0) * SUB), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, sy, 0) * SUB), 0).astype(np.int64)
        z = np.where(ok, cam[2], 0).astype(F32)
    return X, Y, z, ~ok


def _setup(X, Y, tri):
    """tri (...,3) indices -> drawing order (...,3) (vertices 1 and 2 swapped where A < 0), |A|, sign of A."""
    i0, i1, i2 = tri[..., 0], tri[..., 1], tri[..., 2]
    A = (X[i1] - X[i0]) * (Y[i2] - Y[i0]) - (Y[i1] - Y[i0]) * (X[i2] - X[i0])
    sw = A < 0
    order = np.stack([i0, np.where(sw, i2, i1), np.where(sw, i1, i2)], axis=-1)
    return order, np.abs(A), np.sign(A)


def _edges(X, Y, order, PX, PY):
    """Edge functions E_i (weight of drawing-order vertex i: the edge from i+1 to i+2) at points PX, PY, and the coverage."""
    E, cov = [], True
    for i in range(3):
        a, b = order[..., (i + 1) % 3], order[..., (i + 2) % 3]
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        e = dx * (PY - Y[a]) - dy * (PX - X[a])
        cov = cov & ((e > 0) | ((e == 0) & owned(dx, dy)))
        E.append(e)
    return E, cov


def _depth(E, A, zs, dtype):
    """q_i = ((dtype)E_i / (dtype)A) / z_i and depth = 1 / ((q0 + q1) + q2)."""
    fA = np.asarray(A).astype(dtype)
    q = [(np.asarray(E[i]).astype(dtype) / fA) / np.asarray(zs[i], F32).astype(dtype) for i in range(3)]
    return q, dtype(1) / ((q[0] + q[1]) + q[2])


def drawn(X, Y, invalid, triangles, cull=None):
    """Which triangles the cover stage draws at all: indices in range, vertices valid, A != 0, winding not culled."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = X.shape[0]
    inr = ((tri >= 0) & (tri < N)).all(axis=1)
    safe = np.where(inr[:, None], tri, 0)
    _, A, sg = _setup(X, Y, safe)
    ok = inr & ~invalid[safe].any(axis=1) & (A != 0)
    if cull == "back":
        ok &= sg > 0
    elif cull == "front":
        ok &= sg < 0
    return ok


def cover(X, Y, z, triangles, H, W, dtype=F64, invalid=None, cull=None):
    """-> dict: `id` int64 (H,W) (-1 background; the lower index wins an exact depth tie), `depth` nearest, `depth2` second-nearest
    (inf where fewer than two), `hits` per pixel, all (H,W)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    invalid = np.zeros(X.shape[0], bool) if invalid is None else invalid
    ok = drawn(X, Y, invalid, tri, cull)
    ids = np.full((H, W), -1, np.int64)
    d1, d2 = np.full((H, W), np.inf, dtype), np.full((H, W), np.inf, dtype)
    hits = np.zeros((H, W), np.int64)
    for t in np.nonzero(ok)[0]:
        order, A, _ = _setup(X, Y, tri[t])
        xs, ys = X[order], Y[order]
        x0, x1 = max(-((-int(xs.min())) // SUB), 0), min(int(xs.max()) // SUB, W - 1)
        y0, y1 = max(-((-int(ys.min())) // SUB), 0), min(int(ys.max()) // SUB, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        PY, PX = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64) * SUB, np.arange(x0, x1 + 1, dtype=np.int64) * SUB, indexing="ij")
        E, cov = _edges(X, Y, order, PX, PY)
        if not cov.any():
            continue
        _, depth = _depth(E, A, z[order], dtype)
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        o1, o2, oi, oh = d1[sl], d2[sl], ids[sl], hits[sl]
        better = cov & ((depth < o1) | ((depth == o1) & (t < oi)))          # (triangles come in ascending order: the tie never moves)
        worse = cov & ~better
        o2[better] = o1[better]
        o1[better] = depth[better]
        oi[better] = t
        o2[worse] = np.minimum(o2[worse], depth[worse])
        oh[cov] += 1
    return {"id": ids, "depth": np.where(ids >= 0, d1, 0).astype(dtype), "depth2": d2, "hits": hits}


def ray_directions(H, W, K, R, T, dtype=F64):
    """Unit ray direction of every pixel (H,W,3): camera_ray_pixel's float64 direction, rounded to `dtype`, then normalised there."""
    Ki, R, T = np.linalg.inv(np.asarray(K, F64)), np.asarray(R, F64), np.asarray(T, F64).reshape(3)
    o = camera_centre(R, T)
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    q = [((x * Ki[c, 0] + y * Ki[c, 1]) + Ki[c, 2]) - T[c] for c in range(3)]
    d = np.stack([((q[0] * R[0, c] + q[1] * R[1, c]) + q[2] * R[2, c]) - o[c] for c in range(3)], axis=-1).astype(dtype)
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return d / n[..., None]


def _unit(v):
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(all="ignore"):
        return np.where(((n > 0) & np.isfinite(n))[..., None], v / n[..., None], 0).astype(v.dtype)


def resolve(X, Y, z, triangles, ids, depth, vertices, K, R, T, normals=None, colors=None, shade="colors", white_bkgd=False, dtype=F64):
    """The interpolation stage for the winners `ids` (H,W) with their `depth` (H,W) -> rgb, acc, normal, depth, barycentrics (the
    triangle's own vertex order), as the kernel's outputs, in `dtype`."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    H, W = ids.shape
    hit = ids >= 0
    py, px = np.nonzero(hit)
    t = tri[ids[py, px]]
    order, A, sg = _setup(X, Y, t)
    E, _ = _edges(X, Y, order, px.astype(np.int64) * SUB, py.astype(np.int64) * SUB)
    q, _ = _depth(E, A, [z[order[:, i]] for i in range(3)], dtype)
    dep = depth[py, px].astype(dtype)
    w = [q[i] * dep for i in range(3)]
    v = np.asarray(vertices, F32).astype(dtype)
    if normals is not None:
        nb = np.asarray(normals, F32).astype(dtype)
        n = _unit(np.stack([(w[0] * nb[order[:, 0], c] + w[1] * nb[order[:, 1], c]) + w[2] * nb[order[:, 2], c] for c in range(3)], axis=-1))
    else:
        v0, e1, e2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1)
        d = v0 - camera_centre(R, T).astype(F32 if dtype == F32 else F64).astype(dtype)
        away = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > 0
        n = _unit(np.where(away[:, None], -n, n))
    if colors is not None:
        cb = np.asarray(colors, np.uint8).astype(dtype) / dtype(255)
        col = np.stack([(w[0] * cb[order[:, 0], c] + w[1] * cb[order[:, 1], c]) + w[2] * cb[order[:, 2], c] for c in range(3)], axis=-1)
    else:
        col = np.full((py.size, 3), dtype(F32(0.7)), dtype)
    if shade == "headlight":
        r = ray_directions(H, W, K, R, T, dtype)[py, px]
        col = col * np.abs((n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2])[:, None]
    sw = sg < 0
    bary = np.stack([w[0], np.where(sw, w[2], w[1]), np.where(sw, w[1], w[2])], axis=-1)
    out = {"rgb_map": np.full((H, W, 3), 1 if white_bkgd else 0, dtype), "acc_map": hit.astype(dtype), "normal_map": np.zeros((H, W, 3), dtype),
           "depth_map": np.where(hit, depth, 0).astype(dtype), "barycentrics": np.zeros((H, W, 3), dtype)}
    out["rgb_map"][py, px], out["normal_map"][py, px], out["barycentrics"][py, px] = col, n, bary
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def scene_camera(H=48, W=67, focal=70.0):
    """A pinhole camera with an off-centre principal point, rotated 0.3 rad, T = (0.05, -0.02, 2.0)."""
    K = np.array([[focal, 0.0, W / 2.0 + 1.7], [0.0, focal, H / 2.0 - 2.3], [0.0, 0.0, 1.0]])
    a = np.array([0.3, -0.5, 0.8])
    a = a / np.linalg.norm(a) * 0.3
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    return K, R, np.array([0.05, -0.02, 2.0])


def sheet(n, seed, z0=0.0, amplitude=0.05, extent=0.9, jitter=0.3):
    """A wavy sheet of n x n jittered quads, two triangles each: vertices float32 ((n+1)^2,3), triangles int64 (2 n^2,3)."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-extent / 2, extent / 2, n + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    h = extent / n
    x = x + rng.uniform(-jitter, jitter, x.shape) * h
    y = y + rng.uniform(-jitter, jitter, y.shape) * h
    zz = z0 + amplitude * np.sin(7.0 * x + 0.5 * seed) * np.cos(5.0 * y - 0.3 * seed)
    v = np.stack([x, y, zz], axis=-1).reshape(-1, 3).astype(F32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    tri = np.concatenate([np.stack([i, i + 1, i + n + 2], axis=1), np.stack([i, i + n + 2, i + n + 1], axis=1)], axis=0).astype(np.int64)
    return v, tri
