"""Numpy restatement of binding a mesh to a posed body and reposing it (csrc/hl_mesh_animate.hip; DESIGN.md "Animating the mesh"),
written from the formulas.  Every function takes `dtype`:

  np.float64 - the truth;
  np.float32 - the same formulas in the kernel's stated order, every operation rounded to float32 (numpy's elementwise float32
               arithmetic: a product and the sum it goes into are two roundings, as the kernels are compiled).  This is the yardstick of
               the GPU tests: the kernel may be off from the truth by at most FACTOR x what this is off by on the same inputs.

A body vertex j of a frame has the forward row R_j (3x3), t_j, po_j - a rest point x goes to R_j (x + po_j) + t_j - and the SMPL-space
position s_j.  For a mesh vertex x (world) with normal n, R_w / Th the frame's world transform:

    q = (x - Th) R_w
    the K vertices of smallest d_j = |q - s_j|^2, by a stable argsort: (d, index) ascending
    w_k = 1 / (d_k + 1e-8), divided by their sum              M = sum_k w_k R_k          c = sum_k w_k (R_k po_k + t_k)
    u = M^-1 ((q - transl_b) - c)   (by cofactors)              m = normalize(M^T (n R_w)), zero for a zero or non-finite vector
    repose:  y = M_f u + c_f (+ transl_f)     world = R_w y + Th      normal = R_w normalize(cof(M_f) m)
"""
import numpy as np


def rows_from_pose(t):
    """The (V,16) forward rows R[9] t[3] pose_off[3] pad[1] of one frame from what body_restatement.pose returns: its T is [R | t]."""
    V = t["T"].shape[0]
    rows = np.zeros((V, 16))
    rows[:, 0:9] = t["T"][:, :3, :3].reshape(V, 9)
    rows[:, 9:12] = t["T"][:, :3, 3]
    rows[:, 12:15] = t["pose_off"]
    return rows


def to_smpl(x, R, Th, dtype):
    """(x - Th) R, each component as (a R0c + b R1c) + c R2c."""
    x, R, Th = np.asarray(x, dtype=dtype), np.asarray(R, dtype=dtype).reshape(3, 3), np.asarray(Th, dtype=dtype).reshape(3)
    w = x - Th[None]
    return np.stack([(w[:, 0] * R[0, c] + w[:, 1] * R[1, c]) + w[:, 2] * R[2, c] for c in range(3)], axis=1)


def rotate(y, R, dtype):
    """R y for rows of y, each component as (y0 Ri0 + y1 Ri1) + y2 Ri2."""
    R = np.asarray(R, dtype=dtype).reshape(3, 3)
    return np.stack([(y[:, 0] * R[i, 0] + y[:, 1] * R[i, 1]) + y[:, 2] * R[i, 2] for i in range(3)], axis=1)


def distances(q, verts, dtype):
    """(N,V) squared distances (dx dx + dy dy) + dz dz."""
    s = np.asarray(verts, dtype=dtype)[:, :3]
    d = q[:, None, :] - s[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def normalize(v, dtype):
    with np.errstate(all="ignore"):
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok = (length > 0) & np.isfinite(length)
        out = v / np.where(ok, length, dtype(1))[:, None]
    return np.where(ok[:, None], out, dtype(0)).astype(dtype)


def blend(rows, ids, w, dtype):
    """M (N,3,3), c (N,3) of the stored ids and weights, k ascending."""
    rows = np.asarray(rows, dtype=dtype)
    N, K = ids.shape
    M, c = np.zeros((N, 3, 3), dtype=dtype), np.zeros((N, 3), dtype=dtype)
    for k in range(K):
        r = rows[ids[:, k]]
        R, t, po = r[:, 0:9].reshape(N, 3, 3), r[:, 9:12], r[:, 12:15]
        o = ((R[:, :, 0] * po[:, None, 0] + R[:, :, 1] * po[:, None, 1]) + R[:, :, 2] * po[:, None, 2]) + t
        M = M + w[:, k, None, None] * R
        c = c + w[:, k, None] * o
    return M, c


def cofactors(M):
    """The cofactor matrix C of M (N,3,3): M^-1 = C^T / det, det = (m00 C00 + m01 C01) + m02 C02."""
    C = np.empty_like(M)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            C[:, r, c] = M[:, r1, c1] * M[:, r2, c2] - M[:, r1, c2] * M[:, r2, c1]
    return C


def search(x, verts, R, Th, dtype=np.float64):
    """(q, d (N,V), order (N,V)): the part of bind that does not depend on K - bind takes it back as `found`."""
    q = to_smpl(x, R, Th, dtype)
    d = distances(q, verts, dtype)
    return q, d, np.argsort(d, axis=1, kind="stable")


def bind(x, n, verts, rows, R, Th, K, dtype=np.float64, transl=None, found=None):
    """-> dict ids (N,K) int64, weights (N,K), rest (N,3), rest_normals (N,3) or None, q (N,3), d_sorted (N, min(K + 1, V)): the
    smallest squared distances in order (what the tests take the near-ties from).  `verts` are the frame's SMPL-space vertices WITH
    its transl (verts4), `transl` that translation (SMPL-X; the rows do not hold it)."""
    q, d, order = search(x, verts, R, Th, dtype) if found is None else found
    ids = order[:, :K]
    dk = np.take_along_axis(d, ids, axis=1)
    w = dtype(1) / (dk + dtype(1e-8))
    total = np.zeros(len(q), dtype=dtype)
    for k in range(K):
        total = total + w[:, k]
    w = w / total[:, None]
    M, c = blend(rows, ids, w, dtype)
    C = cofactors(M)
    det = (M[:, 0, 0] * C[:, 0, 0] + M[:, 0, 1] * C[:, 0, 1]) + M[:, 0, 2] * C[:, 0, 2]
    inv = np.transpose(C, (0, 2, 1)) / det[:, None, None]
    e = (q if transl is None else q - np.asarray(transl, dtype=dtype).reshape(1, 3)) - c
    u = (inv[:, :, 0] * e[:, None, 0] + inv[:, :, 1] * e[:, None, 1]) + inv[:, :, 2] * e[:, None, 2]
    m = None
    if n is not None:
        s = to_smpl(n, R, np.zeros(3), dtype)
        m = normalize((M[:, 0, :] * s[:, None, 0] + M[:, 1, :] * s[:, None, 1]) + M[:, 2, :] * s[:, None, 2], dtype)
    assert u.dtype == dtype and w.dtype == dtype
    return {"ids": ids, "weights": w, "rest": u, "rest_normals": m, "q": q,
            "d_sorted": np.take_along_axis(d, order[:, :K + 1], axis=1)}


def repose(ids, w, u, m, rows, R, Th, transl=None, dtype=np.float64):
    """One frame -> (vertices (N,3) world, normals (N,3) or None)."""
    w, u = np.asarray(w, dtype=dtype), np.asarray(u, dtype=dtype)
    M, c = blend(rows, np.asarray(ids), w, dtype)
    y = ((M[:, :, 0] * u[:, None, 0] + M[:, :, 1] * u[:, None, 1]) + M[:, :, 2] * u[:, None, 2]) + c
    if transl is not None:
        y = y + np.asarray(transl, dtype=dtype).reshape(1, 3)
    world = rotate(y, R, dtype) + np.asarray(Th, dtype=dtype).reshape(1, 3)
    normals = None
    if m is not None:
        m = np.asarray(m, dtype=dtype)
        C = cofactors(M)
        g = normalize((C[:, :, 0] * m[:, None, 0] + C[:, :, 1] * m[:, None, 1]) + C[:, :, 2] * m[:, None, 2], dtype)
        normals = rotate(g, R, dtype)
    assert world.dtype == dtype
    return world, normals
