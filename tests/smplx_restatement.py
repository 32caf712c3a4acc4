"""Float64 numpy restatement of posing an SMPL-X body, written from the formulas (Pavlakos et al., SMPL-X, 2019; Loper et al., SMPL,
2015, eq. 2-10) with the conventions of the smplx package as the reference runs it - the truth the kernels of csrc/hl_body.hip and the
fp32 torch path are both measured against.

    full_pose = global | body 21 | jaw | leye | reye | left hand 15 | right hand 15, + pose_mean           (165 values)
    coef = betas || expression;  directions = shapedirs[:, :, :nb] || shapedirs[:, :, e0:e0 + ne]
    v_shaped = v_template + directions . coef                    J = J_regressor v_shaped
    R_j = I + sin(a) K + (1 - cos(a)) K K,  a = |theta_j + 1e-8|,  K = [theta_j / a]x     (the package's Rodrigues: not exactly a rotation)
    v_posed = v_shaped + posedirs . vec(R_1 - I, ..., R_54 - I)
    G_0 = [R_0 | J_0],  G_i = G_parent(i) [R_i | J_i - J_parent(i)];  A_i = G_i with G_i [J_i; 0] taken off its last column
    T_v = sum_j w[v, j] A_j;   v = T_v [v_posed; 1] + transl;   joints_i = G_i[:3, 3] + transl;   world = v R^T + Th

The renderer's canonical-space table (NeRF/deform.py: deform_tables, after the reference's renderer.py:87, 364) is built from the SAME
poses and coefficients but from the first len(coef) RAW columns of shapedirs, and without transl: `table` below.
"""
import numpy as np

PARTS = (("global_orient", 1), ("body_pose", 21), ("jaw_pose", 1), ("leye_pose", 1), ("reye_pose", 1), ("left_hand_pose", 15),
         ("right_hand_pose", 15))
KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")


def model64(model):
    m = {k: np.asarray(model[k].numpy() if hasattr(model[k], "numpy") else model[k]).astype(np.float64) for k in KEYS}
    for k in ("hands_meanl", "hands_meanr"):
        m[k] = np.asarray(model[k].numpy() if hasattr(model[k], "numpy") else model[k]).astype(np.float64).reshape(-1)
    return m


def columns(n_cols, num_betas=10, num_expr=10):
    """(nb, e0, ne): body_models.py:1057-1077."""
    if n_cols < 400:
        return min(num_betas, 10), 10, min(num_expr, 10)
    return min(num_betas, 300), 300, min(num_expr, 100)


def pose_mean(m, flat_hand_mean):
    mean = np.zeros(165)
    if not flat_hand_mean:
        mean[75:120], mean[120:165] = m["hands_meanl"], m["hands_meanr"]
    return mean


def full_pose(parts, mean):
    """parts: dict of the part names -> (3n,) arrays (missing: zeros)."""
    return np.concatenate([np.asarray(parts[k], dtype=np.float64).reshape(-1) if parts.get(k) is not None else np.zeros(3 * n)
                           for k, n in PARTS]) + mean


def rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    a = np.linalg.norm(v + 1e-8)
    k = v / a
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def _lbs(m, parents, poses, sd, coef):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    J = poses.shape[0]
    shape_off = sd @ coef
    v_shaped = m["v_template"] + shape_off
    Jr = m["J_regressor"] @ v_shaped
    rot = np.stack([rodrigues(p) for p in poses])
    pose_off = m["posedirs"] @ (rot[1:] - np.eye(3)).reshape(-1)
    G = np.zeros((J, 4, 4))
    for i in range(J):
        local = np.eye(4)
        local[:3, :3] = rot[i]
        local[:3, 3] = Jr[i] if i == 0 else Jr[i] - Jr[parents[i]]
        G[i] = local if i == 0 else G[parents[i]] @ local
    A = G.copy()
    A[:, :3, 3] -= np.einsum("jrc,jc->jr", G[:, :3, :3], Jr)
    T = np.einsum("vj,jrc->vrc", m["weights"], A)
    v = np.einsum("vrc,vc->vr", T[:, :3, :3], v_shaped + pose_off) + T[:, :3, 3]
    return {"v": v, "joints": G[:, :3, 3].copy(), "T": T, "pose_off": pose_off, "shape_off": shape_off}


def pose(m, parents, poses, coef, cols, transl=None, R=None, Th=None):
    """One frame: poses = full_pose (165,), coef = betas || expression, cols = (nb, e0, ne) -> float64 world vertices (V,3), joints (55,3)."""
    nb, e0, ne = cols
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    assert coef.size == nb + ne
    sd = np.concatenate([m["shapedirs"][..., :nb], m["shapedirs"][..., e0:e0 + ne]], axis=-1)
    out = _lbs(m, parents, poses, sd, coef)
    tr = np.zeros(3) if transl is None else np.asarray(transl, dtype=np.float64).reshape(3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    Th = np.zeros(3) if Th is None else np.asarray(Th, dtype=np.float64).reshape(3)
    return {"vertices": (out["v"] + tr) @ R.T + Th, "joints": (out["joints"] + tr) @ R.T + Th}


def bounds(vertices32, y_margin=0.05):
    """SynBody_dataset.py:186-192 on float32 vertices, in float32."""
    v = np.asarray(vertices32)
    assert v.dtype == np.float32
    lo, hi = np.min(v, axis=0), np.max(v, axis=0)
    lo -= 0.05
    hi += 0.05
    lo[1] -= np.float32(y_margin)
    hi[1] += np.float32(y_margin)
    return np.stack([lo, hi], axis=0)


def table(m, parents, poses, coef, big_poses):
    """The 36 table columns per vertex, float64: t[3] Rinv[9] pose_off[3] shape_off[3] pose_off_big[3] Rbig[9] tbig[3] pad[3], from the
    first len(coef) raw columns of shapedirs; the big pose with zero coefficients.  Also the blended 3x3 of the target pose (V,3,3)."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    sd = m["shapedirs"][..., :coef.size]
    t, b = _lbs(m, parents, poses, sd, coef), _lbs(m, parents, big_poses, sd, np.zeros(coef.size))
    V = m["v_template"].shape[0]
    out = np.zeros((V, 36))
    out[:, 0:3] = t["T"][:, :3, 3]
    out[:, 3:12] = np.linalg.inv(t["T"][:, :3, :3]).reshape(V, 9)
    out[:, 12:15] = t["pose_off"]
    out[:, 15:18] = t["shape_off"]
    out[:, 18:21] = b["pose_off"]
    out[:, 21:30] = b["T"][:, :3, :3].reshape(V, 9)
    out[:, 30:33] = b["T"][:, :3, 3]
    return out, t["T"][:, :3, :3]
