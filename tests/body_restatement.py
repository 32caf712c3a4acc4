"""Float64 numpy restatement of posing the body model, written from the formulas (Loper et al., SMPL, 2015, eq. 2-10; the bounds of
SynBodyView_datasets.py:170-179; the table columns NeRF/deform.py: deform_tables documents) - the truth the HIP kernels of
csrc/hl_body.hip and today's fp32 torch path are both measured against.

    v_shaped = v_template + shapedirs . beta                     J = J_regressor v_shaped
    R_j = exp([theta_j]x)  (Rodrigues; the identity at theta = 0)
    v_posed = v_shaped + posedirs . vec(R_1 - I, ..., R_{J-1} - I)
    G_0 = [R_0 | J_0],  G_i = G_parent(i) [R_i | J_i - J_parent(i)]     posed joint i = G_i[:3, 3]
    A_i = G_i with G_i [J_i; 0] taken off its last column
    T_v = sum_j w[v, j] A_j          v_smpl = T_v [v_posed; 1]          world = v_smpl R^T + Th

`rot_dtype=np.float32` rounds the joint rotations to float32 as smpl_numpy.py:62-65 stores them: the golden vectors carry that rounding.
"""
import numpy as np


def rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    a = np.linalg.norm(v)
    if a == 0.0:
        return np.eye(3)
    k = v / a
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def model64(model):
    """The float32 model tensors (dict of torch tensors or arrays) as float64 numpy, the shape directions cut to `S` later."""
    return {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v).astype(np.float64) for k, v in model.items()
            if k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}


def pose(m, parents, poses, shapes, R=None, Th=None, rot_dtype=np.float64):
    """One frame: dict of float64 arrays - vertices (V,3) and joints (J,3) in the world, v_smpl, A (J,4,4), T (V,4,4), pose_off,
    shape_off (V,3)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    shapes = np.asarray(shapes, dtype=np.float64).reshape(-1)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    Th = np.zeros(3) if Th is None else np.asarray(Th, dtype=np.float64).reshape(3)
    J = poses.shape[0]
    shape_off = m["shapedirs"][..., :shapes.size] @ shapes
    v_shaped = m["v_template"] + shape_off
    Jr = m["J_regressor"] @ v_shaped
    rot = np.stack([rodrigues(p) for p in poses]).astype(rot_dtype).astype(np.float64)
    pose_off = m["posedirs"] @ (rot[1:] - np.eye(3)).reshape(-1)
    v_posed = v_shaped + pose_off
    G = np.zeros((J, 4, 4))
    for i in range(J):
        local = np.eye(4)
        local[:3, :3] = rot[i]
        local[:3, 3] = Jr[i] if i == 0 else Jr[i] - Jr[parents[i]]
        G[i] = local if i == 0 else G[parents[i]] @ local
    joints = G[:, :3, 3].copy()
    A = G.copy()
    A[:, :3, 3] -= np.einsum("jrc,jc->jr", G[:, :3, :3], Jr)
    T = np.einsum("vj,jrc->vrc", m["weights"], A)
    v_smpl = np.einsum("vrc,vc->vr", T[:, :3, :3], v_posed) + T[:, :3, 3]
    return {"vertices": v_smpl @ R.T + Th, "joints": joints @ R.T + Th, "v_smpl": v_smpl, "A": A, "T": T, "pose_off": pose_off,
            "shape_off": shape_off}


def bounds(vertices32):
    """SynBodyView_datasets.py:170-179 on float32 vertices, in float32: min / max, - / + 0.05, y once more by 0.05."""
    v = np.asarray(vertices32)
    assert v.dtype == np.float32
    lo, hi = np.min(v, axis=0), np.max(v, axis=0)
    lo -= 0.05
    hi += 0.05
    lo[1] -= 0.05
    hi[1] += 0.05
    return np.stack([lo, hi], axis=0)


def table(m, parents, poses, shapes, big_poses):
    """The 36 columns of the deformation table per vertex, float64: t[3] Rinv[9] pose_off[3] shape_off[3] pose_off_big[3] Rbig[9]
    tbig[3] pad[3]; the big pose is posed with zero shapes.  Also returns the blended 3x3 of the target pose (V,3,3)."""
    t = pose(m, parents, poses, shapes)
    b = pose(m, parents, big_poses, np.zeros(np.asarray(shapes).size))
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
