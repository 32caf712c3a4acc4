"""Generate golden vectors for posing an SMPL-X body FROM THE REFERENCE.

Runs only in the build container (needs /root/reference).

    python tests/golden/gen_golden_smplx.py

Reference entry points exercised (unmodified, imported from /root/reference/recon_NeRF):
    smplx.body_models.SMPLX.__init__ / forward, smplx.lbs.lbs           smplx/body_models.py:910-1087, 1118-1290; smplx/lbs.py
    SynBodyDatasetBatch.prepare_smpl_params / prepare_input / big_pose_params     lib/SynBody_dataset.py:135-225
What is NOT the reference here, and why:
  * the body model: SMPLX_NEUTRAL.npz is licensed data that is not in the repository.  humanliff_amd.synthetic.smplx_like_model at the
    official size (V = 10 475: the class indexes landmark vertices up to id 9929) is written to a temporary SMPLX_NEUTRAL.npz; the
    landmark arrays and hand PCA components the constructor insists on are random filler that no recorded output depends on;
  * the dataset object is made without __init__ (which reads three licensed files) and handed the model; cv2 / imageio are empty stubs.
The class is run twice, dtype=torch.float32 (through prepare_input, as the dataset runs it) and dtype=torch.float64 (forward on the same
inputs): recorded are the inputs, the float64 vertices and first 55 joints, full_pose, the fp32 bounds and the max-abs error of the fp32
run against the float64 run.  Bodies: 1 - pose N(0, 0.25^2) with one body joint and one finger joint exactly zero, random betas,
expression and transl, flat_hand_mean=True; 2 - the same inputs, flat_hand_mean=False; 3 - the dataset's big pose.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference/recon_NeRF")

for n in ["cv2", "imageio"]:
    if n not in sys.modules:
        try:
            __import__(n)
        except ImportError:
            sys.modules[n] = types.ModuleType(n)
if not hasattr(sys.modules["cv2"], "Rodrigues"):
    sys.modules["cv2"].Rodrigues = None          # (smpl_numpy.py imports the name; the SMPL-X path never calls it)

from smplx.body_models import SMPLX  # noqa: E402
from lib import SynBody_dataset as D  # noqa: E402

from humanliff_amd import synthetic as syn  # noqa: E402

V, SEED, ZERO_BODY_JOINT, ZERO_FINGER_JOINT = 10475, 23, 6, 9          # body_pose joint 6, left_hand_pose joint 9
PARTS = (("global_orient", 3), ("body_pose", 63), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3), ("left_hand_pose", 45), ("right_hand_pose", 45))


def write_model(path, model):
    g = np.random.default_rng(SEED)
    kt = model["kintree_table"].numpy().astype(np.int64)
    kt[0, 0] = 4294967295
    filler = {"lmk_faces_idx": g.integers(0, 1000, size=(51,)), "lmk_bary_coords": g.random((51, 3)),
              "dynamic_lmk_faces_idx": g.integers(0, 1000, size=(79, 17)), "dynamic_lmk_bary_coords": g.random((79, 17, 3)),
              "hands_componentsl": g.random((45, 45)), "hands_componentsr": g.random((45, 45))}
    np.savez(path, **{k: v.numpy() for k, v in model.items() if k not in ("kintree_table", "f")}, kintree_table=kt,
             f=g.integers(0, V, size=(20908, 3)).astype(np.uint32), **filler)


def inputs():
    g = syn._gen(SEED + 100)
    d = {k: (torch.randn((1, n), generator=g) * 0.25) for k, n in PARTS}
    d["body_pose"][0, 3 * ZERO_BODY_JOINT:3 * ZERO_BODY_JOINT + 3] = 0.0
    d["left_hand_pose"][0, 3 * ZERO_FINGER_JOINT:3 * ZERO_FINGER_JOINT + 3] = 0.0
    d["betas"] = torch.randn((1, 10), generator=g) * 0.5
    d["expression"] = torch.randn((1, 10), generator=g) * 0.5
    d["transl"] = torch.randn((1, 3), generator=g) * 0.3
    return {k: v.float().numpy() for k, v in d.items()}


def forward(model, prm, dtype):
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in prm.items() if k not in ("R", "Th")}
    with torch.no_grad():
        out = model(global_orient=t["global_orient"], betas=t["betas"], body_pose=t["body_pose"], jaw_pose=t["jaw_pose"],
                    left_hand_pose=t["left_hand_pose"], right_hand_pose=t["right_hand_pose"], leye_pose=t["leye_pose"], reye_pose=t["reye_pose"],
                    expression=t["expression"], transl=t["transl"], return_full_pose=True)
    return out.vertices[0].numpy(), out.joints[0, :55].numpy(), out.full_pose[0].numpy()


def main():
    data = {"seed": np.array(SEED), "V": np.array(V), "zero_body_joint": np.array(ZERO_BODY_JOINT), "zero_finger_joint": np.array(ZERO_FINGER_JOINT)}
    prm = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        write_model(os.path.join(tmp, "SMPLX_NEUTRAL.npz"), syn.smplx_like_model(V, SEED, 400))
        kw = dict(smpl_type="smplx", gender="neutral", use_face_contour=True, use_pca=False, num_betas=10, num_expression_coeffs=10, ext="npz")
        models = {(flat, dt): SMPLX(tmp, flat_hand_mean=flat, dtype=dt, **kw) for flat in (True, False) for dt in (torch.float32, torch.float64)}
        ds = D.SynBodyDatasetBatch.__new__(D.SynBodyDatasetBatch)
        ds.smpl_type = "smplx"
        big = ds.big_pose_params()
        for name, flat, p in (("b1", True, prm), ("b2", False, prm), ("b3", True, big)):
            # the fp32 run as the dataset makes it: a smplx.npz with two frames, the second one read
            two = {k: (v if k == "betas" else np.concatenate([np.zeros_like(v), v])) for k, v in p.items() if k not in ("R", "Th")}
            path = os.path.join(tmp, f"{name}.npz")
            np.savez(path, smplx=np.array(two, dtype=object), meta=np.array({"gender": "neutral"}, dtype=object))
            ds.smpl_model = {"neutral": models[(flat, torch.float32)]}
            wb, vertices32, params = ds.prepare_input(path, 1)
            _, joints32, _ = forward(models[(flat, torch.float32)], p, torch.float32)
            v64, j64, fp64 = forward(models[(flat, torch.float64)], p, torch.float64)
            assert vertices32.dtype == np.float32 and vertices32.shape == (V, 3) and j64.shape == (55, 3) and v64.dtype == np.float64
            for k, _ in PARTS + (("betas", 0), ("expression", 0), ("transl", 0)):
                data[f"{name}_{k}"] = np.asarray(p[k], dtype=np.float32)
            data[f"{name}_flat_hand_mean"] = np.array(flat)
            data[f"{name}_vertices"], data[f"{name}_joints"] = v64, j64
            data[f"{name}_full_pose"] = params["poses"].numpy().astype(np.float32).reshape(165)
            data[f"{name}_shapes"] = params["shapes"].numpy().astype(np.float32)
            data[f"{name}_bounds"] = wb.astype(np.float32)
            data[f"{name}_err_vertices"] = np.array(np.abs(vertices32.astype(np.float64) - v64).max())
            data[f"{name}_err_joints"] = np.array(np.abs(joints32.astype(np.float64) - j64).max())
            assert np.abs(fp64 - data[f"{name}_full_pose"]).max() < 1e-6
            print(name, "vertices mean-abs", float(np.abs(v64).mean()), "fp32 error: vertices", float(data[f"{name}_err_vertices"]), "joints",
                  float(data[f"{name}_err_joints"]), "bounds", wb.tolist())
    out = os.path.join(HERE, "smplx.npz")
    np.savez_compressed(out, **data)
    print("->", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
