"""Novel-pose animation through the canonical-space path: pose a body model for a sequence of frames on the device
(humanliff_amd.body), and render every frame from an orbiting or a fixed camera with the tables the posing made - what the reference's
`pose_num` / `pose_interval` dataset arguments exist for (SynBodyView_datasets.py:215-306).

    python scripts/render_pose_sequence.py --synthetic --out /tmp/seq [--frames 16] [--size 128] [--samples 64] [--fixed-camera]
    python scripts/render_pose_sequence.py --model assets/SMPL_NEUTRAL.pkl --poses poses.npz --planes planes.pt --mlp renderer.pt --out seq
    python scripts/render_pose_sequence.py --smpl_type smplx --model assets/models/smplx [--gender female] --poses subject/smplx.npz ... --out seq

--poses: an .npz with `poses` (F,72) and `shapes` (10,) or (F,10), optionally `R` (3,3) / (F,3,3) and `Th` (3,) / (F,3).
--planes: torch.save'd or .npy tri-planes (1,3,9,H,W) or (3,9,H,W); --mlp: the renderer's state dict.
--smpl_type smplx: --model is an SMPLX_{GENDER}.npz or the directory of them, --poses a SynBody smplx.npz (its 'smplx' dict; --frames of
its poses from the first on, the gender from its 'meta' unless --gender is given).  --synthetic takes the seeded
stand-ins of humanliff_amd.synthetic for whatever is not given (the licensed body model is not shipped) and a swinging-limbs sequence.
Frames are written as PNG (Pillow) or, without Pillow, as .npy; one JSON line of timings at the end.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_sequence(frames):
    """Arms and legs swinging about the big pose, the root turning slowly: (F,72) float32."""
    poses = np.zeros((frames, 72), dtype=np.float32)
    for f in range(frames):
        s = math.sin(2.0 * math.pi * f / max(frames, 1))
        poses[f, 1] = 0.3 * s                                   # root: about y
        poses[f, 5], poses[f, 8] = 0.5 + 0.3 * s, -0.5 + 0.3 * s  # hips: about z
        poses[f, 3], poses[f, 6] = 0.4 * s, -0.4 * s            # hips: about x
        poses[f, 50], poses[f, 53] = -0.8 + 0.4 * s, 0.8 + 0.4 * s  # shoulders: about z
    return poses


def load_array(path):
    a = np.load(path) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    return torch.as_tensor(a, dtype=torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model")
    ap.add_argument("--smpl_type", choices=["smpl", "smplx"], default="smpl")
    ap.add_argument("--gender", default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--poses")
    ap.add_argument("--planes")
    ap.add_argument("--mlp")
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--fixed-camera", action="store_true")
    ap.add_argument("--white-bkgd", action="store_true")
    a = ap.parse_args()
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.SynBodyView_datasets import camera_rays
    from humanliff_amd.body import load_body_model, load_smplx_model
    if not a.synthetic and not (a.model and a.poses and a.planes and a.mlp):
        ap.error("give --model, --poses, --planes and --mlp, or --synthetic for seeded stand-ins of what is missing")
    dev = torch.device("cuda:0")
    smplx = a.smpl_type == "smplx"
    if smplx:
        fitted, gender = None, a.gender or "neutral"
        if a.poses:
            with np.load(a.poses, allow_pickle=True) as z:
                fitted, gender = z["smplx"].item(), a.gender or z["meta"].item()["gender"]
            fitted = {k: np.asarray(v, dtype=np.float32) if k == "betas" else np.asarray(v, dtype=np.float32)[:a.frames] for k, v in fitted.items()}
        else:
            body_pose = synthetic_sequence(a.frames)[:, 3:66]
            fitted = {"global_orient": np.zeros((a.frames, 3), dtype=np.float32), "body_pose": body_pose, "betas": np.zeros((1, 10), dtype=np.float32),
                      "expression": np.zeros((a.frames, 10), dtype=np.float32)}
        model = load_smplx_model(a.model if a.model else syn.smplx_like_model(10475, 23), dev, gender=gender)
    else:
        model = load_body_model(a.model if a.model else syn.smpl_like_model(6890, 5), dev)
    if smplx:
        poses = shapes = R = Th = None
    elif a.poses:
        z = np.load(a.poses)
        poses, shapes = z["poses"].astype(np.float32).reshape(-1, 72), z["shapes"].astype(np.float32)
        R, Th = (z["R"] if "R" in z.files else None), (z["Th"] if "Th" in z.files else None)
    else:
        poses, shapes, R, Th = synthetic_sequence(a.frames), np.zeros(10, dtype=np.float32), None, None
    planes = load_array(a.planes) if a.planes else syn.triplane(seed=11)
    planes = planes.reshape(1, 3, 9, *planes.shape[-2:]).to(dev)
    r = Renderer(use_canonical_space=True, triplane_dim=planes.shape[-1], triplane_ch=27, smpl_type=a.smpl_type, test=True, body_model=model)
    r.load_state_dict(torch.load(a.mlp, map_location="cpu") if a.mlp else syn.render_mlp_state(3), strict=False)
    r = r.to(dev)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if smplx:
        posed = model.pose_dict({k: torch.from_numpy(v) for k, v in fitted.items()})                   # every frame in one call
    else:
        posed = model.pose(torch.from_numpy(poses).to(dev), torch.from_numpy(shapes).to(dev), R, Th)
    bounds = posed.bounds_host()                                                                       # the one read-back of the sequence
    t1 = time.perf_counter()
    os.makedirs(a.out, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    H = W = a.size
    F = posed.F
    images = []
    for f in range(F):
        K, c2w, cam = syn.orbit_camera(0 if a.fixed_camera else f, F, H, W)
        centre = 0.5 * (bounds[f, 0] + bounds[f, 1]).astype(np.float64)
        Rc = c2w.T
        ro, rd, nr, fr, _ = camera_rays(H, W, K, Rc, -Rc @ (cam + centre), bounds[f], dev, return_mask=False)
        u = torch.rand((1, H * W, a.samples), device=dev)
        out = r.render(posed.tp_input(f), None, None, ro[None], rd[None], nr[None, :, None], fr[None, :, None], planes, a.samples,
                       a.white_bkgd, n_samples=a.samples, u=u)
        images.append(out["rgb_map"].reshape(H, W, 3))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for f, img in enumerate(images):
        img8 = (img.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
        if Image is not None:
            Image.fromarray(img8).save(os.path.join(a.out, f"frame_{f:04d}.png"))
        else:
            np.save(os.path.join(a.out, f"frame_{f:04d}.npy"), img8)
    print(json.dumps(dict(frames=F, size=a.size, samples=a.samples, pose_ms=round((t1 - t0) * 1e3, 3),
                          render_ms_per_frame=round((t2 - t1) * 1e3 / F, 3), out=a.out)))


if __name__ == "__main__":
    main()
