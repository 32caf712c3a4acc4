"""What a posed body costs, at SMPL size (6 890 vertices, the synthetic model): the median of `--reps` runs, device time between two
HIP events and host-inclusive time (wall clock around a synchronise) of

  (a) the path before the hl_body kernels: NeRF/deform.py deform_tables with its cache cleared, the host fingerprint read included;
  (b) BodyModel.pose for 1 frame and for 64 frames (vertices, joints, bounds, verts4 and the table of every frame);
  (c) one canonical-space 128 x 128 view (64 + 64 samples) without prebuilt tables - a new pose per view (cache cleared) and the same
      pose again (cache hit, still fingerprinted) - and with them (tp_input['deform']).

  (d) at SMPL-X size (10 475 vertices, 55 joints, a 400-column synthetic model): SmplxModel.pose for 1 frame and for 64 frames, and the
      same rule - vertices, joints and bounds; no table - in fp32 torch ops on the device (NeRF/deform.py's generic functions, frame by frame).

    python scripts/body_pose_time.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def medians(fn, reps, before=None):
    """(median device ms, median host-inclusive ms) of fn() over reps runs, after two warm-up calls."""
    dev_ms, host_ms = [], []
    for i in range(reps + 2):
        if before is not None:
            before()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= 2:
            dev_ms.append(start.elapsed_time(stop))
            host_ms.append((t1 - t0) * 1e3)
    return round(statistics.median(dev_ms), 4), round(statistics.median(host_ms), 4)


def smplx_torch_rule(model, poses, coef, transl):
    """SMPLX.forward + the dataset's bounds for every frame in torch ops on the model's device: poses (F,165) full poses, coef (F,20)."""
    from humanliff_amd.NeRF import deform
    t = model.tensors
    sd = torch.cat([t["shapedirs"][..., :model.num_betas], t["shapedirs"][..., model.expr_start:model.expr_start + model.num_expr]], dim=-1)
    m = dict(t, shapedirs=sd)
    V = model.V
    out = []
    for f in range(poses.shape[0]):
        A = deform.joint_transforms(m, poses[f], coef[f])
        T = (t["weights"] @ A.reshape(-1, 16)).reshape(V, 4, 4)
        v_shaped = t["v_template"] + sd @ coef[f]
        vh = torch.cat([v_shaped + deform._pose_offsets(m, poses[f]), torch.ones((V, 1), device=poses.device)], dim=1)
        v = torch.matmul(T, vh[:, :, None])[:, :3, 0] + transl[f]
        rest = t["J_regressor"] @ v_shaped
        joints = torch.matmul(A[:, :3, :3], rest[:, :, None])[:, :, 0] + A[:, :3, 3] + transl[f]
        lo, hi = v.amin(dim=0) - 0.05, v.amax(dim=0) + 0.05
        lo[1] -= 0.05
        hi[1] += 0.05
        out.append((v, joints, torch.stack([lo, hi])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer, deform
    from humanliff_amd.SynBodyView_datasets import camera_rays
    from humanliff_amd.body import load_body_model
    dev = torch.device("cuda:0")
    model = load_body_model(syn.smpl_like_model(6890, 5), dev)
    g = syn._gen(3)
    poses = (torch.randn((64, 72), generator=g) * 0.25).to(dev)
    shapes = (torch.randn((10,), generator=g) * 0.5).to(dev)
    Rw, Th = syn._rodrigues1(torch.tensor([0.2, -0.3, 0.1])).numpy(), torch.tensor([0.1, -0.2, 0.3]).numpy()
    posed = model.pose(poses[:1], shapes, Rw, Th)
    tp = posed.tp_input(0)
    plain = {k: v for k, v in tp.items() if k != "deform"}
    out = {"V": 6890, "reps": a.reps}

    def tables():
        return deform.deform_tables(model.tensors, plain["params"], plain["t_params"], plain["vertices"])
    out["a_deform_tables_ms"] = dict(zip(("device", "host_inclusive"), medians(tables, a.reps, before=deform._TABLE_CACHE.clear)))
    out["b_pose_1_frame_ms"] = dict(zip(("device", "host_inclusive"), medians(lambda: model.pose(poses[:1], shapes, Rw, Th), a.reps)))
    out["b_pose_64_frames_ms"] = dict(zip(("device", "host_inclusive"), medians(lambda: model.pose(poses, shapes, Rw, Th), a.reps)))

    H = W = 128
    N = 64
    r = Renderer(use_canonical_space=True, triplane_dim=256, triplane_ch=27, test=True, body_model=model)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(dev)
    planes = syn.triplane(seed=11).to(dev)
    bounds = posed.bounds_host()[0]
    K, c2w, cam = syn.orbit_camera(3, 36, H, W)
    Rc = c2w.T
    centre = 0.5 * (bounds[0] + bounds[1]).astype("float64")
    ro, rd, nr, fr, _ = camera_rays(H, W, K, Rc, -Rc @ (cam + centre), bounds, dev, return_mask=False)
    u = torch.rand((1, H * W, N), device=dev)

    def view(t):
        return lambda: r.render(t, None, None, ro[None], rd[None], nr[None, :, None], fr[None, :, None], planes, N, False, n_samples=N, u=u)
    out["c_view_128_new_pose_ms"] = dict(zip(("device", "host_inclusive"), medians(view(plain), a.reps, before=deform._TABLE_CACHE.clear)))
    out["c_view_128_same_pose_ms"] = dict(zip(("device", "host_inclusive"), medians(view(plain), a.reps)))
    out["c_view_128_prebuilt_ms"] = dict(zip(("device", "host_inclusive"), medians(view(tp), a.reps)))
    out["pose_1_frame_no_slower_than_deform_tables"] = out["b_pose_1_frame_ms"]["host_inclusive"] <= out["a_deform_tables_ms"]["host_inclusive"]

    from humanliff_amd.body import load_smplx_model
    xm = load_smplx_model(syn.smplx_like_model(10475, 23, 400), dev)
    g = syn._gen(4)
    parts = [(torch.randn((64, n), generator=g) * 0.25).to(dev) for n in (3, 63, 3, 3, 3, 45, 45)]
    betas, expr, transl = [(torch.randn(s, generator=g) * 0.5).to(dev) for s in ((1, 10), (64, 10), (64, 3))]

    def xpose(F):
        go, bp, jaw, le, re, lh, rh = [p[:F] for p in parts]
        return lambda: xm.pose(go, bp, betas, expr[:F], jaw, le, re, lh, rh, transl[:F])
    first = xpose(64)()
    out["smplx_V"] = 10475
    for F in (1, 64):
        out[f"d_smplx_pose_{F}_frame{'s' if F > 1 else ''}_ms"] = dict(zip(("device", "host_inclusive"), medians(xpose(F), a.reps)))
        out[f"d_smplx_torch_ops_{F}_frame{'s' if F > 1 else ''}_ms"] = dict(zip(("device", "host_inclusive"), medians(
            lambda: smplx_torch_rule(xm, first.poses[:F], first.shapes[:F], transl), a.reps)))
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
