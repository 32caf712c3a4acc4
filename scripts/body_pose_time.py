"""What a posed body costs, at SMPL size (6 890 vertices, the synthetic model): the median of `--reps` runs, device time between two
HIP events and host-inclusive time (wall clock around a synchronise) of

  (a) the path before the hl_body kernels: NeRF/deform.py deform_tables with its cache cleared, the host fingerprint read included;
  (b) BodyModel.pose for 1 frame and for 64 frames (vertices, joints, bounds, verts4 and the table of every frame);
  (c) one canonical-space 128 x 128 view (64 + 64 samples) without prebuilt tables - a new pose per view (cache cleared) and the same
      pose again (cache hit, still fingerprinted) - and with them (tp_input['deform']).

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
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
