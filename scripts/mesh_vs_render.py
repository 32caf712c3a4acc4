"""A mesh image against the NeRF image of the same camera: does the extracted surface lie where the renderer sees the subject?

On the synthetic subject (the planted field of scripts/geometry_time.py): extract_mesh, then raster.rasterize and render_view with the
same K, R, T, pixel for pixel (both put pixel centres at integer coordinates).  Printed, per view: the silhouette IoU of acc > 0.5 and
the median and 95th percentile of |depth_mesh - depth_nerf| on the pixels both cover, after undoing the renderer's
depth_map = (d - near) / (far - near + 1e-5) with the near / far of camera_rays - both depths are then the ray parameter, which is
camera z.  A report, not a gate: no threshold is attached.  (The renderer's map is clamped to [0, 1], and it is the weighted mean of
the samples' depths rather than the depth of the level set; neither is corrected for.)

    python scripts/mesh_vs_render.py [--views 4] [--res 256] [--mesh-res 256] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--mesh-res", type=int, default=256)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--json")
    a = ap.parse_args()
    from geometry_time import setup
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import raster, render_view
    from humanliff_amd.SynBodyView_datasets import camera_rays
    dev = torch.device("cuda:0")
    renderer, tp, planes = setup(dev)
    mesh = renderer.extract_mesh(tp, planes, resolution=a.mesh_res)
    bounds = tp["world_bounds"].reshape(-1, 2, 3)[0].cpu().numpy()
    H = W = a.res
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    rows = []
    for view in range(a.views):
        K, c2w, cam = syn.orbit_camera(view, a.views, H, W)
        R = c2w.T
        T = -R @ cam
        m = raster.rasterize(mesh["vertices"], mesh["triangles"], H, W, K, R, T, normals=mesh["normals"], colors=mesh["colors"])
        rgb, acc, _, depth = render_view(H, W, K, R, T, planes, tp, renderer, n_samples=a.samples, n_importance=a.samples, generator=g)
        near, far = (t.reshape(H, W) for t in camera_rays(H, W, K, R, T, bounds, dev, return_mask=False)[2:4])
        depth_nerf = depth * (far - near + 1e-5) + near
        sm, sn = m["acc_map"][0] > 0.5, acc > 0.5
        both = sm & sn
        diff = (m["depth_map"][0] - depth_nerf).abs()[both]
        row = {"view": view, "mesh_pixels": int(sm.sum()), "nerf_pixels": int(sn.sum()), "iou": round(float(both.sum()) / max(int((sm | sn).sum()), 1), 4),
               "depth_abs_diff_median": round(float(diff.median()), 5) if diff.numel() else None,
               "depth_abs_diff_p95": round(float(torch.quantile(diff, 0.95)), 5) if diff.numel() else None,
               "rgb_abs_diff_mean": round(float((m["rgb_map"][0] - rgb).abs()[both].mean()), 4) if diff.numel() else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"res": a.res, "mesh_res": a.mesh_res, "vertices": int(mesh["vertices"].shape[0]), "triangles": int(mesh["triangles"].shape[0]), "views": rows,
           "iou_mean": round(float(np.mean([r["iou"] for r in rows])), 4)}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
