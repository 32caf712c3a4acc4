"""Times held-out view scoring: humanliff_amd.metrics.image_metrics on the device (HIP events), the float64 numpy / scipy restatement
of the reference's host path with its device-to-host copies (tests/metrics_restatement.py - a restatement, not skimage), and the render
of the view that is scored (128 + 128 samples, resident uniforms).

    python scripts/metrics_time.py [--sizes 512 1024] [--views 1 8] [--reps 10] [--json out.json]

The images are the rendered view as the prediction and the same view plus noise as the ground truth; the mask is the bounds box mask
of an orbit camera (SynBodyView_datasets.camera_rays).  One JSON line per (size, V).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def events_ms(fn, reps):
    """Mean device time of fn() in ms between two HIP events, after one warm-up call."""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--views", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd import metrics, synthetic as syn
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.SynBodyView_datasets import camera_rays
    from tests import metrics_restatement as mr
    dev = torch.device("cuda:0")
    planes = syn.triplane(seed=11).to(dev)
    r = Renderer(use_canonical_space=False, triplane_ch=27, test=True)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(dev)
    tp = {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}
    rows = []
    for S in a.sizes:
        K, c2w, cam = syn.orbit_camera(3, 36, S, S)
        R = c2w.T
        ro, rd, nr, fr, mask = camera_rays(S, S, K, R, -R @ cam, syn.WORLD_BOUNDS, dev, return_mask=True)
        u = torch.rand((S * S, 128), device=dev)

        def render():
            return r.render(tp, None, None, ro[None], rd[None], nr[None, :, None], fr[None, :, None], planes, 128, False, n_samples=128, u=u[None])

        render_ms = events_ms(render, max(a.reps // 3, 2))
        pred1 = render()["rgb_map"].reshape(1, S, S, 3).float().contiguous()
        gt1 = (pred1 + (torch.rand_like(pred1) - 0.5) * 0.1).contiguous()
        mask1 = mask.reshape(1, S, S)
        for V in a.views:
            pred, gt, m = pred1.expand(V, S, S, 3).contiguous(), gt1.expand(V, S, S, 3).contiguous(), mask1.expand(V, S, S).contiguous()
            dev_ms = events_ms(lambda: metrics.image_metrics(pred, gt, m), a.reps)
            dev_u8_ms = events_ms(lambda: metrics.image_metrics(pred, gt, m, return_uint8=True), a.reps)
            got = metrics.image_metrics_host(pred, gt, m)
            # the host path of one view, as the reference runs it: copy the two images and the mask back, score them in float64
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p_h, g_h, m_h = pred[0].cpu().numpy(), gt[0].cpu().numpy(), m[0].cpu().numpy()
            t1 = time.perf_counter()
            want = mr.view_metrics(p_h, g_h, m_h)
            t2 = time.perf_counter()
            row = dict(size=S, views=V, box=[int(t) for t in got["bbox"][0]], masked=int(got["count"][0]),
                       device_ms_per_view=round(dev_ms / V, 4), device_with_uint8_ms_per_view=round(dev_u8_ms / V, 4),
                       host_restatement_ms_per_view=round((t2 - t0) * 1e3, 1), host_copy_ms_per_view=round((t1 - t0) * 1e3, 2),
                       render_ms_per_view=round(render_ms, 2), ssim=float(got["ssim"][0]), ssim_error=abs(float(got["ssim"][0]) - want["ssim"]),
                       mse_relative_error=abs(float(got["mse"][0]) - want["mse"]) / want["mse"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
