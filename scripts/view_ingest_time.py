"""Times the device view ingest (csrc/hl_view_ingest.hip) on V = 8 random 1024 x 1024 views, 1024^2 -> 512^2 (image_scaling 0.5) and
1024^2 -> 409^2 (0.4):

    ingest    HIP-event median of one hl_view_ingest call after warm-up, and the GB/s of the bytes it has to move (4 Hs Ws read,
              13 H W written per view); the upload of the uint8 source that precedes it is timed separately
    host      what a user had to do before: the float32 numpy restatement of the same rule on this machine's CPU
              (tests/view_ingest_restatement.py) plus the upload of its float32 image and uint8 mask; wall clock, median

One JSON line per measurement.  It has no pass mark.

    python scripts/view_ingest_time.py [--views 8] [--iters 30] [--warmup 5] [--host-reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from humanliff_amd.view_ingest import ingest_views               # noqa: E402

S = 1024


def event_median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in pairs]))


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--views", type=int, default=8)
    a.add_argument("--iters", type=int, default=30)
    a.add_argument("--warmup", type=int, default=5)
    a.add_argument("--host-reps", dest="host_reps", type=int, default=3)
    args = a.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_ingest_time.py needs a HIP device: humanliff_amd has no CPU path")
    from tests import view_ingest_restatement as vr
    dev = torch.device("cuda", torch.cuda.current_device())
    V = args.views
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (V, S, S, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    msk = np.broadcast_to(((((xx - S / 2.0) / (0.22 * S)) ** 2 + ((yy - S / 2.0) / (0.36 * S)) ** 2) <= 1.0).astype(np.uint8) * 255, (V, S, S)).copy()
    h_img, h_msk = torch.from_numpy(img).pin_memory(), torch.from_numpy(msk).pin_memory()
    d_img, d_msk = h_img.to(dev), h_msk.to(dev)
    up = event_median_ms(lambda: (h_img.to(dev, non_blocking=True), h_msk.to(dev, non_blocking=True)), 2, 10)
    print(json.dumps({"what": "upload_u8", "views": V, "ms": up, "GB_per_s": V * S * S * 4 / (up * 1e-3) / 1e9}), flush=True)
    for scaling in (0.5, 0.4):
        H = W = int(S * scaling)
        ms = event_median_ms(lambda: ingest_views(d_img, d_msk, H, W), args.warmup, args.iters)
        moved = V * (4 * S * S + 13 * H * W)
        print(json.dumps({"what": "ingest", "views": V, "from": [S, S], "to": [H, W], "ms": ms, "ms_per_view": ms / V,
                          "GB_per_s": moved / (ms * 1e-3) / 1e9}), flush=True)
        times = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            image = vr.resize_area_f32(vr.masked_source(img, msk), H, W)
            body = vr.resize_nearest(msk, H, W)
            torch.from_numpy(image).to(dev), torch.from_numpy(body).to(dev)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        host_ms = float(np.median(times)) * 1e3
        print(json.dumps({"what": "host", "views": V, "to": [H, W], "ms": host_ms, "device_ingest_plus_upload_ms": ms + up,
                          "host_over_device": host_ms / (ms + up)}), flush=True)


if __name__ == "__main__":
    main()
