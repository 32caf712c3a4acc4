"""Times the device view ingest (csrc/hl_view_ingest.hip) on V = 8 random 1024 x 1024 views, 1024^2 -> 512^2 (image_scaling 0.5) and
1024^2 -> 409^2 (0.4):

    ingest    HIP-event median of one hl_view_ingest call after warm-up, and the GB/s of the bytes it has to move (4 Hs Ws read,
              13 H W written per view); the upload of the uint8 source that precedes it is timed separately
    host      what a user had to do before: the float32 numpy restatement of the same rule on this machine's CPU
              (tests/view_ingest_restatement.py) plus the upload of its float32 image and uint8 mask; wall clock, median

--layers times the layered ingest of TightCap instead (hl_view_ingest_layers): V views with the cloth layers 0 .. 3 mixed, a
photograph and five mask planes each (8 source bytes a pixel), 512^2 at image_scaling 1.0 - TightCap's shipped configuration - and
1024^2 -> 512^2, against the numpy restatement of the same rule (tests/tightcap_restatement.py) plus its uploads.

One JSON line per measurement.  It has no pass mark.

    python scripts/view_ingest_time.py [--layers] [--views 8] [--iters 30] [--warmup 5] [--host-reps 3]
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

from humanliff_amd.view_ingest import ingest_layered_views, ingest_views               # noqa: E402

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


def body_planes(V, S):
    """Five (V, S, S) uint8 planes of a figure: a body ellipse, a top and a bottom a little wider than it that overlap in a band, shoes
    partly beside it, and `full`, their union."""
    yy, xx = np.mgrid[0:S, 0:S]
    u, w = (xx - S / 2.0) / S, (yy - S / 2.0) / S
    person = (u / 0.22) ** 2 + (w / 0.36) ** 2 <= 1.0
    wide = (u / 0.25) ** 2 + (w / 0.38) ** 2 <= 1.0
    top, bottom = wide & (w > -0.22) & (w < 0.02), wide & (w > -0.02) & (w < 0.28)
    shoes = (np.abs(w - 0.35) < 0.03) & (np.abs(u) < 0.12)
    planes = {"full": person | top | bottom | shoes, "person": person, "top": top, "bottom": bottom, "shoes": shoes}
    return {n: np.broadcast_to(p.astype(np.uint8) * 255, (V, S, S)).copy() for n, p in planes.items()}


def time_layers(args, dev):
    from tests import tightcap_restatement as tr
    V = args.views
    layers = [v % 4 for v in range(V)]
    rng = np.random.default_rng(0)
    for S, H in ((512, 512), (1024, 512)):
        img, planes = rng.integers(0, 256, (V, S, S, 3), dtype=np.uint8), body_planes(V, S)
        h_img, h_planes = torch.from_numpy(img).pin_memory(), {n: torch.from_numpy(p).pin_memory() for n, p in planes.items()}
        d_img, d_planes = h_img.to(dev), {n: p.to(dev) for n, p in h_planes.items()}
        up = event_median_ms(lambda: (h_img.to(dev, non_blocking=True), [p.to(dev, non_blocking=True) for p in h_planes.values()]), 2, 10)
        print(json.dumps({"what": "upload_u8_layers", "views": V, "from": [S, S], "ms": up, "GB_per_s": V * S * S * 8 / (up * 1e-3) / 1e9}), flush=True)
        ms = event_median_ms(lambda: ingest_layered_views(d_img, d_planes, layers, H, H), args.warmup, args.iters)
        read = sum(S * S * (3 + len(tr.GARMENTS[layer]) + 2 if layer < 3 else 4) for layer in layers)   # a layer reads only the planes it names
        moved = read + V * 13 * H * H
        print(json.dumps({"what": "ingest_layers", "views": V, "layers": layers, "from": [S, S], "to": [H, H], "ms": ms, "ms_per_view": ms / V,
                          "GB_per_s": moved / (ms * 1e-3) / 1e9}), flush=True)
        times = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            ref = tr.ingest(img, planes, layers, H, H)
            torch.from_numpy(ref["f32"]).to(dev), torch.from_numpy(ref["body"]).to(dev)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        host_ms = float(np.median(times)) * 1e3
        print(json.dumps({"what": "host_layers", "views": V, "from": [S, S], "to": [H, H], "ms": host_ms, "device_ingest_plus_upload_ms": ms + up,
                          "host_over_device": host_ms / (ms + up)}), flush=True)


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--layers", action="store_true", help="time the layered (TightCap) ingest instead")
    a.add_argument("--views", type=int, default=8)
    a.add_argument("--iters", type=int, default=30)
    a.add_argument("--warmup", type=int, default=5)
    a.add_argument("--host-reps", dest="host_reps", type=int, default=3)
    args = a.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_ingest_time.py needs a HIP device: humanliff_amd has no CPU path")
    from tests import view_ingest_restatement as vr
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.layers:
        return time_layers(args, dev)
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
