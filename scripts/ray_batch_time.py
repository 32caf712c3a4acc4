"""Times the device ray batches (csrc/hl_ray_batch.hip) on synthetic 512 x 512 views:

    prepare   hl_ray_views_prepare per view, and the GB/s of the body masks it reads and the tables it writes
    batch     one hl_ray_batch launch at bs = 2, n = 2048 (uint8 store)
    fit       FitLoop iterations/s at the reference configuration (fit_loop_time.py's `main`: 100 instances, 2 x 2048 rays, 128 + 128
              samples), fed by RayBatchLoader and, in the same process, by pre-made resident batches cycled from a list (the path every
              earlier measurement of FitLoop used); wall clock over --iters iterations after --warmup, synchronised at both ends
    host      calls/s of the float64 numpy restatement of the reference's sample_ray_batch on this machine's CPU (tests/ray_batch_restatement.py)

One JSON line per measurement.

    python scripts/ray_batch_time.py [--views 16] [--iters 200] [--warmup 20] [--reps 3]
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

from humanliff_amd import synthetic as syn                                                              # noqa: E402
from humanliff_amd.recon_NeRF import Renderer                                                           # noqa: E402
from humanliff_amd.recon_NeRF.fit import FitLoop                                                        # noqa: E402
from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader, ViewStore, sample_ray_batch  # noqa: E402

KW = dict(lrate=5e-4, tri_plane_lrate=1e-1, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4, use_clamp=True, n_samples=128, n_importance=128,
          perturb=1., chunk=1024 * 64)
S, BS, N = 512, 2, 2048


def views(n_views, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    body = ((((xx - S / 2.0) / (0.22 * S)) ** 2 + ((yy - S / 2.0) / (0.36 * S)) ** 2) <= 1.0).astype(np.uint8)
    for v in range(n_views):
        K, c2w, cam = syn.orbit_camera(v, n_views, S, S)
        R = c2w.T.copy()
        yield rng.randint(0, 256, (S, S, 3)).astype(np.uint8), body, K, R, -R @ cam


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def make_model(dev):
    torch.manual_seed(0)
    m = Renderer(use_canonical_space=False, num_instances=1, triplane_dim=256, triplane_ch=27, test=False)
    m.load_state_dict(syn.render_mlp_state(3), strict=False)
    m = m.to(dev)
    m.tri_planes = torch.nn.Parameter(0.1 * torch.randn((100, 4, 3, 9, 256, 256), device=dev))
    return m


def fit_rate(model, batches, warmup, iters):
    """iterations/s of FitLoop.step over `batches` (an endless iterator), wall clock."""
    loop = FitLoop(model, None, **KW)
    for _ in range(warmup):
        loop.step(next(batches))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        loop.step(next(batches))
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def endless(loader):
    while True:
        yield from loader


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--views", type=int, default=16)
    a.add_argument("--iters", type=int, default=200)
    a.add_argument("--warmup", type=int, default=20)
    a.add_argument("--reps", type=int, default=3)
    args = a.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ray_batch_time.py needs a HIP device: humanliff_amd has no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    store = ViewStore(S, S, dev)
    vs = list(views(args.views))
    for i, (img, body, K, R, T) in enumerate(vs):
        store.add(img[None], body[None], K[None], R[None], T[None], syn.WORLD_BOUNDS, i % 100, i % 4)
    store.prepare()
    from humanliff_amd import _lib
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())                                                              # noqa: E731
    V, nw = len(store), (S + 63) // 64
    prep = event_ms(lambda: _lib.check(_lib.lib().hl_ray_views_prepare(p(store.corners), p(store.body), V, S, S, p(store.bitmaps),
                                                                       p(store.row_table), _lib.stream_ptr(dev))), 3, 20)
    moved = V * (S * S + 2 * S * nw * 8 + 3 * 2 * (S + 1) * 4)           # body read; bitmaps written; row table written, read, rewritten
    print(json.dumps({"what": "prepare", "views": V, "ms_per_view": prep / V, "GB_per_s": moved / (prep * 1e-3) / 1e9}), flush=True)
    idx = torch.tensor([1, 5 % V], device=dev)
    step = [0]

    def one():
        step[0] += 1
        sample_ray_batch(store, idx, N, seed=0, step=step[0])
    L = _lib.lib()
    out = sample_ray_batch(store, idx, N)
    raw = event_ms(lambda: L.hl_ray_batch(p(idx), BS, p(store.images), 1, p(store.bitmaps), p(store.row_table), p(store.cameras), V, S, S, N, 0.8,
                                          None, 0, 0, 32, *(p(out[k].view(torch.uint8) if out[k].dtype == torch.bool else out[k]) for k in
                                          ("rgb", "ray_o", "ray_d", "near", "far", "bkgd_msk", "mask_at_box", "coord", "n_valid")),
                                          _lib.stream_ptr(dev)), 10, 200)
    print(json.dumps({"what": "batch", "bs": BS, "n_rays": N, "launch_us": raw * 1e3, "with_python_wrapper_us": event_ms(one, 10, 200) * 1e3,
                      "n_valid": out["n_valid"].tolist()}), flush=True)
    # FitLoop fed two ways, alternating so that drift hits both alike
    loader = RayBatchLoader(store, BS, N, seed=0)
    premade = [next(endless(RayBatchLoader(store, BS, N, seed=s))) for s in range(8)]

    def cycle():
        i = 0
        while True:
            yield premade[i % len(premade)]
            i += 1
    rates = {"loader": [], "premade": []}
    for _ in range(args.reps):
        rates["premade"].append(fit_rate(make_model(dev), cycle(), args.warmup, args.iters))
        rates["loader"].append(fit_rate(make_model(dev), endless(loader), args.warmup, args.iters))
    print(json.dumps({"what": "fit", "iterations_per_s": rates, "loader_over_premade": float(np.median(rates["loader"]) / np.median(rates["premade"]))}),
          flush=True)
    # the reference's host path, restated
    from tests import ray_batch_restatement as rs
    img, body, K, R, T = vs[1]
    imgf = img.astype(np.float32) / 255.
    rng = np.random.RandomState(0)
    picks = rng.randint(0, 10000, (32, 2, N))
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < 3.0:
        rs.sample_ray_batch(imgf, body, K, R, T.reshape(3, 1), np.asarray(syn.WORLD_BOUNDS), N, picks)
        calls += 1
    print(json.dumps({"what": "host", "restatement_calls_per_s": calls / (time.perf_counter() - t0)}), flush=True)


if __name__ == "__main__":
    main()
