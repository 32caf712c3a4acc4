"""What rasterising a mesh costs (humanliff_amd/NeRF/raster.py, csrc/hl_mesh_raster.hip; DESIGN.md "Rasterising the mesh").

  micro   a closed analytic surface - an ellipsoid of body proportions, a latitude / longitude grid of `--quads`^2 quads, two triangles
          each: 708 gives 1.0 M triangles, the order of marching cubes at 512^3 - seen at 512 x 512 by the synthetic orbit camera, F in
          {1, 16, 64} frames (the surface breathing from frame to frame), normals and colours given.  A triangle is smaller than a pixel.
  box     a 12-triangle box that fills the view: every triangle goes through the large list.

Device time between two HIP events around `--reps` back-to-back calls after two warm-up calls, per call; the parent starts `--procs`
fresh child processes one after another and reports the median and the range.  Next to every time: what the cover stage must gather
(12 bytes of indices and three 16-byte records per triangle and image) and the fragments (covered triangle-pixel pairs; the ellipsoid
is convex, so they are twice the silhouette's pixels) - each fragment is at most one 64-bit atomic, fewer where the plain load settles it.

`--stages DIR` adds one more child under `rocprofv3 --kernel-trace` (a run of its own, fewer calls), writing its trace under DIR, and
reports the mean time of every k_raster_* kernel per case from it.

    python scripts/mesh_raster_time.py [--procs 3] [--reps 10] [--quads 708] [--res 512] [--stages DIR] [--json out.json]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = (1, 16, 64)
STAGES = ("k_raster_cameras", "k_raster_clear", "k_raster_project", "k_raster_cover_large", "k_raster_cover", "k_raster_resolve")


def per_call_ms(fn, reps):
    import torch
    for _ in range(2):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def ellipsoid(q, frames, dev):
    """vertices (frames, q (q - 1) + 2, 3), triangles (2 q (q - 1), 3), normals, colours: device tensors; rows of latitude in order, so
    that neighbouring triangles name neighbouring vertices, as marching cubes' lattice order does."""
    import numpy as np
    import torch
    rad = np.array([0.35, 0.85, 0.25])
    lat = np.pi * (np.arange(1, q) / q)                           # the poles are two vertices of their own
    lon = 2 * np.pi * np.arange(q) / q
    u = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.ones(q)[None], np.sin(lat)[:, None] * np.sin(lon)[None]], axis=-1)
    u = np.concatenate([u.reshape(-1, 3), [[0, 1, 0], [0, -1, 0]]])
    ring = np.arange(q)
    a = (np.arange(q - 2)[:, None] * q + ring[None]).reshape(-1)
    b = (np.arange(q - 2)[:, None] * q + (ring[None] + 1) % q).reshape(-1)
    north, south, last = (q - 1) * q, (q - 1) * q + 1, (q - 2) * q
    tri = np.concatenate([np.stack([a, b, b + q], 1), np.stack([a, b + q, a + q], 1),
                          np.stack([np.full(q, north), (ring + 1) % q, ring], 1), np.stack([np.full(q, south), last + ring, last + (ring + 1) % q], 1)])
    n = u / rad
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    scale = 1.0 + 0.03 * np.sin(np.arange(frames) * 0.7)
    v = torch.from_numpy((u * rad).astype(np.float32)).to(dev)[None] * torch.from_numpy(scale.astype(np.float32)).to(dev)[:, None, None]
    col = torch.from_numpy(np.clip(127 + 120 * n, 0, 255).astype(np.uint8)).to(dev)
    return v.contiguous(), torch.from_numpy(tri.astype(np.int32)).to(dev), torch.from_numpy(n.astype(np.float32)).to(dev), col


def view_box(K, c2w, cam, res, dev):
    """A box in front of the camera whose near face reaches beyond the image on every side."""
    import numpy as np
    import torch
    Ki = np.linalg.inv(K)
    c = [cam + c2w @ (Ki @ np.array([sx, sy, 1.0]) * d) for d in (2.0, 3.0) for sy in (-0.2 * res, 1.2 * res) for sx in (-0.2 * res, 1.2 * res)]
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = [t for a, b, c_, d in q for t in ((a, b, c_), (a, c_, d))]
    return torch.tensor(np.array(c), dtype=torch.float32, device=dev), torch.tensor(tri, dtype=torch.int32, device=dev)


def child(a):
    import numpy as np
    import torch
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import raster
    dev = torch.device("cuda:0")
    res = a.res
    K, c2w, cam = syn.orbit_camera(1, 8, res, res)
    R = c2w.T
    T = -R @ cam
    v, tri, n, col = ellipsoid(a.quads, max(FS), dev)
    out = {"triangles": int(tri.shape[0]), "vertices": int(v.shape[1])}
    for F in FS:
        run = lambda: raster.rasterize(v[:F], tri, res, res, K, R, T, normals=n, colors=col, check_indices=False)  # noqa: E731
        out[f"micro_F{F}_ms"] = per_call_ms(run, a.reps)
        out[f"micro_F{F}_silhouette_pixels"] = int(run()["acc_map"].sum().item())
    bv, bt = view_box(K, c2w, cam, res, dev)
    for F in (1, 64):
        vs = bv[None].expand(F, -1, -1).contiguous()
        run = lambda: raster.rasterize(vs, bt, res, res, K, R, T, check_indices=False)  # noqa: E731
        out[f"box_F{F}_ms"] = per_call_ms(run, a.reps)
        out[f"box_F{F}_silhouette_pixels"] = int(run()["acc_map"].sum().item())
    print("RESULT " + json.dumps(out), flush=True)


def stage_times(a):
    """One child under rocprofv3 --kernel-trace -> {case: {kernel: mean us}}; the cases are told apart by the launch order: each case
    is 2 + reps + 1 calls of every kernel, in the order of child()."""
    os.makedirs(a.stages, exist_ok=True)
    reps = 3
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", a.stages, "--", sys.executable, os.path.abspath(__file__), "--child",
           "--reps", str(reps), "--quads", str(a.quads), "--res", str(a.res)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"the profiled process ended with status {r.returncode}:\n{r.stdout[-2000:]}")
    files = glob.glob(os.path.join(a.stages, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.stages}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = next((s for s in STAGES if s in row["Kernel_Name"]), None)
                if name:
                    rows.append((int(row["Start_Timestamp"]), name, int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    cases = [f"micro_F{F}" for F in FS] + ["box_F1", "box_F64"]
    calls = 2 + reps + 1
    out = {}
    starts = [i for i, r_ in enumerate(rows) if r_[1] == "k_raster_clear"]
    if len(starts) != calls * len(cases):
        raise SystemExit(f"{len(starts)} raster calls in the trace, expected {calls * len(cases)}")
    for ci, case in enumerate(cases):
        lo = starts[ci * calls + 2]                                # (past the two warm-up calls)
        hi = starts[(ci + 1) * calls] if ci + 1 < len(cases) else len(rows)
        acc = {}
        for _, name, d in rows[lo:hi]:
            acc.setdefault(name, []).append(d)
        out[case] = {k: round(sum(d) / (reps + 1) / 1e3, 2) for k, d in acc.items() if k != "k_raster_cameras"}      # us per call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quads", type=int, default=708)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--stages")
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--quads", str(a.quads), "--res", str(a.res)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"a measuring process ended with status {r.returncode}")
        runs.append(json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    out = {"res": a.res, "procs": a.procs, "reps": a.reps, "triangles": runs[0]["triangles"], "vertices": runs[0]["vertices"]}
    for k in runs[0]:
        if k.endswith("_ms"):
            vals = [r[k] for r in runs]
            out[k] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
        elif k.endswith("_pixels"):
            out[k] = runs[0][k]
    if a.stages:
        out["stage_us"] = stage_times(a)
        T = out["triangles"]
        for F in FS:
            us = out["stage_us"][f"micro_F{F}"]
            cover = us.get("k_raster_cover", 0.0) * 1e-6
            frags = 2 * out[f"micro_F{F}_silhouette_pixels"]
            out[f"micro_F{F}_cover_gather_GBps"] = round(T * F * 60 / cover / 1e9, 1)
            out[f"micro_F{F}_cover_fragments_per_s"] = round(frags / cover, 0)
            out[f"micro_F{F}_project_GBps"] = round(out["vertices"] * F * 28 / (us.get("k_raster_project", 0.0) * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
