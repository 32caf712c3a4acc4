"""What simplifying a mesh costs, and what it saves downstream (humanliff_amd/NeRF/simplify.py, csrc/hl_mesh_simplify.hip; DESIGN.md
"Simplifying the mesh").

  simplify   the ellipsoid of scripts/mesh_raster_time.py - a latitude / longitude grid of `--quads`^2 quads, 708 gives 1 001 112
             triangles, the order of marching cubes at 512^3 - with normals and colours, clustered on cells of 2, 3 and 4 vertex spacings
             (a spacing: the side of a quad of the mesh's mean area).  A call is simplify._simplify: three entries of the library and the
             three host reads between and after them (bounds, cluster count, output counts and status).
  scale      on the same box in the same run: marching cubes alone at `--mc-res`^3 (the field of scripts/geometry_time.py), and
             bind_mesh + a 64-frame repose + rasterize of those frames at 512 x 512, on the full mesh and on each simplified one.

Device time between two HIP events around `--reps` back-to-back calls after two warm-up calls, per call; the parent starts `--procs`
fresh child processes one after another and reports the median and the range.  `--stages DIR` adds one more child under
`rocprofv3 --kernel-trace` (a run of its own, fewer calls, no scale part) and reports the mean time of every kernel per cell size.

    python scripts/mesh_simplify_time.py [--procs 3] [--reps 10] [--quads 708] [--mc-res 512] [--stages DIR] [--json out.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SPACINGS = (2, 3, 4)
FRAMES = 64
KERNELS = ("k_simplify_bounds_finish", "k_simplify_bounds", "k_simplify_mark", "k_simplify_ids", "k_simplify_members", "k_simplify_quadrics",
           "k_simplify_insert", "k_simplify_used", "k_simplify_solve", "k_simplify_vertex_map", "k_scan_reduce", "k_scan_top", "k_scan_down")


def mesh(q, dev):
    """The ellipsoid as simplify_mesh takes it: fp64 vertices and normals, int32 triangles, uint8 colours on the device, and its spacing."""
    import torch
    from mesh_raster_time import ellipsoid
    v, tri, n, col = ellipsoid(q, 1, dev)
    v = v[0].double().contiguous()
    a, b, c = (v[tri[:, k].long()] for k in range(3))
    area = float(torch.linalg.cross(b - a, c - a).norm(dim=1).sum()) / 2.0
    return v, tri, n.double().contiguous(), col, (area / (tri.shape[0] / 2.0)) ** 0.5


def pipeline(verts, tris, normals, colors, posed, cam, res):
    """bind_mesh + a FRAMES-frame repose + rasterize of those frames."""
    from humanliff_amd.NeRF import animate, raster
    binding = animate.bind_mesh(verts, posed, frame=0, neighbours=4, normals=normals)
    moved = binding.repose(posed, bounds=False)
    return raster.rasterize(moved["vertices"], tris, res, res, *cam, normals=moved["normals"], colors=colors, check_indices=False)


def child(a):
    import torch
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import geometry, raster, simplify
    from humanliff_amd.body import load_body_model
    from mesh_raster_time import per_call_ms
    dev = torch.device("cuda:0")
    v, tri, n, col, spacing = mesh(a.quads, dev)
    out = {"triangles": int(tri.shape[0]), "vertices": int(v.shape[0]), "spacing": spacing}
    small = {}
    for k in SPACINGS:
        run = lambda: simplify._simplify(v, tri, cell=k * spacing, normals=n, colors=col, check=False)  # noqa: E731
        out[f"simplify_{k}_ms"] = per_call_ms(run, a.reps)
        res, _, info = run()
        small[k] = res
        out[f"simplify_{k}_triangles"], out[f"simplify_{k}_vertices"], out[f"simplify_{k}_clusters"] = int(res["triangles"].shape[0]), int(res["vertices"].shape[0]), info["clusters"]
        out[f"simplify_{k}_grid"] = list(info["extents"])
    if a.scale:
        from geometry_time import setup
        r, tp, planes = setup(dev)
        sm = geometry.smooth_constrained(r.density_grid(tp, planes, resolution=a.mc_res))
        out["marching_cubes_ms"] = per_call_ms(lambda: geometry.marching_cubes(sm, 0.0), 3)
        out["marching_cubes_res"], out["marching_cubes_triangles"] = a.mc_res, int(geometry.marching_cubes(sm, 0.0)[1].shape[0])
        del sm
        model = load_body_model(syn.smpl_like_model(6890, 5), dev)
        poses = (torch.randn((FRAMES, 72), generator=syn._gen(9)) * 0.2).to(dev)
        posed = model.pose(poses, torch.zeros(10, device=dev), forward_rows=True)
        centre = posed.vertices[0].double().mean(dim=0)
        K, c2w, cam = syn.orbit_camera(1, 8, 512, 512)
        view = (K, c2w.T, -c2w.T @ cam)
        meshes = {"full": (v, tri, n, col)}
        meshes.update({f"simplified_{k}": (m["vertices"], raster.device_triangles(m["triangles"], dev), m["normals"], m["colors"]) for k, m in small.items()})
        for name, (mv, mt, mn, mc) in meshes.items():
            mv = (mv + centre[None]).float().contiguous()       # (the body is where the bind looks for neighbours; the camera follows)
            shifted = (view[0], view[1], view[2] - view[1] @ centre.cpu().numpy())
            out[f"bind_repose{FRAMES}_rasterize_{name}_ms"] = per_call_ms(lambda: pipeline(mv, mt, mn.float(), mc, posed, shifted, 512), 3)
    print("RESULT " + json.dumps(out), flush=True)


def stage_times(a):
    """One child under rocprofv3 --kernel-trace -> {cell: {kernel: mean us per call}}; the cells are told apart by the launch order:
    each is 2 + reps + 1 calls, in the order of child()."""
    os.makedirs(a.stages, exist_ok=True)
    reps = 3
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", a.stages, "--", sys.executable, os.path.abspath(__file__), "--child",
           "--reps", str(reps), "--quads", str(a.quads)]
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
                name = next((s for s in KERNELS if s in row["Kernel_Name"]), None)
                if name:
                    rows.append((int(row["Start_Timestamp"]), name, int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    calls = 2 + reps + 1
    starts = [i for i, r_ in enumerate(rows) if r_[1] == "k_simplify_bounds"]
    if len(starts) != calls * len(SPACINGS):
        raise SystemExit(f"{len(starts)} simplify calls in the trace, expected {calls * len(SPACINGS)}")
    out = {}
    for ci, k in enumerate(SPACINGS):
        lo = starts[ci * calls + 2]                                # (past the two warm-up calls)
        hi = starts[(ci + 1) * calls] if ci + 1 < len(SPACINGS) else len(rows)
        acc = {}
        for _, name, d in rows[lo:hi]:
            acc.setdefault(name, []).append(d)
        out[f"simplify_{k}"] = {name: round(sum(d) / (reps + 1) / 1e3, 2) for name, d in acc.items()}      # us per call, all launches of the kernel
        out[f"simplify_{k}"]["all_kernels"] = round(sum(sum(d) for d in acc.values()) / (reps + 1) / 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quads", type=int, default=708)
    ap.add_argument("--mc-res", type=int, default=512)
    ap.add_argument("--stages")
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scale", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scale", "--reps", str(a.reps), "--quads", str(a.quads), "--mc-res",
                            str(a.mc_res)], stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"a measuring process ended with status {r.returncode}")
        runs.append(json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    out = {"procs": a.procs, "reps": a.reps}
    for k in runs[0]:
        if k.endswith("_ms"):
            vals = [r[k] for r in runs]
            out[k] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
        else:
            out[k] = runs[0][k]
    T = out["triangles"]
    out["quadric_atomic_bytes_upper_bound"] = 3 * T * 10 * 8
    if a.stages:
        out["stage_us"] = stage_times(a)
        for k in SPACINGS:
            us = out["stage_us"][f"simplify_{k}"].get("k_simplify_quadrics", 0.0)
            if us:
                out[f"simplify_{k}_quadric_atomic_GBps_upper_bound"] = round(3 * T * 10 * 8 / (us * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
