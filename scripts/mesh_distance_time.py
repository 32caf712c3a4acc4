"""What measuring mesh distance costs (humanliff_amd/NeRF/distance.py, csrc/hl_mesh_distance.hip; DESIGN.md "Measuring mesh distance").

  workload   the ellipsoid of scripts/mesh_simplify_time.py - `--quads` 708 gives 1 001 112 triangles - against its simplifications on
             cells of 2, 3 and 4 vertex spacings.  The queries of a side are its vertices plus `--samples` surface samples.  Reported
             apart: the sampler, building the index over a mesh (bounds, areas for the default cell, records + count + scans, fill, and
             the host reads between them), and the query of one side against the other's index, in both directions.
  scale      in the same run: the same query kernel on an index whose one cell holds the whole full mesh - every query tests every
             triangle, brute force - on the first 4 096 queries.

Device time between two HIP events around `--reps` back-to-back calls after two warm-up calls, per call; the parent starts `--procs`
fresh child processes one after another and reports the median and the range.  `--stages DIR` adds one more child under
`rocprofv3 --kernel-trace --stats` (a run of its own: one cell size, no scale part) and reports the mean time of every kernel per launch.

    python scripts/mesh_distance_time.py [--procs 3] [--reps 5] [--quads 708] [--samples 500000] [--stages DIR] [--json out.json]
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
BRUTE_QUERIES = 4096
KERNELS = ("k_dist_area", "k_dist_records", "k_dist_fill", "k_dist_query", "k_dist_sample", "k_dist_reduce_finish", "k_dist_reduce", "k_simplify_bounds_finish",
           "k_simplify_bounds", "k_scan_reduce", "k_scan_top", "k_scan_down")


def child(a):
    import torch
    from humanliff_amd.NeRF import distance, simplify
    from mesh_raster_time import per_call_ms
    from mesh_simplify_time import mesh
    dev = torch.device("cuda:0")
    v, tri, n, col, spacing = mesh(a.quads, dev)
    full = {"vertices": v, "triangles": tri}
    out = {"triangles": int(tri.shape[0]), "vertices": int(v.shape[0]), "spacing": spacing, "samples": a.samples}
    out["sample_full_ms"] = per_call_ms(lambda: distance.sample_surface(full, a.samples), a.reps)
    full_queries = torch.cat([v, distance.sample_surface(full, a.samples)["points"]])
    out["index_full_ms"] = per_call_ms(lambda: distance.build_index(full, check=False), a.reps)
    index_full = distance.build_index(full, check=False)
    out["index_full"] = dict(index_full.info, cell=index_full.cell, cell_in_spacings=index_full.cell / spacing)
    for k in SPACINGS if a.only is None else (a.only,):
        res, _, _ = simplify._simplify(v, tri, cell=k * spacing, check=False)
        small = {"vertices": res["vertices"], "triangles": res["triangles"]}
        out[f"simplified_{k}_triangles"] = int(small["triangles"].shape[0])
        out[f"index_simplified_{k}_ms"] = per_call_ms(lambda: distance.build_index(small, check=False), a.reps)
        index_small = distance.build_index(small, check=False)
        out[f"index_simplified_{k}"] = dict(index_small.info, cell=index_small.cell, cell_in_spacings=index_small.cell / spacing)
        small_queries = torch.cat([small["vertices"], distance.sample_surface(small, a.samples)["points"]])
        out[f"queries_{k}"] = [int(full_queries.shape[0]), int(small_queries.shape[0])]
        out[f"query_full_to_simplified_{k}_ms"] = per_call_ms(lambda: index_small.query(full_queries, check=False), a.reps)
        out[f"query_simplified_{k}_to_full_ms"] = per_call_ms(lambda: index_full.query(small_queries, check=False), a.reps)
        out[f"mesh_distance_{k}_ms"] = per_call_ms(lambda: distance.mesh_distance(full, small, samples=a.samples, thresholds=(spacing,), check=False), 2)
        score = distance.mesh_distance(full, small, samples=a.samples, thresholds=(spacing,), check=False)
        out[f"score_{k}_in_cells"] = {"chamfer": score["chamfer"] / (k * spacing), "hausdorff": score["hausdorff"] / (k * spacing),
                                      "full_to_simplified_rms": score["a_to_b"]["rms"] / (k * spacing), "simplified_to_full_rms": score["b_to_a"]["rms"] / (k * spacing)}
        if a.scale and k == SPACINGS[0]:
            one_cell = distance.build_index(full, cell=10.0 * float((index_full.hi - index_full.lo).max()), check=False)
            assert one_cell.extents == (1, 1, 1)
            q = small_queries[:BRUTE_QUERIES].contiguous()
            out["brute_force_queries"] = int(q.shape[0])
            out["brute_force_query_ms"] = per_call_ms(lambda: one_cell.query(q, check=False), 1)
            out["grid_same_queries_ms"] = per_call_ms(lambda: index_full.query(q, check=False), a.reps)
            same = one_cell.query(q, check=False), index_full.query(q, check=False)
            out["brute_force_same_bytes"] = all(bool((same[0][key] == same[1][key]).all()) for key in ("sqdist", "triangle", "barycentric", "point"))
    print("RESULT " + json.dumps(out), flush=True)


def stage_times(a):
    """One child under rocprofv3 --kernel-trace --stats -> {kernel: {launches, mean us per launch, total us}} over the child's whole run."""
    os.makedirs(a.stages, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.stages, "--", sys.executable, os.path.abspath(__file__), "--child",
           "--reps", "2", "--quads", str(a.quads), "--samples", str(a.samples), "--only", str(SPACINGS[0])]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"the profiled process ended with status {r.returncode}:\n{r.stdout[-2000:]}")
    files = glob.glob(os.path.join(a.stages, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.stages}")
    acc = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = next((s for s in KERNELS if s in row["Kernel_Name"]), None)
                if name:
                    acc.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {name: {"launches": len(d), "mean_us": round(sum(d) / len(d) / 1e3, 2), "max_us": round(max(d) / 1e3, 2), "total_us": round(sum(d) / 1e3, 1)}
            for name, d in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quads", type=int, default=708)
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--stages")
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scale", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scale", "--reps", str(a.reps), "--quads", str(a.quads), "--samples",
                            str(a.samples)], stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"a measuring process ended with status {r.returncode}")
        runs.append(json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:]))
        print(f"process {len(runs)} of {a.procs} done", file=sys.stderr, flush=True)
    out = {"procs": a.procs, "reps": a.reps}
    for k in runs[0]:
        if k.endswith("_ms"):
            vals = [r[k] for r in runs]
            out[k] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
        else:
            out[k] = runs[0][k]
    if a.stages:
        out["stage_us"] = stage_times(a)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
