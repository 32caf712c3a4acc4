"""The distance between two meshes on disk (humanliff_amd/NeRF/distance.py, csrc/hl_mesh_distance.hip; DESIGN.md "Measuring mesh
distance"): Chamfer and Hausdorff distance, precision / recall / F-score at thresholds and normal consistency, each from the exact
closest point on the other mesh's triangles.  The queries of a side are its vertices plus --samples area-weighted surface samples.

    python scripts/mesh_distance.py A.ply B.ply [--samples 100000] [--seed 0] [--thresholds 0.005 0.01] [--cell H] [--json out.json]

The files are PLYs as geometry.write_ply writes them.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(path):
    import numpy as np
    from humanliff_amd.NeRF.geometry import read_ply
    parts = read_ply(path)
    mesh = {"vertices": parts[0], "triangles": parts[1]}
    for extra in parts[2:]:
        if extra.dtype != np.uint8:
            mesh["normals"] = extra
    if len(mesh["triangles"]) == 0:
        raise SystemExit(f"{path}: a mesh without triangles has no surface to measure against")
    return mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[])
    ap.add_argument("--cell", type=float, default=None)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd.NeRF.distance import mesh_distance
    ma, mb = load(a.a), load(a.b)
    out = mesh_distance(ma, mb, samples=a.samples, seed=a.seed, thresholds=a.thresholds, cell=a.cell)
    for side in ("a_to_b", "b_to_a"):
        out[side].pop("sums")
    out.update(a=a.a, b=a.b, samples=a.samples, seed=a.seed, triangles=[len(ma["triangles"]), len(mb["triangles"])])
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
