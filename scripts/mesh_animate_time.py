"""What animating an extracted mesh costs, at the workload's own size: a 6 890-vertex body (the synthetic SMPL-like model) and
`--points` mesh vertices (500 000: the order of an extract_mesh at 512^3), K in {1, 4} neighbours, F in {1, 64} frames.

  hip    animate.bind_mesh / MeshBinding.repose (csrc/hl_mesh_animate.hip), normals and bounds included;
  torch  the same formulas as torch ops on the device - what a user would write today: a chunked cdist + topk for the bind, a gather
         and batched 3x3 products per frame for the repose (DESIGN.md "Animating the mesh" has the formulas).

Device time between two HIP events around `--reps` back-to-back calls after two warm-up calls, per call.  The parent starts `--procs`
fresh child processes one after another and each child alternates hip and torch case by case, so a drift of the shared machine falls on
both; the parent reports the median over the processes and their range.  Next to every repose: the bytes it must write (F N 12 per
attribute, vertices and normals) over the time.

    python scripts/mesh_animate_time.py [--procs 3] [--reps 10] [--points 500000] [--json out.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS, FS, V = (1, 4), (1, 64), 6890


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


def torch_bind(x, n, verts, rows, R, Th, K, chunk=32768):
    """bind in torch ops: ids, weights, rest, rest normals."""
    import torch
    q = (x - Th) @ R
    d_parts, i_parts = [], []
    for s in range(0, q.shape[0], chunk):
        d, i = torch.topk(torch.cdist(q[s:s + chunk], verts).square_(), K, dim=1, largest=False)
        d_parts.append(d)
        i_parts.append(i)
    d, ids = torch.cat(d_parts), torch.cat(i_parts)
    w = 1.0 / (d + 1e-8)
    w = w / w.sum(dim=1, keepdim=True)
    M, c = torch_blend(rows, ids, w)
    cof = torch_cofactors(M)
    det = (M[:, 0] * cof[:, 0]).sum(dim=1)
    u = (cof.transpose(1, 2) @ (q - c)[..., None])[..., 0] / det[:, None]
    m = torch.nn.functional.normalize((M.transpose(1, 2) @ (n @ R)[..., None])[..., 0], dim=1)
    return ids, w, u, m


def torch_cofactors(M):
    """The cofactor matrix of every 3x3: its rows are the cross products of the other two rows."""
    import torch
    return torch.stack([torch.linalg.cross(M[:, 1], M[:, 2]), torch.linalg.cross(M[:, 2], M[:, 0]), torch.linalg.cross(M[:, 0], M[:, 1])], dim=1)


def torch_blend(rows, ids, w):
    r = rows[ids]                                                    # (N,K,16)
    Rk, t, po = r[..., :9].reshape(*ids.shape, 3, 3), r[..., 9:12], r[..., 12:15]
    o = (Rk @ po[..., None])[..., 0] + t
    return (w[..., None, None] * Rk).sum(dim=1), (w[..., None] * o).sum(dim=1)


def torch_repose(ids, w, u, m, rows, R, Th):
    """repose in torch ops, frame by frame (a gather of all frames at once is F N K 64 bytes): vertices, normals, bounds."""
    import torch
    verts, nrms = [], []
    for f in range(rows.shape[0]):
        M, c = torch_blend(rows[f], ids, w)
        y = (M @ u[..., None])[..., 0] + c
        verts.append(y @ R.T + Th)
        nrms.append(torch.nn.functional.normalize((torch_cofactors(M) @ m[..., None])[..., 0], dim=1) @ R.T)
    v = torch.stack(verts)
    lo, hi = v.amin(dim=1) - 0.05, v.amax(dim=1) + 0.05
    lo[:, 1] -= 0.05
    hi[:, 1] += 0.05
    return v, torch.stack(nrms), torch.stack([lo, hi], dim=1)


def child(a):
    import numpy as np
    import torch
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import animate
    from humanliff_amd.body import load_body_model
    dev = torch.device("cuda:0")
    model = load_body_model(syn.smpl_like_model(V, 5), dev)
    g = syn._gen(3)
    poses = (torch.randn((max(FS), 72), generator=g) * 0.25).to(dev)
    shapes = (torch.randn((10,), generator=g) * 0.5).to(dev)
    Rw, Th = syn._rodrigues1(torch.tensor([0.2, -0.3, 0.1])).numpy(), np.array([0.1, -0.2, 0.3], dtype=np.float32)
    posed = {F: model.pose(poses[:F], shapes, Rw, Th, forward_rows=True) for F in FS}
    rng = np.random.default_rng(7)
    body = posed[1].vertices[0].cpu().numpy()
    # a surface point per draw, sorted along the body so that neighbouring threads gather neighbouring rows, as lattice order does
    pick = np.sort(rng.integers(0, V, a.points))
    x = torch.from_numpy((body[pick] + rng.normal(0.0, 0.02, (a.points, 3))).astype(np.float32)).to(dev)
    n = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(a.points, 3)).astype(np.float32)).to(dev), dim=1)
    Rd, Td = torch.from_numpy(Rw).to(dev), torch.from_numpy(Th).to(dev)
    out = {}
    for K in KS:
        verts, rows0 = posed[1].verts4[0, :, :3].contiguous(), posed[1].rows[0]
        out[f"bind_K{K}_hip_ms"] = per_call_ms(lambda: animate.bind_mesh(x, posed[1], neighbours=K, normals=n), a.reps)
        out[f"bind_K{K}_torch_ms"] = per_call_ms(lambda: torch_bind(x, n, verts, rows0, Rd, Td, K), max(2, a.reps // 4))
        b = animate.bind_mesh(x, posed[1], neighbours=K, normals=n)
        ids, w = b.ids.long(), b.weights
        for F in FS:
            out[f"repose_K{K}_F{F}_hip_ms"] = per_call_ms(lambda: b.repose(posed[F]), a.reps)
            out[f"repose_K{K}_F{F}_torch_ms"] = per_call_ms(lambda: torch_repose(ids, w, b.rest, b.rest_normals, posed[F].rows, Rd, Td),
                                                            a.reps if F == 1 else max(2, a.reps // 4))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--points", str(a.points)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"a measuring process ended with status {r.returncode}")
        runs.append(json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    out = {"V": V, "points": a.points, "procs": a.procs, "reps": a.reps}
    for k in runs[0]:
        vals = [r[k] for r in runs]
        out[k] = {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
    for K in KS:
        for F in FS:
            ms = out[f"repose_K{K}_F{F}_hip_ms"]["median"]
            out[f"repose_K{K}_F{F}_hip_output_GBps"] = round(F * a.points * 24 / (ms * 1e-3) / 1e9, 1)      # vertices + normals
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
