"""Times Renderer.extract_geometry(resolution=N, mesher="hip") by stage on the synthetic planes, and the numpy restatement of the
same contract on the host (tests/geometry_restatement.py - a restatement, not PyMCubes).  The stages that finish the mesh
(Renderer.extract_mesh: labelling, filter, normals, colours) are timed in the same run, between HIP events.

    python scripts/geometry_time.py [--res 512] [--reps 3] [--json out.json]      # device
    python scripts/geometry_time.py --cpu 128 [--cpu-scipy-edt]                   # host restatement only

The synthetic MLP has sigma < 0 everywhere on the synthetic planes, so its density bias is shifted until 10 % of a 32^3 lattice
is occupied (sigma >= 0) - the same device-side shift tests/test_geometry_gpu.py applies (at 30 %).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OCCUPIED = 0.1
# compulsory bytes per band variable per sweep: k_grad reads nbr (6 x int32) + x, writes g (3 x fp64); k_jacobi reads nbr, g (own),
# x, lower, upper and writes x (neighbour values are gathers of these same arrays)
SWEEP_BYTES = (24 + 8 + 24) + (24 + 24 + 8 + 16 + 8)


def setup(dev, planes_seed=11):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    planes = syn.triplane(seed=planes_seed, H=64, W=64).to(dev)
    mlp = syn.render_mlp_state(3, gain=2.0)
    tp = {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}

    def renderer(m):
        r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
        r.load_state_dict(m, strict=False)
        return r.to(dev)
    u = renderer(mlp).density_grid(tp, planes, resolution=32)
    mlp["alpha_linear.bias"] = mlp["alpha_linear.bias"] + float(torch.quantile(u.flatten().double().cpu(), OCCUPIED))
    return renderer(mlp), tp, planes


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def timed_events(fn):
    """fn's span on the stream, between two HIP events (a host read inside fn, like the labelling's round flag, is inside the span)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def device(res, reps):
    from humanliff_amd.NeRF import geometry
    dev = torch.device("cuda:0")
    r, tp, planes = setup(dev)
    r.extract_geometry(tp, planes, resolution=64, mesher="hip")              # warm-up (library load, allocator)
    rows = []
    for _ in range(reps):
        u, t_field = timed(lambda: r.density_grid(tp, planes, resolution=res))
        (sm, (iters, nb)), t_smooth = timed(lambda: geometry.smooth_constrained(u, return_info=True))
        _, t_prep = timed(lambda: geometry.smooth_constrained(u, max_iters=0))
        (v, t), t_mc = timed(lambda: geometry.marching_cubes(sm, 0.0))
        _, t_all = timed(lambda: r.extract_geometry(tp, planes, resolution=res, mesher="hip"))
        t_sweep = (t_smooth - t_prep) / iters
        # finishing the mesh
        (labels, sizes, rounds), t_label = timed_events(lambda: geometry._label_components(sm, 0.0))
        kept = geometry.select_components(sizes, "largest")
        _, t_filter = timed_events(lambda: geometry.filter_components(sm, 0.0, labels, int(sizes.numel()), kept))
        b = tp["world_bounds"].reshape(-1, 2, 3)[0]
        ext, lo = (b[1] - b[0]).double(), b[0].double()
        nrm, t_normals = timed_events(lambda: geometry.vertex_normals(sm, 0.0, v, ext))
        vw = v / (res - 1.0) * ext[None, :] + lo[None, :]
        _, t_colors = timed_events(lambda: r.vertex_colors(tp, planes, vw, -nrm))
        _, t_mesh = timed(lambda: r.extract_mesh(tp, planes, resolution=res, components="largest"))
        del labels, nrm, vw
        rows.append(dict(res=res, field_ms=round(t_field, 2), smooth_ms=round(t_smooth, 2), smooth_setup_ms=round(t_prep, 2),
                         sweeps=iters, sweep_ms=round(t_sweep, 4), band=nb,
                         sweep_GBps=round(SWEEP_BYTES * nb / (t_sweep * 1e-3) / 1e9, 1),
                         mc_ms=round(t_mc, 2), vertices=int(v.shape[0]), triangles=int(t.shape[0]),
                         smooth_plus_mc_ms=round(t_smooth + t_mc, 2), extract_geometry_ms=round(t_all, 2),
                         label_ms=round(t_label, 2), label_rounds=rounds, components=int(sizes.numel()), filter_ms=round(t_filter, 2),
                         normals_ms=round(t_normals, 2), colors_ms=round(t_colors, 2), extract_mesh_ms=round(t_mesh, 2)))
        del u, sm, v, t
        print(json.dumps(rows[-1]), flush=True)
    return rows


def host(res, scipy_edt):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import geometry_restatement as gr
    from humanliff_amd import synthetic as syn
    from oracle import render_oracle as ro
    planes = syn.triplane(seed=11, H=64, W=64)
    mlp = syn.render_mlp_state(3, gain=2.0)
    bounds = torch.tensor(syn.WORLD_BOUNDS)

    def field(n):
        X, Y, Z = [torch.linspace(float(bounds[0, k]), float(bounds[1, k]), n) for k in range(3)]
        out = np.empty((n, n, n), dtype=np.float32)
        with torch.no_grad():
            for i in range(n):
                yy, zz = torch.meshgrid(Y, Z, indexing="ij")
                pts = torch.stack([torch.full_like(yy, float(X[i])).reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1)
                out[i] = (-ro.mlp(mlp, ro.plane_features(planes[0], pts, bounds))).reshape(n, n).numpy()
        return out
    shift = float(np.quantile(field(32).astype(np.float64), OCCUPIED))
    u = field(res) - np.float32(shift)        # (the bias shift, applied to the field: the host reference point only needs a like surface)
    edt_fn = gr.edt
    if scipy_edt:
        from scipy import ndimage
        edt_fn = ndimage.distance_transform_edt
    t0 = time.perf_counter()
    sm, iters, nb = gr.smooth_constrained(u, edt_fn=edt_fn)
    t1 = time.perf_counter()
    v, t = gr.marching_cubes(sm, 0.0)
    t2 = time.perf_counter()
    row = dict(host_restatement=True, res=res, edt="scipy" if scipy_edt else "restatement", smooth_s=round(t1 - t0, 2),
               mc_s=round(t2 - t1, 2), sweeps=iters, band=nb, triangles=int(len(t)))
    print(json.dumps(row), flush=True)
    return [row]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=0, help="time the host restatement at this resolution instead")
    ap.add_argument("--cpu-scipy-edt", action="store_true", help="host restatement with scipy's EDT (equal to the restatement's, faster)")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = host(a.cpu, a.cpu_scipy_edt) if a.cpu else device(a.res, a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
