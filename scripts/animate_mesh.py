"""A mesh per frame of a motion without re-extracting: bind an extracted mesh to the body of the pose it was extracted in and repose
it along a pose sequence on the device (humanliff_amd/NeRF/animate.py, csrc/hl_mesh_animate.hip; DESIGN.md "Animating the mesh").

    python scripts/animate_mesh.py --synthetic --out /tmp/anim [--frames 16]
    python scripts/animate_mesh.py --mesh subject.ply --model assets/SMPL_NEUTRAL.pkl --bind-pose extracted.npz --poses motion.npz --out anim
    python scripts/animate_mesh.py --smpl_type smplx --model assets/models/smplx [--gender female] --mesh subject.ply \\
        --bind-pose subject/smplx.npz --poses motion/smplx.npz --out anim

--mesh: a PLY written by geometry.write_ply (vertices, triangles, optionally normals and colours).  --bind-pose: the pose the mesh was
extracted in (its first frame is taken), --poses: the sequence; both in the format of scripts/render_pose_sequence.py - an .npz with
`poses` (F,72), `shapes` and optionally `R`, `Th`, or for --smpl_type smplx a SynBody smplx.npz.  Writes <out>/frame_0000.ply, ...: the
reposed vertices and normals, the triangles and the colours unchanged (they belong to the surface, not to the pose), `--chunk` frames
per repose call so that the F x N output stays bounded.  --synthetic takes the seeded stand-ins of humanliff_amd.synthetic: the body
model, a swinging-limbs sequence and, for the mesh, the body's own vertices pushed 1 cm off their centroid (no triangles).
One JSON line of timings at the end.

--images DIR also rasterises every frame (humanliff_amd/NeRF/raster.py; DESIGN.md "Rasterising the mesh") and writes
DIR/frame_0000.png, ...: headlight-shaded colours on white.  The camera is --camera cam.npz (`K`, `R`, `T` - one camera or one per frame
- and `H`, `W`) or --turntable N: N cameras of --res pixels on a circle around the first frame's bounds, frame f seen from camera f mod N.
--simplify CELL first clusters the mesh on a grid of CELL world units (humanliff_amd/NeRF/simplify.py; DESIGN.md "Simplifying the
mesh"): the binding, every reposed frame and every PLY then carry the smaller mesh.  --simplify-report [SAMPLES] adds to the JSON line how
far the smaller mesh is from the full one, in cells: mesh_distance over the vertices and SAMPLES (default 100 000) surface samples per side
(humanliff_amd/NeRF/distance.py; DESIGN.md "Measuring mesh distance").
The mesh needs triangles; with --synthetic and --images the stand-in is an ellipsoid of the body's proportions around the body's centroid
(triangulated, with normals and colours) instead of the offset vertices.  The JSON line then carries the raster timings too.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def pose_file(model, path, smplx, frames=None):
    """A pose file of render_pose_sequence.py's formats -> PosedBody with forward rows."""
    if smplx:
        with np.load(path, allow_pickle=True) as z:
            fitted = z["smplx"].item()
        fitted = {k: np.asarray(v, dtype=np.float32) if k == "betas" else np.asarray(v, dtype=np.float32)[:frames] for k, v in fitted.items()}
        return model.pose_dict({k: torch.from_numpy(v) for k, v in fitted.items()}, forward_rows=True)
    z = np.load(path)
    poses, shapes = z["poses"].astype(np.float32).reshape(-1, 72)[:frames], z["shapes"].astype(np.float32)
    if shapes.ndim == 2 and shapes.shape[0] > 1:
        shapes = shapes[:frames]
    dev = model.device
    take = lambda k, n: (np.asarray(z[k])[:frames] if np.asarray(z[k]).ndim == n else z[k]) if k in z.files else None  # noqa: E731
    return model.pose(torch.from_numpy(poses).to(dev), torch.from_numpy(shapes).to(dev), take("R", 3), take("Th", 2), forward_rows=True)


def ellipsoid_mesh(centre, radii, q=48):
    """A closed latitude / longitude mesh: vertices (q (q - 1) + 2, 3) float64, triangles, unit normals, uint8 colours from the normals."""
    lat, lon = np.pi * np.arange(1, q) / q, 2 * np.pi * np.arange(q) / q
    u = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.ones(q)[None], np.sin(lat)[:, None] * np.sin(lon)[None]], axis=-1)
    u = np.concatenate([u.reshape(-1, 3), [[0, 1, 0], [0, -1, 0]]])
    ring = np.arange(q)
    a = (np.arange(q - 2)[:, None] * q + ring[None]).reshape(-1)
    b = (np.arange(q - 2)[:, None] * q + (ring[None] + 1) % q).reshape(-1)
    north, south, last = (q - 1) * q, (q - 1) * q + 1, (q - 2) * q
    tri = np.concatenate([np.stack([a, b, b + q], 1), np.stack([a, b + q, a + q], 1),
                          np.stack([np.full(q, north), (ring + 1) % q, ring], 1), np.stack([np.full(q, south), last + ring, last + (ring + 1) % q], 1)])
    n = u / radii
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return {"vertices": centre + u * radii, "triangles": tri.astype(np.int64), "normals": n, "colors": np.clip(127 + 120 * n, 0, 255).astype(np.uint8)}


def turntable(lo, hi, n, res):
    """n cameras (K, R, T stacks) on a horizontal circle around the box lo .. hi, looking at its centre, the box filling most of the view."""
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    Ks, Rs, Ts = [], [], []
    for k in range(n):
        az = 2 * np.pi * k / n
        cam = centre + 1.6 * size * np.array([np.sin(az), 0.0, np.cos(az)])
        fwd = (centre - cam) / np.linalg.norm(centre - cam)
        right = np.cross(fwd, [0.0, -1.0, 0.0])             # image y grows downwards, as in synthetic.orbit_camera
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])    # world -> camera
        f = 1.3 * res
        Ks.append(np.array([[f, 0, res / 2.0], [0, f, res / 2.0], [0, 0, 1.0]])), Rs.append(R), Ts.append(-R @ cam)
    return np.stack(Ks), np.stack(Rs), np.stack(Ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh")
    ap.add_argument("--model")
    ap.add_argument("--smpl_type", choices=["smpl", "smplx"], default="smpl")
    ap.add_argument("--gender", default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--bind-pose")
    ap.add_argument("--poses")
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--neighbours", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--images")
    ap.add_argument("--camera")
    ap.add_argument("--turntable", type=int, default=0)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL")
    ap.add_argument("--simplify-report", type=int, nargs="?", const=100000, default=0, metavar="SAMPLES")
    a = ap.parse_args()
    if a.simplify_report and a.simplify is None:
        ap.error("--simplify-report needs --simplify CELL")
    if a.simplify is not None and not a.simplify > 0:
        ap.error("--simplify CELL: a positive cell size in world units")
    if a.images and bool(a.camera) == bool(a.turntable > 0):
        ap.error("--images needs exactly one of --camera cam.npz and --turntable N")
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import animate, geometry
    from humanliff_amd.body import load_body_model, load_smplx_model
    if not a.synthetic and not (a.mesh and a.model and a.bind_pose and a.poses):
        ap.error("give --mesh, --model, --bind-pose and --poses, or --synthetic for seeded stand-ins")
    dev = torch.device("cuda:0")
    smplx = a.smpl_type == "smplx"
    if a.synthetic:
        from render_pose_sequence import synthetic_sequence
        F = a.frames or 16
        seq = synthetic_sequence(F)
        if smplx:
            model = load_smplx_model(a.model if a.model else syn.smplx_like_model(10475, 23), dev, gender=a.gender or "neutral")
            z = lambda n: np.zeros((F, n), dtype=np.float32)  # noqa: E731
            posed = model.pose_dict({"global_orient": z(3), "body_pose": seq[:, 3:66], "betas": np.zeros((1, 10), dtype=np.float32), "expression": z(10)},
                                    forward_rows=True)
        else:
            model = load_body_model(a.model if a.model else syn.smpl_like_model(6890, 5), dev)
            posed = model.pose(torch.from_numpy(seq).to(dev), torch.zeros(10, device=dev), forward_rows=True)
        bind_posed = posed
        body = posed.vertices[0].cpu().numpy().astype(np.float64)
        off = body - body.mean(axis=0)
        nrm = off / np.linalg.norm(off, axis=1, keepdims=True)
        mesh = {"vertices": body + 0.01 * nrm, "triangles": np.zeros((0, 3), dtype=np.int64), "normals": nrm, "colors": None}
        if a.images:        # (an image needs triangles, which the seeded body does not have)
            mesh = ellipsoid_mesh(body.mean(axis=0), (body.max(axis=0) - body.min(axis=0)) / 2)
    else:
        if smplx and a.gender is None:
            with np.load(a.bind_pose, allow_pickle=True) as z:
                a.gender = z["meta"].item()["gender"]
        model = load_smplx_model(a.model, dev, gender=a.gender or "neutral") if smplx else load_body_model(a.model, dev)
        bind_posed = pose_file(model, a.bind_pose, smplx, 1)
        posed = pose_file(model, a.poses, smplx, a.frames)
        parts = geometry.read_ply(a.mesh)
        mesh = {"vertices": parts[0], "triangles": parts[1], "normals": None, "colors": None}
        for extra in parts[2:]:
            mesh["colors" if extra.dtype == np.uint8 else "normals"] = extra
    os.makedirs(a.out, exist_ok=True)
    simplified = None
    if a.simplify is not None:
        if len(mesh["triangles"]) == 0:
            ap.error("--simplify needs a mesh with triangles (with --synthetic: add --images for the ellipsoid stand-in)")
        from humanliff_amd.NeRF.simplify import simplify_mesh
        before = (len(mesh["vertices"]), len(mesh["triangles"]))
        full, mesh = mesh, simplify_mesh(mesh, cell=a.simplify)
        simplified = {"cell": a.simplify, "vertices": [before[0], len(mesh["vertices"])], "triangles": [before[1], len(mesh["triangles"])]}
        if a.simplify_report:
            if len(mesh["triangles"]) == 0:
                ap.error("--simplify-report: the simplified mesh has no triangles (the mesh lies inside one cell)")
            from humanliff_amd.NeRF.distance import mesh_distance
            score = mesh_distance(full, mesh, samples=a.simplify_report, thresholds=(0.25 * a.simplify, 0.5 * a.simplify))
            in_cells = lambda s: {k: round(s[k] / a.simplify, 5) for k in ("mean", "rms", "max")}  # noqa: E731
            simplified["distance_in_cells"] = {"samples": a.simplify_report, "full_to_simplified": in_cells(score["a_to_b"]),
                                               "simplified_to_full": in_cells(score["b_to_a"]), "chamfer": round(score["chamfer"] / a.simplify, 5),
                                               "hausdorff": round(score["hausdorff"] / a.simplify, 5), "fscore_at_quarter_and_half_cell": score["fscore"]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    binding = animate.bind_mesh(mesh["vertices"], bind_posed, frame=0, neighbours=a.neighbours, normals=mesh["normals"])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    t_repose = t_raster = 0.0
    chunk = max(1, a.chunk)
    if a.images:
        from humanliff_amd.NeRF import raster
        from PIL import Image
        if len(mesh["triangles"]) == 0:
            raise SystemExit("--images: the mesh has no triangles")
        os.makedirs(a.images, exist_ok=True)
        if a.camera:
            with np.load(a.camera) as z:
                Ks, Rs, Ts = (np.asarray(z[k], dtype=np.float64) for k in ("K", "R", "T"))
                Hi, Wi = int(z["H"]), int(z["W"])
            Ks, Rs, Ts = Ks.reshape(-1, 3, 3), Rs.reshape(-1, 3, 3), Ts.reshape(-1, 3)
            for name, x in (("K", Ks), ("R", Rs), ("T", Ts)):
                if x.shape[0] not in (1, posed.F):
                    raise SystemExit(f"--camera: `{name}` holds {x.shape[0]} cameras; give one, or one per frame ({posed.F} frames)")
        else:
            v0 = np.asarray(mesh["vertices"], dtype=np.float64)
            Ks, Rs, Ts = turntable(v0.min(axis=0), v0.max(axis=0), a.turntable, a.res)
            Hi = Wi = a.res

        def per_frame(x, f0, n):
            """The cameras of frames f0 .. f0 + n - 1: the one shared camera, or camera f mod C (a turntable goes round; --camera has C = F)."""
            if x.shape[0] == 1:
                return x[0]
            return x[[f % x.shape[0] for f in range(f0, f0 + n)]]
        tri32 = raster.device_triangles(mesh["triangles"], dev)      # converted once for all chunks
    for f0 in range(0, posed.F, chunk):
        ta = time.perf_counter()
        out = binding.repose(posed, frames=slice(f0, f0 + chunk), bounds=False)
        verts = out["vertices"].cpu().numpy()                       # (the synchronise)
        nrms = None if out["normals"] is None else out["normals"].cpu().numpy()
        t_repose += time.perf_counter() - ta
        if a.images:
            n = verts.shape[0]
            tb = time.perf_counter()
            img = raster.rasterize(out["vertices"], tri32, Hi, Wi, per_frame(Ks, f0, n), per_frame(Rs, f0, n), per_frame(Ts, f0, n),
                                   normals=out["normals"], colors=mesh["colors"], shade="headlight", white_bkgd=True)
            rgb8 = (img["rgb_map"].clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy()       # (the synchronise)
            t_raster += time.perf_counter() - tb
            for k in range(n):
                Image.fromarray(rgb8[k]).save(os.path.join(a.images, f"frame_{f0 + k:04d}.png"))
        for k in range(verts.shape[0]):
            geometry.write_ply(os.path.join(a.out, f"frame_{f0 + k:04d}.ply"), verts[k], mesh["triangles"], None if nrms is None else nrms[k],
                               mesh["colors"])
    line = {"frames": posed.F, "mesh_vertices": binding.N, "neighbours": binding.K, "bind_ms": round((t1 - t0) * 1e3, 3),
            "repose_and_read_back_ms_per_frame": round(t_repose * 1e3 / posed.F, 3), "out": a.out}
    if a.images:
        line.update(images=a.images, image_size=[Hi, Wi], triangles=int(len(mesh["triangles"])),
                    raster_and_read_back_ms_per_frame=round(t_raster * 1e3 / posed.F, 3))
    if simplified:
        line.update(simplify=simplified)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
