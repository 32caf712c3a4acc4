"""End-to-end example on synthetic weights: layer-conditioned DDIM sampling of several subjects, then orbit renders of every
final tri-plane, sharded over the ranks it is launched with (BASELINE configs[3] / configs[4] at reduced counts).

    python scripts/sample_and_render.py --subjects 2 --layers 2 --ddim 10 --views 4 --res 256
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 scripts/sample_and_render.py --subjects 64 ...

Mirrors scripts/triplane_sample_layered.py of the reference: per subject, layer k is sampled with x_cond = the layer k-1 sample
(:124-134); the finished tri-plane is reshaped to (1,3,9,256,256) (:158) and rendered view by view (:159-199); samples / images are
all-gathered at the end (:211-212).  Rays, near/far and the importance uniforms are made on the device (NeRF.render_view).
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from humanliff_amd import distributed as hd, synthetic as syn
from humanliff_amd.NeRF import Renderer, render_view
from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=2)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--ddim", type=int, default=10)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4, help="subjects sampled together on one GPU")
    ap.add_argument("--float-images", action="store_true", help="gather fp32 images instead of uint8")
    ap.add_argument("--meshes", help="write one PLY mesh per subject and layer here (extract_geometry, mesher='hip'; "
                                     "triplane_sample_layered.py:201-207)")
    ap.add_argument("--mesh-res", type=int, default=512, help="density lattice resolution of the meshes (the reference's 512)")
    ap.add_argument("--mesh-components", default="none", help="which solid components the meshes keep: largest, K (the K largest) or "
                                                              "none (all of them: no filter)")
    ap.add_argument("--mesh-attributes", action="store_true", help="write vertex normals and colours into the PLY files (extract_mesh)")
    ap.add_argument("--mesh-simplify", type=float, default=None, metavar="K",
                    help="cluster the meshes on cells of K >= 1 lattice voxels before writing them (extract_mesh(..., simplify=K))")
    ap.add_argument("--fid-weights", help="a saved state dict of pytorch-fid's InceptionV3 (INTEGRATION.md): with --fid-stats and / or "
                                          "--fid-features, every rendered view goes through a FeatureCollector (InceptionFID, 64 views a "
                                          "call) as it is produced - no PNG round trip")
    ap.add_argument("--fid-stats", metavar="OUT.npz", help="write the mean and covariance of the views' pool3 features here (pytorch-fid's "
                                                           "--save-stats layout; scripts/triplane_fid.py scores two such files)")
    ap.add_argument("--fid-features", metavar="OUT.npy", help="write the views' pool3 features (n, 2048) float32 here (scripts/triplane_fid.py "
                                                              "--kid --prc scores two such files)")
    args = ap.parse_args()
    if bool(args.fid_weights) != bool(args.fid_stats or args.fid_features):
        ap.error("--fid-weights goes together with --fid-stats and / or --fid-features")
    if args.mesh_simplify is not None and not args.mesh_simplify >= 1:
        ap.error("--mesh-simplify: a cell size of at least 1 voxel")
    if args.mesh_components not in ("none", "largest") and not (args.mesh_components.isdigit() and int(args.mesh_components) > 0):
        ap.error("--mesh-components: largest, a positive integer K or none")
    rank, world, dev = hd.init_distributed()
    fid_views = None
    if args.fid_stats or args.fid_features:
        if world != 1:
            ap.error("--fid-stats / --fid-features: the views are taken in order on one device; run it with one rank")
        from humanliff_amd.feature_metrics import FeatureCollector
        from humanliff_amd.fid import FidStatistics, InceptionFID
        fid_views = FeatureCollector(InceptionFID.from_state_dict(torch.load(args.fid_weights, map_location="cpu"), dev), batch=64,
                                     stats=FidStatistics(dev) if args.fid_stats else None, keep=bool(args.fid_features))
    cfg = dict(bench.F4, timestep_respacing=f"ddim{args.ddim}")
    model, diffusion = create_model_and_diffusion(**cfg)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(syn.state_from_shapes(keys, seed=1))
    model = model.to(dev).eval()
    r = Renderer(use_canonical_space=False, triplane_dim=256, triplane_ch=27, smpl_type="smpl", test=True)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(dev)
    shape = (27, 256, 256)

    def sample_fn(x_cond, layer, ids):
        g = torch.Generator().manual_seed(1000 * layer + ids[0])
        noise = torch.randn((len(ids),) + shape, generator=g).to(dev)
        y = torch.full((len(ids),), layer, dtype=torch.int64, device=dev)
        return diffusion.ddim_sample_loop(model, (len(ids),) + shape, x_cond=x_cond, noise=noise, clip_denoised=True,
                                          model_kwargs={"y": y}, device=dev)

    tp = {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}
    H = W = args.res

    def render_fn(sid, sample, v):
        planes = sample.clamp(-1, 1).reshape(1, 3, 9, 256, 256)                   # triplane_sample_layered.py:158
        K, c2w, cam = syn.orbit_camera(v, args.views, H, W)
        R = c2w.T.copy(); T = (-R @ cam).reshape(3, 1)
        rgb = render_view(H, W, K, R, T, planes, tp, r, n_samples=128, n_importance=128)[0]
        if fid_views is not None:                                                 # enqueue-only: nothing is read back per view
            fid_views.add(rgb.detach().float().clamp(0, 1).permute(2, 0, 1).contiguous())
        return rgb

    torch.cuda.synchronize(); t0 = time.perf_counter()
    # sampling, rendering and the gathers (samples: one all-gather; images: per subject, uint8, asynchronous behind the next
    # subject's renders) - humanliff_amd.distributed.sample_and_render, the same code the world-size-2 CPU test drives
    samples, images = hd.sample_and_render(sample_fn, render_fn, args.subjects, args.layers, shape, args.batch, args.views, (H, W, 3), dev,
                                           as_uint8=not args.float_images, images_root=0)   # only rank 0 writes images (:214-219)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    t1 = t0
    if rank == 0:
        steps = args.subjects * args.layers * args.ddim
        rays = args.subjects * args.views * H * W
        print(f"ranks {world}: {args.subjects} subjects x {args.layers} layers x DDIM-{args.ddim} ({steps} denoise steps) + "
              f"{args.subjects * args.views} views {H}x{W} ({rays / 1e6:.1f} Mrays) + gathers in {t2 - t0:.2f} s; "
              f"samples {tuple(samples.shape)} images {tuple(images.shape)} {images.dtype} mean {float(images.float().mean()):.4f}")
        if fid_views is not None:
            fid_views.flush()
            if args.fid_stats:
                fid_views.stats.save(args.fid_stats)
                print(f"{args.fid_stats}: mean and covariance of the pool3 features of {fid_views.stats.count} views")
            if args.fid_features:
                with open(args.fid_features, "wb") as f:
                    np.save(f, fid_views.features().cpu().numpy())
                print(f"{args.fid_features}: pool3 features of {fid_views.count} views")
        if args.meshes:
            from humanliff_amd.NeRF.geometry import write_ply
            os.makedirs(args.meshes, exist_ok=True)
            for sid in range(args.subjects):
                for layer in range(args.layers):
                    planes = samples[sid, layer].to(dev).clamp(-1, 1).reshape(1, 3, 9, 256, 256)
                    path = os.path.join(args.meshes, f"subject{sid:03d}_layer{layer}.ply")
                    if args.mesh_components == "none" and not args.mesh_attributes and args.mesh_simplify is None:
                        v, t = r.extract_geometry(tp, planes, resolution=args.mesh_res, threshold=0, mesher="hip")
                        write_ply(path, v, t)
                        print(f"{path}: {len(v)} vertices, {len(t)} triangles")
                        continue
                    keep = args.mesh_components if args.mesh_components == "largest" else int(args.mesh_components) if args.mesh_components != "none" else None
                    m = r.extract_mesh(tp, planes, resolution=args.mesh_res, threshold=0, components=keep, normals=args.mesh_attributes,
                                       colors=args.mesh_attributes, simplify=args.mesh_simplify)
                    write_ply(path, m["vertices"], m["triangles"], normals=m["normals"], colors=m["colors"])
                    print(f"{path}: {len(m['vertices'])} vertices, {len(m['triangles'])} triangles, {len(m['component_sizes'])} solid "
                          f"components{' (kept: ' + args.mesh_components + ')' if args.mesh_components != 'none' else ''}")
                    if args.mesh_simplify is not None:
                        print(f"{path}: simplified from {len(m['vertex_map'])} marching-cubes vertices (cells of {args.mesh_simplify:g} voxels)")


if __name__ == "__main__":
    main()
