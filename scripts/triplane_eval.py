"""Held-out view evaluation of fitted tri-planes: recon_NeRF/run_nerf_batch.py --test -> humanliff_amd evaluate_views.

    python scripts/triplane_eval.py --ckpt logs/fit/001000.tar --humans 0 1 --view_ids 6 7 --image_size 128 --savedir logs/fit/test
    python scripts/triplane_eval.py --ckpt logs/fit/001000.tar --views-npz views.npz

--ckpt is a FitLoop checkpoint (scripts/triplane_fit.py).  No dataset ships with the project: without --views-npz the views are orbit
cameras of humanliff_amd.synthetic (rays, near / far and mask_at_box by SynBodyView_datasets.camera_rays) with a seeded smooth target
image - plumbing, not a quality number.  With --views_num 185 the view ids are the reference's held-out list (heldout_view_ids,
optionally --test_layer_id); any other orbit needs --view_ids.  View id i is orbit position i % views_num of cloth layer i // views_num.

--data synbody --data_root DIR --smpl_model PATH [--image_scaling S --views_num N --poses_num N --pose_interval N --layer_idx L] scores the
same view ids on a SynBody directory tree: the files are decoded, resized on the device (csrc/hl_view_ingest.hip) and held in a ViewStore,
whose test_view gives the rays and the ground truth (recon_NeRF/lib/SynBody_dataset.py).

--data tightcap does the same on a TightCap tree (recon_NeRF/lib/TightCap_dataset.py: the cloth layers are composed on the device from one
photograph and five masks per view) with test_TightCap's held-out views (heldout_view_ids(tightcap=True)); --image_scaling defaults to 1.0 there.

--views-npz loads real views: arrays ray_o_all, ray_d_all (N, R, 3), near_all, far_all (N, R), rgb_all (N, R, 3), mask_at_box_all (N, R),
instance_idx, cloth_layer_index, pose_index, view_id (N), world_bounds (N, 2, 3) and optionally H, W; the N views must be grouped by
instance_idx.

--lpips-weights PATH fills novel_view_lpips: PATH is a state dict of lpips.LPIPS(net='vgg') saved on a machine that has the package
(torch.save(loss_fn_vgg.state_dict(), 'lpips_vgg.pt')); the network runs in HIP (humanliff_amd.lpips.LpipsVGG).  Without
it the entries are NaN: no weights ship with the project.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from humanliff_amd import synthetic as syn                                           # noqa: E402
from humanliff_amd.SynBodyView_datasets import camera_rays                           # noqa: E402
from humanliff_amd.recon_NeRF import Renderer                                        # noqa: E402
from humanliff_amd.recon_NeRF.lib.all_test import heldout_view_ids                   # noqa: E402
from humanliff_amd.recon_NeRF.lib.lpips_views import evaluate_views_lpips           # noqa: E402


def parse():
    a = argparse.ArgumentParser()
    a.add_argument("--ckpt", type=str, required=True)
    a.add_argument("--savedir", type=str, default=None)
    a.add_argument("--humans", type=int, nargs="*", default=None, help="instance indices (default: every instance of the checkpoint)")
    a.add_argument("--views_num", type=int, default=185)
    a.add_argument("--test_layer_id", type=int, default=-1)
    a.add_argument("--view_ids", type=int, nargs="*", default=None)
    a.add_argument("--image_size", type=int, default=256)
    a.add_argument("--n_samples", type=int, default=128)
    a.add_argument("--n_importance", type=int, default=128)
    a.add_argument("--white_bkgd", action="store_true")
    a.add_argument("--data_range", type=float, default=2.0)
    a.add_argument("--views-npz", dest="views_npz", type=str, default=None)
    a.add_argument("--seed", type=int, default=0)
    a.add_argument("--data", choices=["synthetic", "synbody", "tightcap"], default="synthetic")
    a.add_argument("--data_root", type=str, default=None, help="--data synbody / tightcap: a subject's directory; the human list lies beside it")
    a.add_argument("--smpl_model", type=str, default=None, help="--data synbody / tightcap: the SMPL asset (.pkl / .npz) load_body_model reads")
    a.add_argument("--smpl_type", choices=["smpl", "smplx"], default="smpl",
                   help="--data synbody: 'smplx' poses <subject>/smplx.npz with the SMPL-X models of --smplx_dir (the reference's default for SynBody)")
    a.add_argument("--smplx_dir", type=str, default=None, help="--smpl_type smplx: the directory of SMPLX_{MALE,FEMALE,NEUTRAL}.npz")
    a.add_argument("--image_scaling", type=float, default=None, help="default: 0.5 (synbody), 1.0 (tightcap)")
    a.add_argument("--poses_num", type=int, default=1)
    a.add_argument("--pose_start", type=int, default=0)
    a.add_argument("--pose_interval", type=int, default=5)
    a.add_argument("--layer_idx", type=int, default=None)
    a.add_argument("--decode_threads", type=int, default=8)
    a.add_argument("--lpips-weights", dest="lpips_weights", type=str, default=None, help="saved state dict of lpips.LPIPS(net='vgg')")
    return a.parse_args()


def target_image(H, W, seed):
    """A smooth seeded RGB image in [0, 1]."""
    rng = np.random.default_rng(seed)
    ph, fx, fy = rng.random(3) * 2 * math.pi, 2 + rng.random(3) * 4, 2 + rng.random(3) * 4
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    return torch.from_numpy(np.stack([0.5 + 0.5 * np.sin(fx[c] * xx + fy[c] * yy + ph[c]) for c in range(3)], -1)).float()


def synthetic_views(args, humans, dev):
    ids = heldout_view_ids(args.views_num, args.test_layer_id, view_ids=args.view_ids)
    H = W = args.image_size
    for human in humans:
        for view_id in ids:
            K, c2w, cam = syn.orbit_camera(view_id % args.views_num, args.views_num, H, W)
            R = c2w.T                                                        # world -> camera
            ro, rd, near, far, mask = camera_rays(H, W, K, R, -R @ cam, syn.WORLD_BOUNDS, dev, return_mask=True)
            yield {"ray_o_all": ro[None, None], "ray_d_all": rd[None, None], "near_all": near[None, None, :, None],
                   "far_all": far[None, None, :, None], "mask_at_box_all": mask[None, None],
                   "rgb_all": target_image(H, W, args.seed * 1000003 + view_id).reshape(1, 1, H * W, 3),
                   "instance_idx": torch.tensor([human]), "cloth_layer_index": torch.tensor([(view_id // args.views_num) % 4]),
                   "pose_index": torch.tensor([0]), "world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None], "view_id": view_id, "H": H, "W": W}


def synbody_views(args, humans, dev):
    """The held-out views of a SynBody or TightCap tree, read and resized on the device (recon_NeRF/lib/SynBody_dataset.py,
    TightCap_dataset.py) and scored through ViewStore.test_view.  View id i is view i % views_num of cloth layer i // views_num (with
    --layer_idx: of that layer), first pose."""
    from humanliff_amd.body import load_body_model, load_smplx_models
    tightcap = args.data == "tightcap"
    if tightcap:
        from humanliff_amd.recon_NeRF.lib.TightCap_dataset import TightCapIndex as Index, load_view_store, store_test_views
    else:
        from humanliff_amd.recon_NeRF.lib.SynBody_dataset import SynBodyIndex as Index, load_view_store, store_test_views
    smplx = args.smpl_type == "smplx"
    if smplx and (tightcap or not args.data_root or not args.smplx_dir):
        raise SystemExit("--smpl_type smplx is for --data synbody and needs --data_root DIR and --smplx_dir DIR")
    if not smplx and (not args.data_root or not args.smpl_model):
        raise SystemExit(f"--data {args.data} needs --data_root DIR and --smpl_model PATH")
    image_scaling = (1.0 if tightcap else 0.5) if args.image_scaling is None else args.image_scaling
    ids = heldout_view_ids(args.views_num, args.test_layer_id, tightcap=tightcap, view_ids=args.view_ids)
    index = Index(args.data_root, multi_person=True, num_instance=max(humans) + 1, pose_start=args.pose_start,
                         pose_interval=args.pose_interval, poses_num=args.poses_num, views_num=args.views_num, layer_idx=args.layer_idx)
    nv, per_layer = args.views_num, args.poses_num * args.views_num
    per_human = index.cloth_layer_num * per_layer
    layer_of = (lambda i: 0) if args.layer_idx is not None else (lambda i: (i // nv) % 4)
    items = [h * per_human + layer_of(i) * per_layer + i % nv for h in humans for i in ids]
    body = load_smplx_models(args.smplx_dir, dev) if smplx else load_body_model(args.smpl_model, dev)
    store = load_view_store(index, body, image_scaling=image_scaling, device=dev, items=items, decode_threads=args.decode_threads,
                            **({"smpl_type": "smplx"} if smplx else {}))
    return store_test_views(store, view_ids=[i for _ in humans for i in ids])


def npz_views(path):
    z = np.load(path)
    n = z["ray_o_all"].shape[0]
    for i in range(n):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k][i]))        # noqa: E731
        tp = {"ray_o_all": t("ray_o_all")[None, None].float(), "ray_d_all": t("ray_d_all")[None, None].float(),
              "near_all": t("near_all").reshape(1, 1, -1, 1).float(), "far_all": t("far_all").reshape(1, 1, -1, 1).float(),
              "rgb_all": t("rgb_all")[None, None].float(), "mask_at_box_all": t("mask_at_box_all")[None, None] != 0,
              "instance_idx": torch.tensor([int(z["instance_idx"][i])]), "cloth_layer_index": torch.tensor([int(z["cloth_layer_index"][i])]),
              "pose_index": torch.tensor([int(z["pose_index"][i])]), "world_bounds": t("world_bounds")[None].float(),
              "view_id": int(z["view_id"][i])}
        if "H" in z and "W" in z:
            tp["H"], tp["W"] = int(np.asarray(z["H"]).reshape(-1)[0]), int(np.asarray(z["W"]).reshape(-1)[0])
        yield tp


def main():
    args = parse()
    if not torch.cuda.is_available():
        raise SystemExit("triplane_eval.py needs a HIP device: humanliff_amd has no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = torch.load(args.ckpt, map_location="cpu")["network_fn_state_dict"]
    ni, _, _, ch, dim, _ = sd["tri_planes"].shape
    model = Renderer(use_canonical_space=False, num_instances=ni, triplane_dim=dim, triplane_ch=3 * ch, test=True)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)
    torch.manual_seed(args.seed)
    humans = list(range(ni)) if args.humans is None else args.humans
    if args.views_npz:
        views = npz_views(args.views_npz)
    else:
        views = synbody_views(args, humans, dev) if args.data in ("synbody", "tightcap") else synthetic_views(args, humans, dev)
    lpips_fn = None
    if args.lpips_weights:
        from humanliff_amd.lpips import LpipsVGG
        lpips_fn = LpipsVGG.from_state_dict(torch.load(args.lpips_weights, map_location="cpu"), dev)
    # (evaluate_views_lpips is evaluate_views with the hook's device scores read back once per subject; without a hook they are the same)
    metric = evaluate_views_lpips(model, views, lpips_fn, n_samples=args.n_samples, n_importance=args.n_importance, white_bkgd=args.white_bkgd,
                                  data_range=args.data_range, savedir=args.savedir)
    mse, psnr, ssim = metric["novel_view_mean_human"]
    lpips = float(np.mean(metric["novel_view_lpips"]))
    print(f"mean over {metric['novel_view_mse'].size} views of {len(metric['all_human_names'])} subjects: mse {mse:.6f} psnr {psnr:.4f} ssim {ssim:.6f}"
          f" lpips {lpips:.6f}")


if __name__ == "__main__":
    main()
