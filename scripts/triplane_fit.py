"""Tri-plane fitting on synthetic rays: recon_NeRF/run_nerf_batch.py's (and run_nerf_batch_ft.py's) flags -> humanliff_amd FitLoop.

    python scripts/triplane_fit.py --expname fit --num_instance 100 --batch_size 2 --n_rand 2048 --n_samples 128 --n_importance 128 \
        --triplane_ch 27 --lrate_decay 10 --tri_plane_lrate 1e-1 --tv_loss --tv_loss_coef 1e-2 --l1_loss_coef 5e-4 --use_clamp --n_iteration 1000
    python scripts/triplane_fit.py --expname ft --ft_triplane_only --lrate 0 --batch_size 8 --num_instance 1 ...

No dataset ships with the project.  --data synthetic (default): the batches are humanliff_amd.synthetic.fit_batch (orbit rays, random
targets), a fresh one per step.  --data rendered: --views orbit views of a seeded tri-plane inside a box of 0.6 x the world bounds are rendered (render_view),
acc > 0.5 is their body mask, all but --heldout of them go into a device-resident ViewStore and a FRESH tri-plane is fitted to them through
RayBatchLoader (rays sampled on the device, csrc/hl_ray_batch.hip); evaluate_views' PSNR on the held-out views is printed before and after.
--data synbody: the views of a SynBody directory tree (--data_root DIR, the first subject's directory, with human_list.txt beside it;
--smpl_model PATH, the body model asset) are decoded, resized by --image_scaling on the device (csrc/hl_view_ingest.hip) and held in a
ViewStore (recon_NeRF/lib/SynBody_dataset.py); --num_instance subjects x 4 cloth layers (or --layer_idx) x --poses_num x --views_num views.
With --ft_triplane_only it is run_nerf_batch_ft.py's flow (:348-360, 110-129): for every subject of human_list.txt[--start_idx:--end_idx] and
every cloth layer, a one-subject tri-plane is fitted with the decoder of the run's checkpoint frozen - layer 0 starts from the checkpoint's
first tri-plane, layer l from layer l - 1 of the subject's own file - and saved as {subject}_{n_iteration:06d}.tar.  (The learning rate
follows FitLoop's schedule; the reference's separate 0.5 ^ (step / 500) decay of that script is not restated.)
--data tightcap: the same for a TightCap tree (TightCap_human_list.txt beside the subjects; one photograph and five masks per view): every
view's cloth layers are composed on the device (hl_view_ingest_layers; recon_NeRF/lib/TightCap_dataset.py).  --image_scaling and
--views_num default to the reference's configs: 0.5 and 185 for synbody, 1.0 and 382 for tightcap.
--tv_loss is accepted and ignored: FitLoop always computes both regularisers (a coefficient of 0 switches a term off).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from humanliff_amd import synthetic as syn          # noqa: E402
from humanliff_amd.recon_NeRF import Renderer        # noqa: E402
from humanliff_amd.recon_NeRF.fit import FitLoop     # noqa: E402


def parse():
    a = argparse.ArgumentParser()
    a.add_argument("--expname", type=str, default="fit")
    a.add_argument("--basedir", type=str, default="./logs/")
    a.add_argument("--n_iteration", type=int, default=50000)
    a.add_argument("--lrate", type=float, default=5e-4)
    a.add_argument("--tri_plane_lrate", type=float, default=1e-3)
    a.add_argument("--lrate_decay", type=int, default=250)
    a.add_argument("--no_reload", action="store_true")
    a.add_argument("--ft_path", type=str, default=None)
    a.add_argument("--use_clamp", action="store_true")
    a.add_argument("--tv_loss", action="store_true")
    a.add_argument("--tv_loss_coef", type=float, default=5e-4)
    a.add_argument("--l1_loss_coef", type=float, default=2e-4)
    a.add_argument("--ft_triplane_only", action="store_true")
    a.add_argument("--triplane_dim", type=int, default=256)
    a.add_argument("--triplane_ch", type=int, default=27)
    a.add_argument("--n_samples", type=int, default=64)
    a.add_argument("--n_importance", type=int, default=64)
    a.add_argument("--n_rand", type=int, default=2048)
    a.add_argument("--chunk", type=int, default=1024 * 64)
    a.add_argument("--perturb", type=float, default=1.)
    a.add_argument("--batch_size", type=int, default=1)
    a.add_argument("--num_instance", type=int, default=100)
    a.add_argument("--i_print", type=int, default=100)
    a.add_argument("--i_weights", type=int, default=10000)
    a.add_argument("--seed", type=int, default=0)
    a.add_argument("--data", choices=["synthetic", "rendered", "synbody", "tightcap"], default="synthetic")
    a.add_argument("--data_root", type=str, default=None, help="--data synbody / tightcap: a subject's directory; the human list lies beside it")
    a.add_argument("--smpl_model", type=str, default=None, help="--data synbody / tightcap: the SMPL asset (.pkl / .npz) load_body_model reads")
    a.add_argument("--smpl_type", choices=["smpl", "smplx"], default="smpl",
                   help="--data synbody: 'smplx' poses <subject>/smplx.npz with the SMPL-X models of --smplx_dir (the reference's default for SynBody)")
    a.add_argument("--smplx_dir", type=str, default=None, help="--smpl_type smplx: the directory of SMPLX_{MALE,FEMALE,NEUTRAL}.npz")
    a.add_argument("--image_scaling", type=float, default=None, help="default: 0.5 (synbody), 1.0 (tightcap)")
    a.add_argument("--views_num", type=int, default=None, help="default: 185 (synbody), 382 (tightcap)")
    a.add_argument("--poses_num", type=int, default=1)
    a.add_argument("--pose_start", type=int, default=0)
    a.add_argument("--pose_interval", type=int, default=5)
    a.add_argument("--layer_idx", type=int, default=None)
    a.add_argument("--single_person", action="store_true", help="--data synbody / tightcap: only --data_root itself (multi_person=False)")
    a.add_argument("--start_idx", type=int, default=0, help="--ft_triplane_only: first subject of human_list.txt")
    a.add_argument("--end_idx", type=int, default=None)
    a.add_argument("--decode_threads", type=int, default=8)
    a.add_argument("--views", type=int, default=24, help="--data rendered: orbit views rendered from the hidden tri-plane")
    a.add_argument("--heldout", type=int, default=4, help="--data rendered: of which this many (evenly spaced) are only scored")
    a.add_argument("--image_size", type=int, default=128, help="--data rendered: side of the rendered views")
    args = a.parse_args()
    tightcap = args.data == "tightcap"
    args.image_scaling = (1.0 if tightcap else 0.5) if args.image_scaling is None else args.image_scaling
    args.views_num = (382 if tightcap else 185) if args.views_num is None else args.views_num
    return args


def batches(args, dev):
    step = 0
    while True:
        tp = syn.fit_batch(args.batch_size, args.n_rand, args.num_instance, seed=args.seed * 1000003 + step)
        yield {k: v.to(dev, non_blocking=True) for k, v in tp.items()}
        step += 1


def rendered_views(args, dev):
    """Render the views of a hidden tri-plane and split them: (ViewStore of the training views, store of the held-out ones)."""
    from humanliff_amd.NeRF import Renderer as ViewRenderer
    from humanliff_amd.NeRF.renderer import render_view
    from humanliff_amd.SynBodyView_datasets import camera_rays
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import ViewStore
    S = args.image_size
    hidden = ViewRenderer(use_canonical_space=False, triplane_dim=args.triplane_dim, triplane_ch=args.triplane_ch, smpl_type='smpl', test=True)
    hidden.load_state_dict(syn.render_mlp_state(3), strict=False)
    hidden = hidden.to(dev)
    planes = syn.triplane(seed=11 + args.seed, H=args.triplane_dim, W=args.triplane_dim).to(dev)
    # the hidden subject fills a box of 0.6 x the world bounds (a seeded tri-plane is opaque everywhere inside its box): the rest of
    # the world box is the empty space the background class is drawn from
    inner = (0.6 * torch.tensor(syn.WORLD_BOUNDS)).tolist()
    tp = {"world_bounds": torch.tensor(inner, device=dev)[None]}
    held = set(range(0, args.views, max(args.views // max(args.heldout, 1), 1))[:args.heldout])
    train, test = ViewStore(S, S, dev), ViewStore(S, S, dev)
    with torch.no_grad():
        for v in range(args.views):
            K, c2w, cam = syn.orbit_camera(v, args.views, S, S)
            R = c2w.T.copy()
            rgb, acc, _, _ = render_view(S, S, K, R, -R @ cam, planes, tp, hidden, n_samples=args.n_samples, n_importance=args.n_importance)
            hit = camera_rays(S, S, K, R, -R @ cam, inner, dev)[4].reshape(S, S)          # rays that cross the subject's box
            (test if v in held else train).add((rgb * hit[..., None])[None].contiguous(), ((acc > 0.5) & hit)[None], K[None], R[None],
                                               (-R @ cam)[None], syn.WORLD_BOUNDS, 0, 0)
    return train.prepare(), test.prepare()


def heldout_tp(store):
    """The held-out views as evaluate_views' tp_input dicts (ViewStore.test_view: the reference's split != 'train' tuple)."""
    for v in range(len(store)):
        rgb, ray_o, ray_d, near, far, _, mask_at_box, _ = store.test_view(v)
        yield {"rgb_all": rgb[None, None], "ray_o_all": ray_o[None, None], "ray_d_all": ray_d[None, None], "near_all": near[None, None, :, None],
               "far_all": far[None, None, :, None], "mask_at_box_all": mask_at_box[None, None], "instance_idx": store.instance_idx[v:v + 1],
               "cloth_layer_index": store.cloth_layer_index[v:v + 1], "pose_index": torch.tensor([0]), "world_bounds": store.world_bounds[v:v + 1],
               "view_id": v, "H": store.H, "W": store.W}


def fit_rendered(args, model, dev, kw):
    from humanliff_amd.recon_NeRF.lib.all_test import evaluate_views
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader
    train, test = rendered_views(args, dev)
    print(f"rendered {len(train)} training and {len(test)} held-out views of {args.image_size} x {args.image_size}; "
          f"class counts (body, background) of the first: {train.class_counts()[0].tolist()}", flush=True)

    def score(tag):
        model.test = True
        m = evaluate_views(model, heldout_tp(test), n_samples=args.n_samples, n_importance=args.n_importance, human_names=["hidden"])
        model.test = False
        print(f"[{tag}] held-out views: mse {m['novel_view_mean_human'][0]:.6f} psnr {m['novel_view_mean_human'][1]:.3f} "
              f"ssim {m['novel_view_mean_human'][2]:.4f}", flush=True)

    score("before")
    FitLoop(model, RayBatchLoader(train, args.batch_size, args.n_rand, seed=args.seed), **kw).run_loop()
    score("after")


def dataset_reader(args):
    """(index class, load_view_store, name of the human list) of --data synbody / tightcap: the only things the two paths differ in."""
    if args.data == "tightcap":
        from humanliff_amd.recon_NeRF.lib.TightCap_dataset import TightCapIndex, load_view_store
        return TightCapIndex, load_view_store, 'TightCap_human_list.txt'
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import SynBodyIndex, load_view_store
    return SynBodyIndex, load_view_store, 'human_list.txt'


def synbody_store(args, dev, body, data_root, multi_person, num_instance, layer_idx):
    Index, load_view_store, _ = dataset_reader(args)
    index = Index(data_root, multi_person=multi_person, num_instance=num_instance, pose_start=args.pose_start,
                         pose_interval=args.pose_interval, poses_num=args.poses_num, views_num=args.views_num, layer_idx=layer_idx)
    kw = {"smpl_type": "smplx"} if args.smpl_type == "smplx" else {}
    store = load_view_store(index, body, image_scaling=args.image_scaling, device=dev, decode_threads=args.decode_threads, **kw)
    print(f"loaded {len(store)} views of {store.H} x {store.W} from {data_root}"
          f"{'' if layer_idx is None else f' (cloth layer {layer_idx})'}; class counts (body, background) of the first: "
          f"{store.class_counts()[0].tolist()}", flush=True)
    return store


def new_model(args, dev, num_instances):
    model = Renderer(use_canonical_space=False, num_instances=num_instances, triplane_dim=args.triplane_dim, triplane_ch=args.triplane_ch, test=False)
    model.load_state_dict(syn.render_mlp_state(3), strict=False)
    return model.to(dev)


def finetune_synbody(args, dev, body, kw):
    """run_nerf_batch_ft.py:348-360 with create_nerf's tri-plane hand-over (:110-120)."""
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader
    logdir = os.path.join(args.basedir, args.expname)
    if args.ft_path not in (None, 'None'):
        base_ckpt = os.path.join(logdir, args.ft_path)
    else:
        runs = sorted(f for f in os.listdir(logdir) if f.endswith('.tar') and f[:-4].isdigit()) if os.path.isdir(logdir) else []
        if not runs:
            raise SystemExit(f"--ft_triplane_only needs the fitted decoder: no NNNNNN.tar checkpoint in {logdir} (fit without the flag first, or name one with --ft_path)")
        base_ckpt = os.path.join(logdir, runs[-1])
    root_dir = os.path.dirname(args.data_root)
    with open(os.path.join(root_dir, dataset_reader(args)[2])) as f:
        names = [n.strip() for n in f.readlines()][args.start_idx:args.end_idx]
    kw = dict(kw, ft_triplane_only=True, expname=None)                       # (the hand-over below replaces FitLoop's own reload)
    for name in names:
        own = os.path.join(logdir, f'{name}_{args.n_iteration:06d}.tar')
        for layer in (range(4) if args.layer_idx is None else [args.layer_idx]):
            state = torch.load(base_ckpt, map_location='cpu')['network_fn_state_dict']
            if layer == 0 or not os.path.exists(own):
                state['tri_planes'] = state['tri_planes'][0:1].clone()
            else:
                planes = torch.load(own, map_location='cpu')['network_fn_state_dict']['tri_planes']
                planes[:, layer] = planes[:, layer - 1]
                state['tri_planes'] = planes
            model = new_model(args, dev, 1)
            model.load_state_dict(state, strict=False)
            store = synbody_store(args, dev, body, os.path.join(root_dir, name), False, 1, layer)
            loop = FitLoop(model, RayBatchLoader(store, min(args.batch_size, len(store)), args.n_rand, seed=args.seed), **kw)
            while loop.global_step < args.n_iteration:
                for tp in loop.data:
                    losses = loop.step(tp)
                    if loop.global_step % args.i_print == 0 or loop.global_step == args.n_iteration:
                        print(f"[FT] {name} layer {layer} iter {loop.global_step} loss {float(losses[0]):.5f} img loss {float(losses[1]):.5f}", flush=True)
                    if loop.global_step >= args.n_iteration:
                        break
            os.makedirs(logdir, exist_ok=True)
            torch.save({'network_fn_state_dict': {'tri_planes': model.tri_planes.detach().cpu().clone()}}, own)
            print('Saved checkpoints at', own, flush=True)


def fit_synbody(args, model, dev, kw):
    from humanliff_amd.body import load_body_model, load_smplx_models
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader
    if args.smpl_type == "smplx":
        if args.data != "synbody" or not args.data_root or not args.smplx_dir:
            raise SystemExit("--smpl_type smplx is for --data synbody and needs --data_root DIR and --smplx_dir DIR")
        body = load_smplx_models(args.smplx_dir, dev)
    else:
        if not args.data_root or not args.smpl_model:
            raise SystemExit(f"--data {args.data} needs --data_root DIR and --smpl_model PATH")
        body = load_body_model(args.smpl_model, dev)
    if args.ft_triplane_only:
        return finetune_synbody(args, dev, body, kw)
    store = synbody_store(args, dev, body, args.data_root, not args.single_person, 1 if args.single_person else args.num_instance, args.layer_idx)
    FitLoop(model, RayBatchLoader(store, args.batch_size, args.n_rand, seed=args.seed), **kw).run_loop()


def main():
    args = parse()
    if not torch.cuda.is_available():
        raise SystemExit("triplane_fit.py needs a HIP device: humanliff_amd has no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    model = Renderer(use_canonical_space=False, num_instances=args.num_instance, triplane_dim=args.triplane_dim,
                     triplane_ch=args.triplane_ch, test=False)
    model.load_state_dict(syn.render_mlp_state(3), strict=False)
    model = model.to(dev)
    kw = dict(lrate=args.lrate, tri_plane_lrate=args.tri_plane_lrate, lrate_decay=args.lrate_decay,
              tv_loss_coef=args.tv_loss_coef, l1_loss_coef=args.l1_loss_coef, use_clamp=args.use_clamp, n_samples=args.n_samples,
              n_importance=args.n_importance, perturb=args.perturb, chunk=args.chunk, ft_triplane_only=args.ft_triplane_only,
              n_iteration=args.n_iteration, i_print=args.i_print, i_weights=args.i_weights, basedir=args.basedir, expname=args.expname,
              ft_path=args.ft_path, no_reload=args.no_reload)
    if args.data == "rendered":
        return fit_rendered(args, model, dev, kw)
    if args.data in ("synbody", "tightcap"):
        return fit_synbody(args, model, dev, kw)
    FitLoop(model, batches(args, dev), **kw).run_loop()


if __name__ == "__main__":
    main()
