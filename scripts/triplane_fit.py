"""Tri-plane fitting on synthetic rays: recon_NeRF/run_nerf_batch.py's (and run_nerf_batch_ft.py's) flags -> humanliff_amd FitLoop.

    python scripts/triplane_fit.py --expname fit --num_instance 100 --batch_size 2 --n_rand 2048 --n_samples 128 --n_importance 128 \
        --triplane_ch 27 --lrate_decay 10 --tri_plane_lrate 1e-1 --tv_loss --tv_loss_coef 1e-2 --l1_loss_coef 5e-4 --use_clamp --n_iteration 1000
    python scripts/triplane_fit.py --expname ft --ft_triplane_only --lrate 0 --batch_size 8 --num_instance 1 ...

No dataset ships with the project: the batches are humanliff_amd.synthetic.fit_batch (orbit rays, random targets), a fresh one per step.
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
    return a.parse_args()


def batches(args, dev):
    step = 0
    while True:
        tp = syn.fit_batch(args.batch_size, args.n_rand, args.num_instance, seed=args.seed * 1000003 + step)
        yield {k: v.to(dev, non_blocking=True) for k, v in tp.items()}
        step += 1


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
    FitLoop(model, batches(args, dev), lrate=args.lrate, tri_plane_lrate=args.tri_plane_lrate, lrate_decay=args.lrate_decay,
            tv_loss_coef=args.tv_loss_coef, l1_loss_coef=args.l1_loss_coef, use_clamp=args.use_clamp, n_samples=args.n_samples,
            n_importance=args.n_importance, perturb=args.perturb, chunk=args.chunk, ft_triplane_only=args.ft_triplane_only,
            n_iteration=args.n_iteration, i_print=args.i_print, i_weights=args.i_weights, basedir=args.basedir, expname=args.expname,
            ft_path=args.ft_path, no_reload=args.no_reload).run_loop()


if __name__ == "__main__":
    main()
