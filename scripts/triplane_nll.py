"""Bits per dimension of a tri-plane diffusion model: the reference's scripts/image_nll.py flow for tri-planes, on the fused HIP
evaluation kernels (GaussianDiffusion.calc_bpd_loop).  One process; averaging over ranks is not done.

    python scripts/triplane_nll.py --model_path model.pt --data planes.npz [script_util flags] [--out DIR]
    python scripts/triplane_nll.py --synthetic [--num_samples 4 --batch_size 2 --timestep_respacing 50]

--data: an .npz with `x_start` (N, 27, 256, 256) in [-1, 1], optionally `x_cond` (same shape; zeros if absent: layer 0) and `y` (N,)
class labels.  --synthetic: seeded weights (humanliff_amd.synthetic) and seeded inputs quantised to 255 levels.  Prints the running
mean bpd after every batch, then writes {vb,mse,xstart_mse}_terms.npz (the per-timestep means, as image_nll.py) under --out.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humanliff_amd import synthetic as syn  # noqa: E402
from humanliff_amd.improved_diffusion.script_util import (add_dict_to_argparser, args_to_dict, create_model_and_diffusion,  # noqa: E402
                                                           model_and_diffusion_defaults)


def create_argparser():
    defaults = model_and_diffusion_defaults()
    defaults.update(dict(image_size=256, in_channels=27, out_channels=27, num_channels=192, num_res_blocks=3,
                         attention_resolutions="32,16,8", class_cond=True, rescale_timesteps=False))
    defaults.update(dict(clip_denoised=True, num_samples=4, batch_size=2, model_path="", data="", out=".", synthetic=False, seed=0))
    ap = argparse.ArgumentParser()
    add_dict_to_argparser(ap, defaults)
    return ap


def batches(args, dev):
    if args.synthetic:
        g = torch.Generator().manual_seed(args.seed)
        shape = (args.num_samples, args.in_channels, args.image_size, args.image_size)
        xs = torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0
        xc = (torch.randn(shape, generator=g) * 0.5).clamp(-1, 1)
        y = torch.randint(0, 4, (args.num_samples,), generator=g)
    else:
        d = np.load(args.data)
        xs = torch.from_numpy(d["x_start"]).float()[:args.num_samples]
        xc = torch.from_numpy(d["x_cond"]).float()[:len(xs)] if "x_cond" in d.files else torch.zeros_like(xs)
        y = torch.from_numpy(d["y"]).long()[:len(xs)] if "y" in d.files else torch.zeros(len(xs), dtype=torch.int64)
    for i in range(0, len(xs), args.batch_size):
        yield xs[i:i + args.batch_size].to(dev), xc[i:i + args.batch_size].to(dev), y[i:i + args.batch_size].to(dev)


def main():
    args = create_argparser().parse_args()
    dev = torch.device("cuda:0")
    model, diffusion = create_model_and_diffusion(**args_to_dict(args, model_and_diffusion_defaults().keys()))
    if args.synthetic:
        model.load_state_dict(syn.state_from_shapes([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=1))
    else:
        model.load_state_dict(torch.load(args.model_path, map_location="cpu"))
    model.to(dev).eval()
    torch.manual_seed(args.seed)
    all_bpd, metrics = [], {"vb": [], "mse": [], "xstart_mse": []}
    for xs, xc, y in batches(args, dev):
        kw = {"y": y} if args.class_cond else {}
        m = diffusion.calc_bpd_loop(model, xs, clip_denoised=args.clip_denoised, model_kwargs=kw, x_cond=xc)
        for k in metrics:
            metrics[k].append(m[k].mean(dim=0).cpu().numpy())
        all_bpd.append(m["total_bpd"].cpu().numpy())
        bpd = float(np.concatenate(all_bpd).mean())
        print(f"done {sum(len(b) for b in all_bpd)} samples: bpd={bpd}", flush=True)
        assert np.isfinite(bpd), "non-finite bits per dimension"
    os.makedirs(args.out, exist_ok=True)
    for k, v in metrics.items():
        np.savez(os.path.join(args.out, f"{k}_terms.npz"), np.mean(np.stack(v), axis=0))
    print("evaluation complete")


if __name__ == "__main__":
    main()
