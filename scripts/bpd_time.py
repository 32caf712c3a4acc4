"""Time of the bits-per-dim evaluation on the production net (27 x 256 x 256, synthetic weights), B = 1 and B = 4:
  - one calc_bpd_loop step (randn + fused q_sample + UNet forward + fused vb-terms kernel), from a 20-step respaced loop;
  - a plain UNet forward at the same batch;
  - the tail after the model alone: the fused kernels (q_sample + vb terms) against the eager tensor algebra of the same terms
    (q_sample, p_mean_variance, q_posterior, normal_kl, the decoder NLL, where, three mean_flat, the eps re-derivation), the
    reference's calc_bpd_loop body.
Device time from a host clock around synchronised work (the tails: CUDA events over 50 repetitions).

    python scripts/bpd_time.py [--batches 1,4] [--steps 20]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from humanliff_amd import _lib  # noqa: E402
from humanliff_amd.improved_diffusion import gaussian_diffusion as gd  # noqa: E402
from humanliff_amd.improved_diffusion.losses import discretized_gaussian_log_likelihood, normal_kl  # noqa: E402
from humanliff_amd.improved_diffusion.nn import mean_flat  # noqa: E402
from humanliff_amd.improved_diffusion.script_util import create_gaussian_diffusion  # noqa: E402


def sync_time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def event_time(fn, reps=50):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def eager_tail(d, xs, noise, out, t):
    """The reference's per-step algebra after the model call (calc_bpd_loop :808-835, _vb_terms_bpd, p_mean_variance) on the GPU."""
    x_t = d.q_sample(xs, t, noise=noise)
    true_mean, _, true_lv = d.q_posterior_mean_variance(x_start=xs, x_t=x_t, t=t)
    mean, lv, x0 = d._pmv_autograd(out, x_t, t, True)
    kl = mean_flat(normal_kl(true_mean, true_lv, mean, lv)) / np.log(2.0)
    nll = mean_flat(-discretized_gaussian_log_likelihood(xs, means=mean, log_scales=0.5 * lv)) / np.log(2.0)
    vb = torch.where(t == 0, nll, kl)
    xm = mean_flat((x0 - xs) ** 2)
    eps = d._predict_eps_from_xstart(x_t, t, x0)
    return vb, xm, mean_flat((eps - noise) ** 2)


def fused_tail(d, xs, noise, out, t, res, scratch, nbytes):
    L, st = _lib.lib(), _lib.stream_ptr()
    B, T = xs.shape[0], d.num_timesteps
    n = xs.numel() // B
    tab = d._table("eval", xs.device)
    x_t = torch.empty_like(xs)
    _lib.check(L.hl_diffusion_q_sample(_lib.ptr(xs), _lib.ptr(noise), _lib.ptr(tab), _lib.ptr(t), _lib.ptr(x_t), n, B, T, st))
    _lib.check(L.hl_diffusion_vb_terms(0, 0, 1, _lib.ptr(xs), _lib.ptr(x_t), _lib.ptr(noise), _lib.ptr(out), None, n, _lib.ptr(tab),
                                       _lib.ptr(t), n, B, T, _lib.ptr(res[0]), _lib.ptr(res[1]), _lib.ptr(res[2]), T, 0,
                                       _lib.ptr(scratch, torch.float64), nbytes, st))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_unet(dev)
    F4 = bench.F4
    d = create_gaussian_diffusion(steps=F4["diffusion_steps"], noise_schedule=F4["noise_schedule"], rescale_timesteps=F4["rescale_timesteps"],
                                  timestep_respacing=str(args.steps))
    assert d.model_mean_type == gd.ModelMeanType.EPSILON and d.model_var_type == gd.ModelVarType.FIXED_LARGE
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(5)
        xs = (torch.randint(0, 256, (B, 27, 256, 256), generator=g).float() / 127.5 - 1.0).to(dev)
        xc = torch.zeros_like(xs)
        y = torch.zeros((B,), dtype=torch.int64, device=dev)
        t = torch.full((B,), 500, dtype=torch.int64, device=dev)
        with torch.no_grad():
            fwd = lambda: model(xs, t, xc, y=y)  # noqa: E731
            for _ in range(3):
                fwd()
            t_fwd = sync_time(fwd, 10)
            d.calc_bpd_loop(model, xs, model_kwargs={"y": y}, x_cond=xc)          # warm-up (tables, wrapper, workspace)
            t_loop = sync_time(lambda: d.calc_bpd_loop(model, xs, model_kwargs={"y": y}, x_cond=xc), 2)
            noise = torch.randn_like(xs)
            out = torch.randn_like(xs)
            tt = torch.full((B,), 7, dtype=torch.int64, device=dev)
            res = [torch.empty((B, d.num_timesteps), device=dev) for _ in range(3)]
            nbytes = _lib.lib().hl_diffusion_vb_scratch_bytes(xs.numel() // B, B)
            scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            t_fused = event_time(lambda: fused_tail(d, xs, noise, out, tt, res, scratch, nbytes))
            t_eager = event_time(lambda: eager_tail(d, xs, noise, out, tt))
            vb_e, xm_e, mse_e = eager_tail(d, xs, noise, out, tt)
            fused_tail(d, xs, noise, out, tt, res, scratch, nbytes)
            torch.cuda.synchronize()
            agree = max(float(((res[0][:, 0] - vb_e).abs() / vb_e.abs()).max()), float(((res[2][:, 0] - mse_e).abs() / mse_e).max()))
        per_step = t_loop / d.num_timesteps
        print(f"B={B}: bpd step {per_step * 1e3:.3f} ms, plain forward {t_fwd * 1e3:.3f} ms (step / forward {per_step / t_fwd:.3f}); "
              f"tail fused {t_fused * 1e6:.1f} us vs eager {t_eager * 1e6:.1f} us ({t_eager / t_fused:.1f}x, "
              f"{(t_eager - t_fused) / per_step * 100:.2f} % of a step); fused vs eager terms rel {agree:.1e}", flush=True)


if __name__ == "__main__":
    main()
