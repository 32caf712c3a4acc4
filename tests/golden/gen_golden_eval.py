"""Golden vectors of the likelihood evaluation and the DDIM inversion FROM THE REFERENCE.

Runs only in the build container (imports /root/reference/human_diffusion/improved_diffusion unmodified).

    python tests/golden/gen_golden_eval.py      -> tests/golden/diffusion_eval.npz

Exercised: GaussianDiffusion.ddim_reverse_sample (gaussian_diffusion.py:531-567), _prior_bpd / calc_bpd_loop (:774-848) through
_vb_terms_bpd (:653-687) and losses.py, SpacedDiffusion's model wrapping (respace.py:63-122), ddim_sample_loop.
The reference calls the model without a condition in both methods; the condition reaches it through a closure
(`lambda x, t, xc, **k: stub(x, t, XC, **k)`), the HIP side passes x_cond=XC.  Noise is injected through th.randn_like
(draw k = a generator seeded with SEED + k), exactly as the sampler goldens do.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden_diffusion import UNET_CASES, load_seeded, stub_model, unet_args, unet_inputs  # noqa: E402  (puts the reference on sys.path)
from improved_diffusion import gaussian_diffusion as gd  # noqa: E402
from improved_diffusion.respace import SpacedDiffusion, space_timesteps  # noqa: E402
from improved_diffusion.script_util import create_model_and_diffusion  # noqa: E402

M, V = gd.ModelMeanType, gd.ModelVarType

# name: (mean type, var type, stub kind); stub kinds are defined in tests/test_diffusion_eval_cpu.py (stub_out) in the same words
BPD_CASES = {
    "eps_large": (M.EPSILON, V.FIXED_LARGE, "eps"),
    "eps_small": (M.EPSILON, V.FIXED_SMALL, "eps"),
    "startx": (M.START_X, V.FIXED_LARGE, "near"),
    "prevx": (M.PREVIOUS_X, V.FIXED_SMALL, "near"),
    "range": (M.EPSILON, V.LEARNED_RANGE, "range"),
}
BPD_SHAPES = {"v": (2, 27, 8, 8), "s": (2, 3, 5, 7)}     # n % 4 == 0 (vector path) and n = 105 (scalar path)


def stub_out(kind, x, t, xc, y):
    """Only + - * clamp: bit-identical on every CPU ISA."""
    e = stub_model(x, t, xc, y=y)
    if kind == "eps":
        return e
    if kind == "near":                      # an x_0 / x_{t-1} prediction close to x_t, so the decoder term is well conditioned
        return x + 0.01 * e
    return torch.cat([e, (0.3 * x - 0.2 * xc).clamp(-1, 1)], dim=1)


def quantised(shape, seed):
    """x_start on the 255-level grid of [-1, 1] (uint8 images rescaled), exact +-1 included."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, generator=g).float()
    q.view(-1)[:8] = torch.tensor([0.0, 255.0, 0.0, 255.0, 1.0, 254.0, 128.0, 127.0])
    return q / 127.5 - 1.0


class Draws:
    def __init__(self, seed):
        self.seed, self.n = seed, 0

    def __call__(self, ref):
        g = torch.Generator().manual_seed(self.seed + self.n)
        self.n += 1
        return torch.randn(tuple(ref.shape), generator=g)


def spaced(spec, mean=M.EPSILON, var=V.FIXED_LARGE):
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, spec), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=mean, model_var_type=var, loss_type=gd.LossType.MSE, rescale_timesteps=False)


def with_noise(draws, fn):
    orig = torch.randn_like
    torch.randn_like = draws
    try:
        return fn()
    finally:
        torch.randn_like = orig


def gen_reverse(out):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((3, 27, 8, 8), generator=g)
    xc = torch.randn((3, 27, 8, 8), generator=g) * 0.5
    y = torch.tensor([0, 3, 1])
    model = lambda xx, tt, _xc, **k: stub_model(xx, tt, xc, **k)  # noqa: E731
    for tag, spec in [("full", [1000]), ("ddim50", "ddim50"), ("r250", "250")]:
        d = spaced(spec)
        T = d.num_timesteps
        t = torch.tensor([T - 1, 0, T // 3])
        for clip in (True, False):
            r = d.ddim_reverse_sample(model, x, t, clip_denoised=clip, model_kwargs={"y": y})
            out[f"rev_{tag}_{int(clip)}_t"] = t.numpy()
            out[f"rev_{tag}_{int(clip)}_sample"] = r["sample"].numpy()
            out[f"rev_{tag}_{int(clip)}_x0"] = r["pred_xstart"].numpy()


def gen_bpd_stub(out):
    for sh, shape in BPD_SHAPES.items():
        B, C = shape[:2]
        xs = quantised(shape, seed=21)
        g = torch.Generator().manual_seed(22)
        xc = torch.randn(shape, generator=g) * 0.5
        y = torch.tensor([2, 1])
        out[f"bpd_{sh}_x_start"] = xs.numpy()
        out[f"bpd_{sh}_xc"] = xc.numpy()
        for name, (mean, var, kind) in BPD_CASES.items():
            if sh == "s" and name not in ("eps_large", "range"):
                continue
            d = spaced("10", mean, var)
            model = lambda xx, tt, _xc, kind=kind, **k: stub_out(kind, xx, tt, xc, k.get("y"))  # noqa: E731
            draws = Draws(9000)
            r = with_noise(draws, lambda: d.calc_bpd_loop(model, xs, clip_denoised=True, model_kwargs={"y": y}))
            assert draws.n == d.num_timesteps
            for k, v in r.items():
                out[f"bpd_{sh}_{name}_{k}"] = v.numpy()
            print("bpd", sh, name, "total", r["total_bpd"].numpy(), "vb[:, 0]", r["vb"][:, 0].numpy())


def gen_tiny32(out):
    args = unet_args(UNET_CASES["tiny32"][0])
    args["timestep_respacing"] = "10"
    model, diffusion = create_model_and_diffusion(**args)
    model.eval()
    load_seeded(model, seed=1)
    B = 2
    _, xc = unet_inputs(B, 32, seed=7)
    y = torch.tensor([1, 2])
    xs = quantised((B, 27, 32, 32), seed=31)
    closure = lambda xx, tt, _xc, **k: model(xx, tt, xc, **k)  # noqa: E731
    draws = Draws(9100)
    with torch.no_grad():
        r = with_noise(draws, lambda: diffusion.calc_bpd_loop(closure, xs, clip_denoised=True, model_kwargs={"y": y}))
    for k, v in r.items():
        out[f"tiny32_bpd_{k}"] = v.numpy()
    print("tiny32 bpd", r["total_bpd"].numpy())
    # DDIM-10 inversion (t ascending) of x_start, then ddim_sample_loop from the x_T it gives
    args["timestep_respacing"] = "ddim10"
    model2, d2 = create_model_and_diffusion(**args)
    model2.eval()
    load_seeded(model2, seed=1)
    closure2 = lambda xx, tt, _xc, **k: model2(xx, tt, xc, **k)  # noqa: E731
    x = xs.clone()
    with torch.no_grad():
        for i in range(d2.num_timesteps):
            x = d2.ddim_reverse_sample(closure2, x, torch.tensor([i] * B), clip_denoised=True, model_kwargs={"y": y})["sample"]
        x_T = x.clone()
        draws = Draws(9200)
        back = with_noise(draws, lambda: d2.ddim_sample_loop(model2, (B, 27, 32, 32), x_cond=xc, noise=x_T, clip_denoised=True,
                                                             model_kwargs={"y": y}, device=torch.device("cpu")))
    out["tiny32_inv_xT"] = x_T.numpy()
    out["tiny32_inv_back"] = back.numpy()
    out["tiny32_x_start"] = xs.numpy()
    print("tiny32 inversion: |x_T| mean", float(x_T.abs().mean()), "round trip max err", float((back - xs).abs().max()))


if __name__ == "__main__":
    res = {}
    gen_reverse(res)
    gen_bpd_stub(res)
    gen_tiny32(res)
    np.savez_compressed(os.path.join(HERE, "diffusion_eval.npz"), **res)
