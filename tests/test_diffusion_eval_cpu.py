"""DDIM inversion and bits-per-dim evaluation: API shape, CPU refusal, and the golden's variational-bound terms against a float64
numpy restatement of the reference's losses.py / _vb_terms_bpd / calc_bpd_loop.  CPU only."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN

M_EPS, M_X0, M_XPREV = "EPSILON", "START_X", "PREVIOUS_X"
# name: (mean type, var type, stub kind), as tests/golden/gen_golden_eval.py BPD_CASES
BPD_CASES = {
    "eps_large": (M_EPS, "FIXED_LARGE", "eps"),
    "eps_small": (M_EPS, "FIXED_SMALL", "eps"),
    "startx": (M_X0, "FIXED_LARGE", "near"),
    "prevx": (M_XPREV, "FIXED_SMALL", "near"),
    "range": (M_EPS, "LEARNED_RANGE", "range"),
}
BPD_SEED = 9000


def golden():
    return np.load(os.path.join(GOLDEN, "diffusion_eval.npz"))


def diffusion(spec, mean="EPSILON", var="FIXED_LARGE"):
    from humanliff_amd.improved_diffusion import gaussian_diffusion as gd
    from humanliff_amd.improved_diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, spec), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=gd.ModelMeanType[mean], model_var_type=gd.ModelVarType[var], loss_type=gd.LossType.MSE,
                           rescale_timesteps=False)


def noise_draw(seed, k, shape):
    g = torch.Generator().manual_seed(seed + k)
    return torch.randn(tuple(shape), generator=g)


def stub_f64(kind, x, t_orig, xc, y):
    """The golden generator's stubs (tests/golden/gen_golden_diffusion.py stub_model) in float64."""
    tt = (t_orig.astype(np.float64) * 0.001).reshape(-1, 1, 1, 1)
    yy = (y.astype(np.float64) * 0.05).reshape(-1, 1, 1, 1)
    e = np.clip(0.6 * x + 0.25 * xc - tt + yy, -1.5, 1.5) * 1.3
    if kind == "eps":
        return e
    if kind == "near":
        return x + 0.01 * e
    return np.concatenate([e, np.clip(0.3 * x - 0.2 * xc, -1, 1)], axis=1)


# ---- float64 restatement of losses.py (:12-77) -------------------------------------------------------------------------------------------
def normal_kl64(m1, lv1, m2, lv2):
    return 0.5 * (-1.0 + lv2 - lv1 + np.exp(lv1 - lv2) + (m1 - m2) ** 2 * np.exp(-lv2))


def approx_cdf64(x):
    return 0.5 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def decoder_nll64(x, mean, log_scales):
    c = x - mean
    inv = np.exp(-log_scales)
    cdf_plus = approx_cdf64(inv * (c + 1.0 / 255.0))
    cdf_min = approx_cdf64(inv * (c - 1.0 / 255.0))
    lp = np.where(x < -0.999, np.log(np.maximum(cdf_plus, 1e-12)),
                  np.where(x > 0.999, np.log(np.maximum(1.0 - cdf_min, 1e-12)), np.log(np.maximum(cdf_plus - cdf_min, 1e-12))))
    return -lp


def calc_bpd_f64(d, kind, x_start, xc, y, seed=BPD_SEED):
    """calc_bpd_loop (:792-848) in float64 on the schedule's float64 tables, with the golden's injected noise stream."""
    from humanliff_amd.improved_diffusion.gaussian_diffusion import ModelMeanType, ModelVarType
    B, C = x_start.shape[:2]
    T = d.num_timesteps
    tmap = np.array(d.timestep_map)
    mflat = lambda a: a.reshape(B, -1).mean(axis=1)  # noqa: E731
    res = {k: np.zeros((B, T)) for k in ("vb", "xstart_mse", "mse", "nll", "kl")}
    for k, t in enumerate(range(T - 1, -1, -1)):
        nz = noise_draw(seed, k, x_start.shape).double().numpy()
        x_t = d.sqrt_alphas_cumprod[t] * x_start + d.sqrt_one_minus_alphas_cumprod[t] * nz
        out = stub_f64(kind, x_t, np.full(B, tmap[t]), xc, y)
        if d.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
            out, v = out[:, :C], out[:, C:]
            if d.model_var_type == ModelVarType.LEARNED:
                lv = v
            else:
                frac = (v + 1) / 2
                lv = frac * np.log(d.betas[t]) + (1 - frac) * d.posterior_log_variance_clipped[t]
        else:
            lv = d._fixed_variance()[1][t]
        if d.model_mean_type == ModelMeanType.PREVIOUS_X:
            x0 = np.clip(out / d.posterior_mean_coef1[t] - d.posterior_mean_coef2[t] / d.posterior_mean_coef1[t] * x_t, -1, 1)
            mean = out
        else:
            x0 = out if d.model_mean_type == ModelMeanType.START_X else d.sqrt_recip_alphas_cumprod[t] * x_t - d.sqrt_recipm1_alphas_cumprod[t] * out
            x0 = np.clip(x0, -1, 1)
            mean = d.posterior_mean_coef1[t] * x0 + d.posterior_mean_coef2[t] * x_t
        lv = np.broadcast_to(lv, x_t.shape)
        true_mean = d.posterior_mean_coef1[t] * x_start + d.posterior_mean_coef2[t] * x_t
        kl = mflat(normal_kl64(true_mean, d.posterior_log_variance_clipped[t], mean, lv)) / math.log(2.0)
        nll = mflat(decoder_nll64(x_start, mean, 0.5 * lv)) / math.log(2.0)
        res["kl"][:, k], res["nll"][:, k] = kl, nll
        res["vb"][:, k] = nll if t == 0 else kl
        res["xstart_mse"][:, k] = mflat((x0 - x_start) ** 2)
        eps = (d.sqrt_recip_alphas_cumprod[t] * x_t - x0) / d.sqrt_recipm1_alphas_cumprod[t]
        res["mse"][:, k] = mflat((eps - nz) ** 2)
    qm = d.sqrt_alphas_cumprod[T - 1] * x_start
    res["prior_bpd"] = mflat(normal_kl64(qm, d.log_one_minus_alphas_cumprod[T - 1], 0.0, 0.0)) / math.log(2.0)
    res["total_bpd"] = res["vb"].sum(axis=1) + res["prior_bpd"]
    return res


# Bounds of the fp32 statements against the float64 restatement.  Measured on the golden (the reference's fp32 PyTorch-CPU run), largest
# over the seven cases: decoder NLL 9.6e-7 relative; x_0 MSE 2.6e-6 and eps MSE 1.1e-5 relative; KL terms 1.8e-4 relative but at most
# 3e-8 bits absolute (the smallest KL is 1.8e-4 bits, where -1 + lv2 - lv1 + exp(lv1 - lv2) cancels in fp32); prior 6e-5 relative of a
# term of ~1e-4 bits.  Hence: smooth terms within 2e-5 relative or 1e-6 bits absolute, the decoder NLL within 1e-5 relative (ten times
# the reference's own fp32 error, room for the device's tanh / exp / log).
KL_RTOL, KL_ATOL = 2e-5, 1e-6
NLL_RTOL = 1e-5


def assert_close_to_f64(got, want, case=""):
    """got: dict of fp32 results (B,) / (B, T) in the reference's column order; want: calc_bpd_f64."""
    for k in ("xstart_mse", "mse", "prior_bpd"):
        np.testing.assert_allclose(got[k], want[k], rtol=KL_RTOL, atol=KL_ATOL, err_msg=f"{case} {k}")
    np.testing.assert_allclose(got["vb"][:, :-1], want["vb"][:, :-1], rtol=KL_RTOL, atol=KL_ATOL, err_msg=f"{case} KL terms")
    np.testing.assert_allclose(got["vb"][:, -1], want["vb"][:, -1], rtol=NLL_RTOL, err_msg=f"{case} decoder NLL")
    np.testing.assert_allclose(got["total_bpd"], want["total_bpd"], rtol=NLL_RTOL, err_msg=f"{case} total_bpd")


def bpd_case(g, sh, name):
    mean, var, kind = BPD_CASES[name]
    d = diffusion("10", mean, var)
    xs, xc = g[f"bpd_{sh}_x_start"], g[f"bpd_{sh}_xc"]
    return d, kind, xs, xc, np.array([2, 1])


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_methods_exist_with_the_reference_parameter_order():
    from humanliff_amd.improved_diffusion.gaussian_diffusion import GaussianDiffusion
    from humanliff_amd.improved_diffusion.respace import SpacedDiffusion
    sig = inspect.signature(GaussianDiffusion.ddim_reverse_sample)
    assert list(sig.parameters)[:8] == ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "eta"]
    assert sig.parameters["eta"].default == 0.0 and sig.parameters["clip_denoised"].default is True
    assert sig.parameters["x_cond"].kind == inspect.Parameter.KEYWORD_ONLY and sig.parameters["x_cond"].default is None
    sig = inspect.signature(GaussianDiffusion.calc_bpd_loop)
    assert list(sig.parameters)[:5] == ["self", "model", "x_start", "clip_denoised", "model_kwargs"]
    assert sig.parameters["x_cond"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(GaussianDiffusion._prior_bpd).parameters) == ["self", "x_start"]
    for name in ("ddim_reverse_sample_loop", "ddim_reverse_sample_loop_progressive"):
        ps = inspect.signature(getattr(GaussianDiffusion, name)).parameters
        assert list(ps)[:3] == ["self", "model", "x_start"]
        assert all(ps[k].kind == inspect.Parameter.KEYWORD_ONLY for k in list(ps)[3:])
    for name in ("ddim_reverse_sample", "calc_bpd_loop", "_prior_bpd", "ddim_reverse_sample_loop"):
        assert callable(getattr(SpacedDiffusion, name))


def test_eta_must_be_zero():
    d = diffusion("ddim10")
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(AssertionError):
        d.ddim_reverse_sample(lambda *a, **k: x, x, torch.tensor([0]), eta=0.5)


def test_cpu_tensors_raise():
    d = diffusion("10")
    x = torch.zeros(2, 3, 4, 4)
    model = lambda xx, tt, xc, **k: xx  # noqa: E731
    with pytest.raises(RuntimeError):
        d.ddim_reverse_sample(model, x, torch.tensor([0, 1]))
    with pytest.raises(RuntimeError):
        d.calc_bpd_loop(model, x)
    with pytest.raises(RuntimeError):
        d._prior_bpd(x)
    with pytest.raises(RuntimeError):
        d.ddim_reverse_sample_loop(model, x)


def test_golden_covers_every_decoder_branch():
    g = golden()
    xs = g["bpd_v_x_start"]
    assert (xs == -1.0).any() and (xs == 1.0).any() and ((xs > -0.999) & (xs < 0.999)).any()
    assert np.allclose(np.round((xs + 1) * 127.5), (xs + 1) * 127.5, atol=1e-5)


@pytest.mark.parametrize("sh,name", [("v", n) for n in BPD_CASES] + [("s", "eps_large"), ("s", "range")])
def test_golden_bpd_matches_float64_restatement(sh, name):
    """The reference's fp32 calc_bpd_loop (the golden) against the float64 restatement above: pins what the decoder NLL, the KL terms,
    the MSEs and the prior compute, and measures the fp32 error the GPU tests allow."""
    g = golden()
    d, kind, xs, xc, y = bpd_case(g, sh, name)
    want = calc_bpd_f64(d, kind, xs.astype(np.float64), xc.astype(np.float64), y)
    got = {k: g[f"bpd_{sh}_{name}_{k}"] for k in ("vb", "xstart_mse", "mse", "prior_bpd", "total_bpd")}
    assert got["vb"].shape == (2, 10) and got["prior_bpd"].shape == (2,)
    assert_close_to_f64(got, want, f"{sh}/{name}")
    # the last column is t == 0 (loop order, t descending): the decoder NLL, not the KL
    assert not np.allclose(want["nll"][:, -1], want["kl"][:, -1], rtol=1e-3)
