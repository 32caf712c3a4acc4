"""DDIM inversion and bits-per-dim evaluation on the fused HIP kernels (hl_diffusion_eval.hip) against the reference's goldens
(tests/golden/gen_golden_eval.py) and the float64 restatement of tests/test_diffusion_eval_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_diffusion_eval_cpu import (BPD_CASES, BPD_SEED, assert_close_to_f64, bpd_case, calc_bpd_f64, diffusion, golden,
                                           noise_draw)
from tests.test_oracle_diffusion import _stub, load_unet_case

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


def stub_model(kind, xc):
    """The golden's stubs on the device (+ - * clamp only: exact IEEE on any device); xc is the condition the closure binds."""
    def model(x, t, _xc, y=None):
        e = _stub(x, t, xc, y)
        if kind == "eps":
            return e
        if kind == "near":
            return x + 0.01 * e
        return torch.cat([e, (0.3 * x - 0.2 * xc).clamp(-1, 1)], dim=1)
    return model


class Draws:
    def __init__(self, seed):
        self.seed, self.n = seed, 0

    def __call__(self, ref):
        out = noise_draw(self.seed, self.n, ref.shape).to(ref.device)
        self.n += 1
        return out


def with_noise(draws, fn):
    orig = torch.randn_like
    torch.randn_like = draws
    try:
        return fn()
    finally:
        torch.randn_like = orig


def run_bpd(d, kind, xs, xc, y, seed=BPD_SEED, pass_cond=True):
    xs_d, xc_d = torch.as_tensor(xs).to(dev), torch.as_tensor(xc).to(dev)
    draws = Draws(seed)
    model = stub_model(kind, xc_d)
    r = with_noise(draws, lambda: d.calc_bpd_loop(model, xs_d, clip_denoised=True, model_kwargs={"y": torch.as_tensor(y).to(dev)},
                                                  x_cond=xc_d if pass_cond else None))
    assert draws.n == d.num_timesteps                        # one randn_like per timestep, like the reference
    return r


@pytest.mark.parametrize("tag,spec", [("full", [1000]), ("ddim50", "ddim50"), ("r250", "250")])
@pytest.mark.parametrize("clip", [True, False])
def test_reverse_steps_match_reference(tag, spec, clip):
    g = golden()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((3, 27, 8, 8), generator=gen)
    xc = torch.randn((3, 27, 8, 8), generator=gen) * 0.5
    y = torch.tensor([0, 3, 1])
    d = diffusion(spec)
    c = int(clip)
    t = torch.from_numpy(g[f"rev_{tag}_{c}_t"]).long()
    r = d.ddim_reverse_sample(stub_model("eps", xc.to(dev)), x.to(dev), t.to(dev), clip_denoised=clip, model_kwargs={"y": y.to(dev)},
                              x_cond=xc.to(dev))

    def near(a, b):   # the bound of test_unet_gpu.py::test_sampler_steps_match_reference: 2 ulp of the host's fp32 schedule scalars
        return ((a.cpu() - b).abs() <= 3e-7 * b.abs() + 2e-7).all()

    assert near(r["sample"], torch.from_numpy(g[f"rev_{tag}_{c}_sample"]))
    assert near(r["pred_xstart"], torch.from_numpy(g[f"rev_{tag}_{c}_x0"]))


@pytest.mark.parametrize("sh,name", [("v", n) for n in BPD_CASES] + [("s", "eps_large"), ("s", "range")])
def test_bpd_loop_stub_matches_reference_and_float64(sh, name):
    """Every mean / variance type, the vector path (n = 1728) and the scalar path (n = 105)."""
    g = golden()
    d, kind, xs, xc, y = bpd_case(g, sh, name)
    r = run_bpd(d, kind, xs, xc, y)
    got = {k: r[k].cpu().numpy() for k in KEYS}
    assert got["vb"].shape == (2, 10) and got["total_bpd"].shape == (2,)
    assert_close_to_f64(got, calc_bpd_f64(d, kind, xs.astype(np.float64), xc.astype(np.float64), y), f"{sh}/{name}")
    for k in ("xstart_mse", "mse", "prior_bpd"):
        np.testing.assert_allclose(got[k], g[f"bpd_{sh}_{name}_{k}"], rtol=1e-5, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(got["vb"][:, :-1], g[f"bpd_{sh}_{name}_vb"][:, :-1], rtol=1e-5, atol=1e-6, err_msg="KL")
    np.testing.assert_allclose(got["vb"][:, -1], g[f"bpd_{sh}_{name}_vb"][:, -1], rtol=2e-5, err_msg="decoder NLL")
    np.testing.assert_allclose(got["total_bpd"], g[f"bpd_{sh}_{name}_total_bpd"], rtol=2e-5)


def test_bpd_loop_is_bit_reproducible():
    g = golden()
    d, kind, xs, xc, y = bpd_case(g, "v", "range")
    a, b = run_bpd(d, kind, xs, xc, y), run_bpd(d, kind, xs, xc, y)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["eps_large", "prevx", "range"])
def test_fused_terms_match_the_vb_terms_algebra_on_the_gpu(name):
    """Column k of calc_bpd_loop against the existing differentiable _vb_terms_bpd (tensor algebra on the GPU) at the same x_t."""
    g = golden()
    d, kind, xs, xc, y = bpd_case(g, "v", name)
    r = run_bpd(d, kind, xs, xc, y)
    xs_d, xc_d, y_d = torch.from_numpy(xs).to(dev), torch.from_numpy(xc).to(dev), torch.from_numpy(y).to(dev)
    model = d._wrap_model(stub_model(kind, xc_d))          # _vb_terms_bpd is below SpacedDiffusion's wrapping
    T = d.num_timesteps
    for k, t in enumerate(range(T - 1, -1, -1)):
        tb = torch.full((2,), t, dtype=torch.int64, device=dev)
        nz = noise_draw(BPD_SEED, k, xs.shape).to(dev)
        x_t = d.q_sample(xs_d, tb, noise=nz)
        with torch.no_grad():
            ref = d._vb_terms_bpd(model, xs_d, x_t, tb, clip_denoised=True, model_kwargs={"y": y_d})
        torch.testing.assert_close(r["vb"][:, k], ref["output"], rtol=1e-5, atol=1e-6)
        xm = ((ref["pred_xstart"] - xs_d) ** 2).mean(dim=(1, 2, 3))
        torch.testing.assert_close(r["xstart_mse"][:, k], xm, rtol=1e-5, atol=1e-7)


def test_out_of_range_timestep():
    from humanliff_amd import _lib
    d = diffusion("ddim10")
    x = torch.zeros((2, 3, 4, 4), device=dev)
    model = lambda xx, tt, xc, **k: xx  # noqa: E731
    with pytest.raises(IndexError):
        d.ddim_reverse_sample(model, x, torch.tensor([0, 10], device=dev))
    with pytest.raises(IndexError):
        d.ddim_reverse_sample(model, x, torch.tensor([-1, 0], device=dev))
    # the kernels themselves never read outside the table: that sample's outputs become NaN
    L = _lib.lib()
    tab = d._table("eval", dev)
    t = torch.tensor([3, 10], device=dev)
    n = 48
    vb, xm, mse = (torch.zeros((2, 1), device=dev) for _ in range(3))
    nbytes = L.hl_diffusion_vb_scratch_bytes(n, 2)
    scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    _lib.check(L.hl_diffusion_vb_terms(0, 0, 1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, n, _lib.ptr(tab), _lib.ptr(t), n, 2,
                                       10, _lib.ptr(vb), _lib.ptr(xm), _lib.ptr(mse), 1, 0, _lib.ptr(scratch, torch.float64), nbytes,
                                       _lib.stream_ptr()))
    sample = torch.zeros_like(x)
    _lib.check(L.hl_diffusion_reverse_step(0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(tab), _lib.ptr(t), _lib.ptr(sample), None, n, 2, 10, 1,
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(vb[0]).all() and torch.isnan(vb[1]).all() and torch.isnan(mse[1]).all()
    assert torch.isfinite(sample[0]).all() and torch.isnan(sample[1]).all()
    assert L.hl_diffusion_vb_terms(0, 1, 1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, n, _lib.ptr(tab), _lib.ptr(t), n, 2,
                                   10, _lib.ptr(vb), _lib.ptr(xm), _lib.ptr(mse), 1, 0, _lib.ptr(scratch, torch.float64), nbytes,
                                   _lib.stream_ptr()) == -1      # a learned variance type without the variance half


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 27, 8, 8)])
def test_reverse_step_scalar_and_vector_paths(shape):
    """n % 4 != 0 takes the scalar path; both agree with the reference's tensor algebra on the device."""
    d = diffusion("ddim50")
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=gen).to(dev)
    xc = (torch.randn(shape, generator=gen) * 0.5).to(dev)
    y = torch.tensor([1, 2], device=dev)
    t = torch.tensor([49, 7], device=dev)
    model = stub_model("eps", xc)
    r = d.ddim_reverse_sample(model, x, t, model_kwargs={"y": y})
    eps = model(x, torch.tensor(d.timestep_map, device=dev)[t], None, y=y)
    x0 = d._predict_xstart_from_eps(x, t, eps).clamp(-1, 1)
    e = d._predict_eps_from_xstart(x, t, x0)
    from humanliff_amd.improved_diffusion.gaussian_diffusion import _extract_into_tensor
    abn = _extract_into_tensor(d.alphas_cumprod_next, t, x.shape)
    want = x0 * torch.sqrt(abn) + torch.sqrt(1 - abn) * e
    assert torch.equal(r["pred_xstart"], x0)
    torch.testing.assert_close(r["sample"], want, rtol=1e-6, atol=1e-6)


def test_bpd_loop_fullsize_many_workgroups():
    """One 27 x 256 x 256 case at B = 2: 1024 workgroups per sample feed the fixed-order reduction."""
    d = diffusion("10")
    shape = (2, 27, 256, 256)
    g = torch.Generator().manual_seed(41)
    xs = (torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0).numpy()
    xc = (torch.randn(shape, generator=g) * 0.5).numpy()
    y = np.array([0, 3])
    r = run_bpd(d, "eps", xs, xc, y, seed=9300)
    got = {k: r[k].cpu().numpy() for k in KEYS}
    assert_close_to_f64(got, calc_bpd_f64(d, "eps", xs.astype(np.float64), xc.astype(np.float64), y, seed=9300), "fullsize")
    r2 = run_bpd(d, "eps", xs, xc, y, seed=9300)
    assert all(torch.equal(r[k], r2[k]) for k in KEYS)


def tiny32(spec):
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults
    g, ks, sd, _, xc, _, _ = load_unet_case("tiny32")
    a = model_and_diffusion_defaults()
    a.update(dict(in_channels=27, out_channels=27, class_cond=True, num_heads=4, rescale_timesteps=False, image_size=32,
                  num_channels=32, num_res_blocks=1, attention_resolutions="16,8", timestep_respacing=spec))
    model, diff = create_model_and_diffusion(**a)
    model.load_state_dict(sd)
    return model.to(dev).eval(), diff, xc.to(dev)


def test_tiny32_unet_bpd_matches_reference():
    g = golden()
    model, d, xc = tiny32("10")
    xs = torch.from_numpy(g["tiny32_x_start"]).to(dev)
    draws = Draws(9100)
    r = with_noise(draws, lambda: d.calc_bpd_loop(model, xs, model_kwargs={"y": torch.tensor([1, 2], device=dev)}, x_cond=xc))
    assert draws.n == 10
    for k in KEYS:
        want = torch.from_numpy(g[f"tiny32_bpd_{k}"])
        err = float(((r[k].cpu() - want).abs() / want.abs().clamp(min=1e-3)).max())
        print(f"tiny32 bpd {k}: max relative error {err:.2e}")
        assert err < 1e-4, (k, err)            # 10 UNet evaluations in fp32 (DESIGN.md quotes the measured error)


def test_tiny32_ddim_inversion_round_trip_matches_reference():
    g = golden()
    model, d, xc = tiny32("ddim10")
    y = torch.tensor([1, 2], device=dev)
    xs = torch.from_numpy(g["tiny32_x_start"]).to(dev)
    steps = list(d.ddim_reverse_sample_loop_progressive(model, xs, x_cond=xc, model_kwargs={"y": y}))
    assert len(steps) == 10 and set(steps[-1]) == {"sample", "pred_xstart"}
    x_T = d.ddim_reverse_sample_loop(model, xs, x_cond=xc, model_kwargs={"y": y})
    assert torch.equal(x_T, steps[-1]["sample"])
    err_xT = float((x_T.cpu() - torch.from_numpy(g["tiny32_inv_xT"])).abs().max())
    # the way back: ddim_sample_loop from the reference's x_T, and chained from ours (20 recurrent UNet evaluations in all)
    back = {}
    for tag, start in (("golden", torch.from_numpy(g["tiny32_inv_xT"]).to(dev)), ("chained", x_T)):
        draws = Draws(9200)
        back[tag] = with_noise(draws, lambda: d.ddim_sample_loop(model, (2, 27, 32, 32), x_cond=xc, noise=start, model_kwargs={"y": y}))
    err_back = float((back["golden"].cpu() - torch.from_numpy(g["tiny32_inv_back"])).abs().max())
    err_chain = float((back["chained"].cpu() - torch.from_numpy(g["tiny32_inv_back"])).abs().max())
    print(f"tiny32 inversion max-abs error: x_T {err_xT:.2e}, back from the reference's x_T {err_back:.2e}, chained {err_chain:.2e}")
    # the inversion (the new path): measured 7.3e-6
    assert err_xT < 1e-4, err_xT
    # the way back is the existing ddim_sample_loop, ten steps of a random-weight net from an x_T that is far from N(0, 1) (the reference's
    # own round trip misses x_start by 2.0, the net does not invert well): measured 1.2e-4 from the reference's x_T, 2.1e-4 chained
    assert err_back < 5e-4 and err_chain < 5e-4, (err_back, err_chain)
