"""The fused optimizer tail (csrc/hl_optim.hip through humanliff_amd.optim.FusedAdamW) and the native TrainLoop on the MI355X:
  - the fused step against clip_grad_value_ + torch.optim.AdamW (foreach and single-tensor) + update_ema on the same device;
  - bit-reproducibility, and no host synchronisation inside the step;
  - TrainLoop against the reference's TrainLoop (tests/golden/train_loop_tiny32.npz, gen_golden_train_loop.py);
  - resume from a checkpoint, bit-identical to an uninterrupted run; use_amp's scaled gradients; the 497 M-parameter production net."""
import os

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from humanliff_amd.improved_diffusion import train_util
from humanliff_amd.improved_diffusion.nn import update_ema
from humanliff_amd.improved_diffusion.resample import ScheduleSampler
from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults
from humanliff_amd.improved_diffusion.train_util import TrainLoop
from humanliff_amd.optim import FusedAdamW
from tests.golden_util import GOLDEN
from tests.train_loop_cases import LOOP, NP_SEED, NSLICE, WDS, batches, model_overrides, noise_stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (1, 3, 27, 4097, (1 << 20) + 5)


def ulps(a, b):
    """Elementwise distance in fp32 ulps (NaN at the same place counts 0, NaN against a number a huge value)."""
    ia = a.contiguous().view(torch.int32).long()
    ib = b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = (ia - ib).abs()
    both_nan = torch.isnan(a) & torch.isnan(b)
    return torch.where(both_nan, torch.zeros_like(d), d)


def rel(a, b):
    """max |a - b| / max |b| over the finite elements (NaN / inf must sit at the same places)."""
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    f = torch.isfinite(b)
    if not f.any():
        return 0.0
    return float((a[f].double() - b[f].double()).abs().max() / b[f].double().abs().max().clamp_min(1e-30))


def make_case(seed, offsets=True):
    """~50 parameters of the sizes above, every fifth a view at a one-element storage offset; their gradients for 5 steps (the
    third step's gradients carry +inf, -inf and one NaN)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    params, grads = [], []
    for i in range(50):
        n = SIZES[i % len(SIZES)]
        if offsets and i % 5 == 2:
            store = torch.randn(n + 1, device=DEV, generator=g)
            params.append(store[1:])
        else:
            params.append(torch.randn(n, device=DEV, generator=g))
        grads.append([torch.randn(n, device=DEV, generator=g) * (0.2 + i % 3) for _ in range(5)])
    grads[4][2][0] = float("inf")
    grads[9][2][1] = -float("inf")
    grads[14][2][2] = float("nan")
    return params, grads


def run_fused(params0, grads, wd, rates, clip, steps=5):
    ps = [p.clone() if p.storage_offset() == 0 else torch.cat([p.new_zeros(1), p])[1:] for p in params0]
    opt = FusedAdamW(ps, lr=1e-3, weight_decay=wd)
    emas = [[p.detach().clone() for p in ps] for _ in rates]
    opt.attach_ema(emas, rates)
    out = []
    for s in range(steps):
        for p, gl in zip(ps, grads):
            p.grad = gl[s].clone() if p.grad is None else p.grad.copy_(gl[s])
        opt.param_groups[0]["lr"] = 1e-3 * (1 - 0.1 * s)
        opt.step(clip_value=clip)
        out.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
                    [opt.state[p]["exp_avg_sq"].clone() for p in ps], [[e.clone() for e in el] for el in emas], opt.grad_sqsum.clone()))
    return out, ps, opt


def run_torch(params0, grads, wd, rates, clip, foreach, steps=5):
    ps = [p.detach().clone().requires_grad_(True) for p in params0]
    opt = torch.optim.AdamW(ps, lr=1e-3, weight_decay=wd, foreach=foreach)
    emas = [[p.detach().clone() for p in ps] for _ in rates]
    out = []
    for s in range(steps):
        for p, gl in zip(ps, grads):
            p.grad = gl[s].clone()
        sq = sum(float((gl[s].double() ** 2).sum()) for gl in grads)
        opt.param_groups[0]["lr"] = 1e-3 * (1 - 0.1 * s)
        torch.nn.utils.clip_grad_value_(ps, clip)
        opt.step()
        for r, el in zip(rates, emas):
            update_ema(el, ps, rate=r)
        out.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
                    [opt.state[p]["exp_avg_sq"].clone() for p in ps], [[e.clone() for e in el] for el in emas], sq))
    return out


@pytest.mark.parametrize("wd,rates", [(0.0, (0.9999,)), (0.01, (0.9999, 0.99)), (0.01, (0.999, 0.99, 0.9))])
def test_fused_step_matches_torch_adamw(wd, rates):
    params, grads = make_case(seed=3)
    got, _, _ = run_fused(params, grads, wd, rates, clip=0.5)
    for foreach in (True, False):
        want = run_torch(params, grads, wd, rates, clip=0.5, foreach=foreach)
        for s in range(5):
            (gp, gm, gv, ge, gsq), (wp, wm, wv, we, wsq) = got[s], want[s]
            pairs = list(zip(gp, wp)) + list(zip(gm, wm)) + list(zip(gv, wv)) + [(a, b) for el, wl in zip(ge, we) for a, b in zip(el, wl)]
            # The kernel follows the multi-tensor path's op order and fused multiply-adds: it is BIT-IDENTICAL to torch's foreach
            # AdamW + clip_grad_value_ + update_ema at every step, inf / NaN gradients included (so within the issue's 1 ulp at step 1).
            # The single-tensor path rounds differently (no fma; division by bias_correction2_sqrt as a multiplication), and where
            # p - lr * update cancels, one rounding apart is many ulps of the result: it is held to the relative bound at every step.
            if foreach:
                worst = max(int(ulps(a, b).max()) for a, b in pairs)
                assert worst == 0, f"step {s + 1}: {worst} ulps from torch's foreach AdamW"
            worst = max(rel(a, b) for a, b in pairs)
            assert worst <= 1e-6, f"step {s + 1} (foreach={foreach}): relative {worst}"
            if np.isfinite(wsq):
                assert abs(float(gsq) - wsq) <= 1e-12 * wsq, (s, float(gsq), wsq)
            else:
                assert not np.isfinite(float(gsq))


def test_fused_step_without_clip_and_without_grad():
    """clip_value None passes the gradient through; a parameter without .grad keeps p / moments and still gets its EMA."""
    params, grads = make_case(seed=5, offsets=False)
    ps = [p.clone().requires_grad_(True) for p in params[:10]]
    ref = [p.detach().clone().requires_grad_(True) for p in ps]
    opt, ropt = FusedAdamW(ps, lr=1e-3, weight_decay=0.0), torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.0, foreach=True)
    ema, rema = [p.detach().clone() for p in ps], [p.detach().clone() for p in ref]
    opt.attach_ema([ema], [0.99])
    for i in range(1, 10):
        ps[i].grad, ref[i].grad = grads[i][0].clone(), grads[i][0].clone()
    opt.step()
    ropt.step()
    update_ema(rema, ref, rate=0.99)
    assert torch.equal(ps[0].detach(), params[0]) and len(opt.state[ps[0]]) == 0
    for a, b in zip(ps + ema, ref + rema):
        assert int(ulps(a.detach(), b.detach()).max()) == 0
    assert torch.equal(ps[3].grad, grads[3][0])          # .grad is never written


def test_fused_step_reproducible_and_no_host_sync():
    params, grads = make_case(seed=7)
    a, _, _ = run_fused(params, grads, 0.01, (0.9999, 0.99), clip=0.5, steps=3)
    b, ps, opt = run_fused(params, grads, 0.01, (0.9999, 0.99), clip=0.5, steps=3)
    for (ap, am, av, ae, asq), (bp, bm, bv, be, bsq) in zip(a, b):
        for x, y in zip(ap + am + av + [e for el in ae for e in el], bp + bm + bv + [e for el in be for e in el]):
            assert torch.equal(x, y) or (torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x.nan_to_num(), y.nan_to_num()))
        assert torch.equal(asq, bsq) or (bool(torch.isnan(asq)) and bool(torch.isnan(bsq)))
    # steady state: the table is packed; a step enqueues its two launches and returns
    for p, gl in zip(ps, grads):
        p.grad.copy_(gl[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            opt.step(clip_value=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ---- TrainLoop --------------------------------------------------------------------------------------------------------------------
def tiny(seed=1):
    a = model_and_diffusion_defaults()
    a.update(model_overrides())
    model, diffusion = create_model_and_diffusion(**a)
    model.load_state_dict(syn.state_from_shapes([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed), strict=True)
    return model.to(DEV).train(), diffusion


class FixedSampler(ScheduleSampler):
    """Hands out given timesteps in order (weights 1): two runs see the same t."""

    def __init__(self, diffusion, ts):
        self.diffusion, self.ts = diffusion, list(ts)

    def weights(self):
        return np.ones([self.diffusion.num_timesteps])

    def sample(self, batch_size, device):
        t = torch.as_tensor(self.ts.pop(0), dtype=torch.int64)
        assert t.shape == (batch_size,)
        return t.to(device), torch.ones(batch_size, device=device)


def with_noise(diffusion, noises, record=None):
    orig = diffusion.training_losses

    def training_losses(m, x_start, x_cond, t, model_kwargs=None, noise=None):
        out = orig(m, x_start, x_cond, t, model_kwargs=model_kwargs, noise=noises.pop(0).to(x_start.device))
        if record is not None:
            record.append(out["loss"].detach().cpu().numpy())
        return out

    diffusion.training_losses = training_losses


def noise_list(n, shape=(2, 27, 32, 32)):
    g = noise_stream()
    return [torch.randn(shape, generator=g) for _ in range(n)]


def make_loop(model, diffusion, data, tmp, steps, **kw):
    args = dict(model=model, diffusion=diffusion, data=iter(data), batch_size=LOOP["batch_size"], microbatch=LOOP["microbatch"],
                lr=LOOP["lr"], ema_rate=LOOP["ema_rate"], log_interval=1, save_interval=LOOP["save_interval"], resume_checkpoint="",
                use_amp=False, weight_decay=0.0, lr_anneal_steps=steps, use_cond=True, log_dir=str(tmp))
    args.update(kw)
    return TrainLoop(**args)


@pytest.mark.parametrize("case", [0, 1])
def test_train_loop_matches_reference(case, tmp_path):
    g = np.load(os.path.join(GOLDEN, "train_loop_tiny32.npz"))
    P = f"wd{case}_"
    model, diffusion = tiny()
    rec = []
    with_noise(diffusion, noise_list(2 * LOOP["steps"]), rec)
    loop = make_loop(model, diffusion, batches(), tmp_path, LOOP["steps"], weight_decay=WDS[case])
    norms = []
    dump = loop.log.dump

    def dump_rec():
        out = dump()
        norms.append(out["grad_norm"])
        return out

    loop.log.dump = dump_rec
    np.random.seed(NP_SEED)
    loop.run_loop()
    loss = np.stack(rec)
    assert np.abs(loss[:2] - g[P + "loss"][:2]).max() <= 2.5e-6 * np.abs(g[P + "loss"][:2]).max()
    assert abs(norms[0] - g[P + "grad_norm"][0]) <= 2.5e-6 * g[P + "grad_norm"][0], (norms, g[P + "grad_norm"])
    assert np.allclose(norms, g[P + "grad_norm"], rtol=1e-4)
    sd = dict(model.named_parameters())
    names = [n for n, _ in model.named_parameters()]
    s = LOOP["steps"] - 1
    bound = 2 * LOOP["lr"] * LOOP["steps"]
    close = total = 0
    for k in map(str, g[P + "keys"]):
        i = names.index(k)
        vals = [(sd[k].detach().reshape(-1)[:NSLICE], g[f"{P}s{s}_p_{k}"])]
        for r, ema in zip(loop.ema_rate, loop.ema_params):
            vals.append((ema[i].reshape(-1)[:NSLICE], g[f"{P}s{s}_e{r}_{k}"]))
        for got, want in vals:
            got = got.double().cpu().numpy()
            err = np.abs(got - want)
            assert err.max() <= bound, (k, err.max())       # a gradient near zero may flip sign: m / sqrt(v) moves p by ~lr
            close += int(np.sum(err <= 1e-6 * np.abs(want)))
            total += err.size
    print(f"case {case}: {close} of {total} picked elements within 1e-6 relative")
    assert close >= 0.999 * total, (close, total)          # over every picked parameter and EMA element together
    csv_path = os.path.join(str(tmp_path), "progress.csv")
    assert os.path.exists(csv_path)
    head = open(csv_path).readline().strip().split(",")
    for key in ("loss", "mse", "grad_norm", "step", "samples"):
        assert key in head, head
    assert any(k.startswith("loss_q") for k in head) and any(k.startswith("mse_q") for k in head), head


def test_train_loop_resume_is_bit_identical(tmp_path):
    steps = 4
    data = batches(steps=steps)
    rng = np.random.RandomState(9)
    ts = [rng.randint(0, 1000, size=2) for _ in range(2 * steps)]
    noises = noise_list(2 * steps)
    # uninterrupted
    m1, d1 = tiny()
    with_noise(d1, list(noises))
    a = make_loop(m1, d1, data, tmp_path / "a", steps, schedule_sampler=FixedSampler(d1, ts), weight_decay=0.01)
    a.run_loop()
    # two steps, then a fresh loop from model000002.pt
    m2, d2 = tiny()
    with_noise(d2, list(noises[:4]))
    b = make_loop(m2, d2, data[:2], tmp_path / "b", 2, schedule_sampler=FixedSampler(d2, ts[:4]), weight_decay=0.01)
    b.run_loop()
    assert sorted(os.listdir(tmp_path / "b")) == sorted(["progress.csv"] + train_util.checkpoint_names(0, b.ema_rate) +
                                                        train_util.checkpoint_names(2, b.ema_rate))
    m3, d3 = tiny(seed=4)                                   # (other weights: everything must come from the checkpoint)
    with_noise(d3, list(noises[4:]))
    c = make_loop(m3, d3, data[2:], tmp_path / "b", steps, schedule_sampler=FixedSampler(d3, ts[4:]), weight_decay=0.01,
                  resume_checkpoint=str(tmp_path / "b" / "model000002.pt"))
    assert c.resume_step == 2
    c.run_loop()
    for name in train_util.checkpoint_names(4, a.ema_rate):
        x = torch.load(tmp_path / "a" / name, map_location="cpu")
        y = torch.load(tmp_path / "b" / name, map_location="cpu")
        if name.startswith("opt"):
            assert x["param_groups"] == y["param_groups"]
            for k in x["state"]:
                for f in ("step", "exp_avg", "exp_avg_sq"):
                    assert torch.equal(x["state"][k][f], y["state"][k][f]), (name, k, f)
        else:
            assert x.keys() == y.keys()
            for k in x:
                assert torch.equal(x[k], y[k]), (name, k)
    # opt000004.pt is torch.optim.AdamW's format
    ref = torch.optim.AdamW(m1.parameters(), lr=1e-4, weight_decay=0.01)
    ref.load_state_dict(torch.load(tmp_path / "a" / "opt000004.pt", map_location=DEV))
    assert float(ref.state[next(m1.parameters())]["step"]) == 4.0


def test_train_loop_amp_scales_the_gradients(tmp_path, monkeypatch):
    def first_norm(scale, steps):
        monkeypatch.setattr(train_util, "AMP_LOSS_SCALE", scale)
        model, diffusion = tiny()
        with_noise(diffusion, noise_list(2 * steps))
        loop = make_loop(model, diffusion, batches(steps=steps), tmp_path / str(scale), steps, use_amp=True)
        norms = []
        dump = loop.log.dump
        loop.log.dump = lambda: norms.append(dump()["grad_norm"])
        np.random.seed(NP_SEED)
        loop.run_loop()
        return norms, model

    unscaled, _ = first_norm(1.0, 1)
    scaled, model = first_norm(65536.0, 10)
    assert abs(scaled[0] / unscaled[0] / 65536.0 - 1) <= 1e-3, (scaled[0], unscaled[0])
    assert np.all(np.isfinite(scaled))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_fused_step_production_net():
    """One fused step on the 497 M-parameter production UNet: finite, bit-reproducible, bit-identical to AdamW + clip + EMA."""
    import bench_legs
    model, _, _ = bench_legs.build_unet(DEV)
    ps = list(model.parameters())
    assert sum(p.numel() for p in ps) > 490_000_000
    g = torch.Generator(device=DEV).manual_seed(1)
    grads = [torch.randn(p.shape, device=DEV, generator=g) * 0.3 for p in ps]
    p0 = [p.detach().clone() for p in ps]

    def fused():
        with torch.no_grad():
            for p, q in zip(ps, p0):
                p.copy_(q)
        for p, gr in zip(ps, grads):
            p.grad = gr
        opt = FusedAdamW(ps, lr=1e-4, weight_decay=0.0)
        ema = [q.clone() for q in p0]
        opt.attach_ema([ema], [0.9999])
        opt.step(clip_value=0.5)
        return [p.detach().clone() for p in ps], ema, float(opt.grad_sqsum)

    a = fused()
    b = fused()
    assert a[2] == b[2] and np.isfinite(a[2])
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert all(bool(torch.isfinite(x).all()) for x in a[0])
    want_sq = sum(float((gr.double() ** 2).sum()) for gr in grads)
    assert abs(a[2] - want_sq) <= 1e-12 * want_sq
    del b
    ref = [q.clone().requires_grad_(True) for q in p0]
    for r, gr in zip(ref, grads):
        r.grad = gr.clone()
    torch.nn.utils.clip_grad_value_(ref, 0.5)
    ropt = torch.optim.AdamW(ref, lr=1e-4, weight_decay=0.0)
    ropt.step()
    rema = [q.clone() for q in p0]
    update_ema(rema, ref, rate=0.9999)
    worst = max(int(ulps(x, y.detach()).max()) for x, y in zip(a[0] + a[1], ref + rema))
    assert worst == 0, worst                             # bit-identical to torch's (foreach) AdamW + clip + EMA
