"""Generate golden vectors for the training loop FROM THE UNMODIFIED REFERENCE TrainLoop (human_diffusion/improved_diffusion/train_util.py)
on the CPU.  Runs only where the reference is available:

    python tests/golden/gen_golden_train_loop.py

Setup: `blobfile` is stubbed in sys.modules by local-file equivalents (the reference imports it for its checkpoints) and a one-rank gloo
process group is opened through a file:// store (TrainLoop calls dist.get_world_size / get_rank / barrier).  The tiny32 controlnet net
(tests/train_loop_cases.py) trains 3 steps at batch 4, microbatch 2, ema_rate "0.9999,0.99", use_amp=False, once with weight_decay 0 and
once with 0.01.  t comes from the UniformSampler under np.random.seed(0); the q_sample noise is drawn from a seeded generator by a
wrapper around diffusion.training_losses, which also records the per-sample losses.

Stored per case (prefix wd0_ / wd1_) and step s: the losses, grad_norm (the reference's own _log_grad_norm value), the unclipped gradients,
post-step values and EMAs (both rates) of the picked parameters (their first NSLICE elements), exp_avg / exp_avg_sq after the last step,
and abs-sums over all parameters / EMAs.
It also stores LossSecondMomentResampler vectors (prefix lsm_): weights after warm-up and draws under a seed (np.int is patched to
np.int64 for numpy >= 1.24).
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference/human_diffusion")

bf = types.ModuleType("blobfile")
bf.BlobFile = open
bf.join = os.path.join
bf.dirname = os.path.dirname
bf.exists = os.path.exists
sys.modules["blobfile"] = bf
if not hasattr(np, "int"):
    np.int = np.int64

import torch.distributed as dist  # noqa: E402

from improved_diffusion import logger  # noqa: E402
from improved_diffusion.resample import LossSecondMomentResampler  # noqa: E402
from improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults  # noqa: E402
from improved_diffusion.train_util import TrainLoop  # noqa: E402

from humanliff_amd import synthetic as syn  # noqa: E402
from tests.train_loop_cases import LOOP, NP_SEED, NSLICE, PICK, WDS, batches, model_overrides, noise_stream  # noqa: E402


def run_case(wd, tmp):
    a = model_and_diffusion_defaults()
    a.update(model_overrides())
    model, diffusion = create_model_and_diffusion(**a)
    model.load_state_dict(syn.state_from_shapes([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 1), strict=True)
    names = [n for n, _ in model.named_parameters()]
    pick = [k for k in PICK if k in names]
    gn = noise_stream()
    rec = {"loss": [], "t": []}
    orig = diffusion.training_losses

    def training_losses(m, x_start, x_cond, t, model_kwargs=None, noise=None):
        noise = torch.randn(x_start.shape, generator=gn)
        out = orig(m, x_start, x_cond, t, model_kwargs=model_kwargs, noise=noise)
        rec["loss"].append(out["loss"].detach().numpy().copy())
        rec["t"].append(t.numpy().copy())
        return out

    diffusion.training_losses = training_losses
    data = iter(batches())
    loop = TrainLoop(model=model, diffusion=diffusion, data=data, batch_size=LOOP["batch_size"], microbatch=LOOP["microbatch"],
                     lr=LOOP["lr"], ema_rate=LOOP["ema_rate"], log_interval=LOOP["log_interval"], save_interval=LOOP["save_interval"],
                     resume_checkpoint="", use_amp=False, weight_decay=wd, lr_anneal_steps=LOOP["steps"], use_cond=True)
    out = {}
    gnorm = []
    orig_norm = loop._log_grad_norm

    def log_grad_norm():
        sd = dict(model.named_parameters())
        gnorm.append(float(np.sqrt(sum((p.grad ** 2).sum().item() for p in loop.master_params))))
        s = len(gnorm) - 1
        for k in pick:
            out[f"s{s}_g_{k}"] = sd[k].grad.reshape(-1)[:NSLICE].numpy().copy()
        out[f"s{s}_grad_abs_sum"] = sum(float(p.grad.double().abs().sum()) for p in loop.master_params)
        orig_norm()

    loop._log_grad_norm = log_grad_norm
    orig_step = loop.run_step

    def run_step(*args):
        orig_step(*args)
        s = len(gnorm) - 1
        sd = dict(model.named_parameters())
        for k in pick:
            i = names.index(k)
            out[f"s{s}_p_{k}"] = sd[k].detach().reshape(-1)[:NSLICE].numpy().copy()
            st = loop.opt.state[sd[k]]
            if s == LOOP["steps"] - 1:
                out[f"s{s}_m_{k}"] = st["exp_avg"].reshape(-1)[:NSLICE].numpy().copy()
                out[f"s{s}_v_{k}"] = st["exp_avg_sq"].reshape(-1)[:NSLICE].numpy().copy()
            for r, ema in zip(loop.ema_rate, loop.ema_params):
                out[f"s{s}_e{r}_{k}"] = ema[i].detach().reshape(-1)[:NSLICE].numpy().copy()
        out[f"s{s}_p_abs_sum"] = sum(float(p.detach().double().abs().sum()) for p in loop.master_params)
        out[f"s{s}_e_abs_sum"] = np.array([sum(float(p.detach().double().abs().sum()) for p in ema) for ema in loop.ema_params])
        out[f"s{s}_lr"] = loop.opt.param_groups[0]["lr"]

    loop.run_step = run_step
    np.random.seed(NP_SEED)
    loop.run_loop()
    out["loss"] = np.stack(rec["loss"])               # (steps * microbatches, microbatch)
    out["t"] = np.stack(rec["t"])
    out["grad_norm"] = np.array(gnorm)
    out["keys"] = np.array(pick)
    # the initial values of the picked parameters (EMA targets start as copies)
    m0, _ = create_model_and_diffusion(**a)
    m0.load_state_dict(syn.state_from_shapes([(k, tuple(v.shape)) for k, v in m0.state_dict().items()], 1), strict=True)
    sd0 = dict(m0.named_parameters())
    for k in pick:
        out[f"p0_{k}"] = sd0[k].detach().reshape(-1)[:NSLICE].numpy().copy()
    assert sorted(os.listdir(tmp))[:1], "the reference saved nothing"
    return out


def lsm_vectors():
    class D:
        num_timesteps = 50
    s = LossSecondMomentResampler(D())
    rng = np.random.RandomState(5)
    ts, losses = [], []
    while not s._warmed_up():
        t = rng.randint(0, 50, size=8)
        l = rng.rand(8) * (1 + t / 10.0)
        ts.append(t)
        losses.append(l)
        s.update_with_all_losses(t.tolist(), l.tolist())
    for _ in range(7):                                 # past the warm-up: the history shifts
        t = rng.randint(0, 50, size=8)
        l = rng.rand(8)
        ts.append(t)
        losses.append(l)
        s.update_with_all_losses(t.tolist(), l.tolist())
    np.random.seed(3)
    idx, w = s.sample(16, "cpu")
    return dict(lsm_ts=np.concatenate(ts), lsm_losses=np.concatenate(losses), lsm_weights=s.weights(), lsm_draw_t=idx.numpy(),
                lsm_draw_w=w.numpy())


if __name__ == "__main__":
    torch.set_num_threads(8)
    tmp = tempfile.mkdtemp()
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "pg"), rank=0, world_size=1)
    res = {}
    for i, wd in enumerate(WDS):
        d = os.path.join(tmp, f"wd{i}")
        os.makedirs(d)
        os.environ["DIFFUSION_BLOB_LOGDIR"] = d
        logger.configure(dir=d)
        for k, v in run_case(wd, d).items():
            res[f"wd{i}_{k}"] = v
        print("wd", wd, "grad_norm", res[f"wd{i}_grad_norm"], "loss", res[f"wd{i}_loss"].mean(axis=1))
    res.update(lsm_vectors())
    res["wds"] = np.array(WDS)
    np.savez_compressed(os.path.join(HERE, "train_loop_tiny32.npz"), **res)
    dist.destroy_process_group()
