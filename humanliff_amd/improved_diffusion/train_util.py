"""The diffusion training loop (human_diffusion/improved_diffusion/train_util.py TrainLoop) on the HIP training path, with the step's
tail - grad norm, clip_grad_value_(0.5), AdamW, EMA - in one fused launch (humanliff_amd.optim.FusedAdamW, csrc/hl_optim.hip).

Same constructor, checkpoints and logged keys as the reference, and the reference's behaviour where it is surprising (DESIGN.md
"Training loop" lists them): use_amp=True backpropagates the loss times GradScaler's initial scale 2^16 and never unscales it (the
reference's run_step calls optimize_normal; optimize_amp is dead code), so grad_norm is logged scaled and the clip acts on the scaled
gradients.  What differs is the plumbing:
  - no blobfile / logger / dist_util: checkpoints and progress.csv go to `log_dir` (keyword; else $DIFFUSION_BLOB_LOGDIR, else a new
    directory under the system's temp dir), the device is the model's;
  - the logged values are accumulated on the device and read back once per log_interval (the reference reads ~950 norms and every
    loss key back each step);
  - DDP (RCCL) wraps the model only when a process group with more than one rank is initialised; a world of one trains the bare model.
"""
import csv
import datetime
import os
import tempfile

import numpy as np
import torch as th
import torch.distributed as dist

from ..optim import FusedAdamW
from .resample import LossAwareSampler, UniformSampler

AMP_LOSS_SCALE = 65536.0         # torch.cuda.amp.GradScaler's init_scale: the factor the reference's use_amp path backpropagates
ANNEAL_STEPS = 100000            # _anneal_lr: lr goes linearly from `lr` to ANNEAL_LR_END over the first ANNEAL_STEPS global steps
ANNEAL_LR_END = 1e-5
CLIP_VALUE = 0.5                 # optimize_normal's clip_grad_value_


def _dist_on():
    return dist.is_available() and dist.is_initialized()


def _rank():
    return dist.get_rank() if _dist_on() else 0


def _world():
    return dist.get_world_size() if _dist_on() else 1


class DeviceLog:
    """logger.logkv_mean / logkv / dumpkvs of the reference with the means kept on the device: one host read per dump."""

    def __init__(self, log_dir, device):
        self.dir = log_dir
        self.device = device
        self._sums = {}           # key -> fp64 device tensor (sum, count); count on the device too (quartile counts depend on t)
        self._host = {}           # key -> value known on the host (logkv)
        self._csv_keys = []
        self.last = {}

    def mean(self, key, values, counts=None):
        """Add values (device tensor, any shape, summed) with counts (device, same shape; default 1 each) to key's running mean."""
        v = values.detach().double().reshape(-1)
        c = th.ones_like(v) if counts is None else counts.double().reshape(-1)
        acc = self._sums.get(key)
        if acc is None:
            acc = self._sums[key] = th.zeros(2, dtype=th.float64, device=self.device)
        acc[0] += v.sum()
        acc[1] += c.sum()

    def kv(self, key, value):
        self._host[key] = value

    def dump(self):
        keys = sorted(self._sums)
        out = dict(self._host)
        if keys:
            vals = th.stack([self._sums[k] for k in keys]).cpu().numpy()     # the one host read of the interval
            for k, (s, c) in zip(keys, vals):
                if c > 0:
                    out[k] = s / c
        self._sums.clear()
        self._host.clear()
        self.last = out
        if _rank() == 0:
            self._write(out)
        return out

    def _write(self, kvs):
        lines = [f"| {k:<20} | {('%-8.3g' % v) if isinstance(v, (float, np.floating)) else str(v):<10} |" for k, v in sorted(kvs.items())]
        if lines:
            bar = "-" * max(len(s) for s in lines)
            print("\n".join([bar] + lines + [bar]), flush=True)
        path = os.path.join(self.dir, "progress.csv")
        new = [k for k in sorted(kvs) if k not in self._csv_keys]
        if new:                                                             # new keys: rewrite the file with the wider header
            rows = []
            if os.path.exists(path) and self._csv_keys:
                with open(path) as f:
                    rows = list(csv.reader(f))[1:]
            self._csv_keys += new
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(self._csv_keys)
                for r in rows:
                    w.writerow(r + [""] * (len(self._csv_keys) - len(r)))
        with open(path, "a", newline="") as f:
            csv.writer(f).writerow([kvs.get(k, "") for k in self._csv_keys])


class TrainLoop:
    def __init__(self, *, model, diffusion, data, batch_size, microbatch, lr, ema_rate, log_interval, save_interval, resume_checkpoint,
                 use_fp16=False, fp16_scale_growth=1e-3, use_amp=False, schedule_sampler=None, weight_decay=0.0, lr_anneal_steps=0,
                 use_cond=False, writer=None, log_dir=None):
        if use_fp16:
            raise NotImplementedError("use_fp16 (convert_to_fp16 master parameters) is not supported on the HIP training path: "
                                      "train with use_amp=True, which runs the UNet's training kernels in reduced precision")
        self.model = model
        self.diffusion = diffusion
        self.data = data
        self.batch_size = batch_size
        self.microbatch = microbatch if microbatch > 0 else batch_size
        self.lr = lr
        self.ema_rate = [ema_rate] if isinstance(ema_rate, float) else [float(x) for x in str(ema_rate).split(",")]
        self.log_interval = log_interval
        self.save_interval = save_interval
        self.resume_checkpoint = resume_checkpoint
        self.use_fp16 = use_fp16
        self.use_amp = use_amp
        self.fp16_scale_growth = fp16_scale_growth
        self.schedule_sampler = schedule_sampler or UniformSampler(diffusion)
        self.weight_decay = weight_decay
        self.lr_anneal_steps = lr_anneal_steps
        self.use_cond = use_cond
        self.writer = writer
        self.log_dir = log_dir or os.environ.get("DIFFUSION_BLOB_LOGDIR") or os.path.join(
            tempfile.gettempdir(), datetime.datetime.now().strftime("humanliff-%Y-%m-%d-%H-%M-%S-%f"))
        os.makedirs(self.log_dir, exist_ok=True)

        self.step = 0
        self.resume_step = 0
        self.global_batch = self.batch_size * _world()
        self.device = next(self.model.parameters()).device
        self.model_params = list(self.model.parameters())
        self.master_params = self.model_params
        self.log = DeviceLog(self.log_dir, self.device)

        self._load_and_sync_parameters()
        self.opt = FusedAdamW(self.master_params, lr=self.lr, weight_decay=self.weight_decay)
        if self.resume_step:
            self._load_optimizer_state()
            self.ema_params = [self._load_ema_parameters(rate) for rate in self.ema_rate]
        else:
            self.ema_params = [[p.detach().clone() for p in self.master_params] for _ in self.ema_rate]
        self.opt.attach_ema(self.ema_params, self.ema_rate)

        if _world() > 1:
            from torch.nn.parallel.distributed import DistributedDataParallel as DDP
            self.use_ddp = True
            self.ddp_model = DDP(self.model, device_ids=[self.device], output_device=self.device, broadcast_buffers=False,
                                 bucket_cap_mb=128, find_unused_parameters=False)
        else:
            self.use_ddp = False
            self.ddp_model = self.model

    # ---- checkpoints ------------------------------------------------------------------------------------------------------------
    def _sync(self, tensors):
        if _world() > 1:
            for t in tensors:
                with th.no_grad():
                    dist.broadcast(t, 0)

    def _load_and_sync_parameters(self):
        ckpt = self.resume_checkpoint
        if ckpt:
            self.resume_step = parse_resume_step_from_filename(ckpt)
            if _rank() == 0:
                print(f"loading model from checkpoint: {ckpt}...", flush=True)
                self.model.load_state_dict(th.load(ckpt, map_location=self.device))
        self._sync(self.model.parameters())

    def _load_ema_parameters(self, rate):
        ema = [p.detach().clone() for p in self.master_params]
        path = find_ema_checkpoint(self.resume_checkpoint, self.resume_step, rate)
        if path and _rank() == 0:
            print(f"loading EMA from checkpoint: {path}...", flush=True)
            sd = th.load(path, map_location=self.device)
            ema = [sd[name].detach().clone().contiguous() for name, _ in self.model.named_parameters()]
        self._sync(ema)
        return ema

    def _load_optimizer_state(self):
        path = os.path.join(os.path.dirname(self.resume_checkpoint), f"opt{self.resume_step:06}.pt")
        if os.path.exists(path):
            print(f"loading optimizer state from checkpoint: {path}", flush=True)
            self.opt.load_state_dict(th.load(path, map_location=self.device))

    def _params_to_state_dict(self, params):
        sd = self.model.state_dict()
        for (name, _), p in zip(self.model.named_parameters(), params):
            assert name in sd
            sd[name] = p
        return sd

    def save(self):
        step = self.step + self.resume_step
        if _rank() == 0:
            print(f"saving model 0...", flush=True)
            th.save(self._params_to_state_dict(self.master_params), os.path.join(self.log_dir, f"model{step:06d}.pt"))
            for rate, params in zip(self.ema_rate, self.ema_params):
                print(f"saving model {rate}...", flush=True)
                th.save(self._params_to_state_dict(params), os.path.join(self.log_dir, f"ema_{rate}_{step:06d}.pt"))
            th.save(self.opt.state_dict(), os.path.join(self.log_dir, f"opt{step:06d}.pt"))
        if _dist_on():
            dist.barrier()

    # ---- the loop ---------------------------------------------------------------------------------------------------------------
    def run_loop(self):
        while not self.lr_anneal_steps or self.step + self.resume_step < self.lr_anneal_steps:
            batch, layer_condition, cond = next(self.data)
            self.run_step(batch, layer_condition, cond)
            if self.step % self.log_interval == 0:
                self.log.dump()
            if self.step % self.save_interval == 0 or self.step == 20000:
                self.save()
                if os.environ.get("DIFFUSION_TRAINING_TEST", "") and self.step > 0:
                    return
            self.step += 1
        if (self.step - 1) % self.save_interval != 0:
            self.save()

    def run_step(self, batch, layer_condition, cond):
        self.forward_backward(batch, layer_condition, cond)
        self.optimize_normal()
        self.log_step()

    def _zero_grad(self):
        for p in self.model_params:                          # in place, as fp16_util.zero_grad: the gradient buffers (and so the
            if p.grad is not None:                           # optimizer's table) stay where they are
                p.grad.detach_()
                p.grad.zero_()

    def forward_backward(self, batch, layer_condition, cond):
        self._zero_grad()
        dev = self.device
        loss = None
        for i in range(0, batch.shape[0], self.microbatch):
            micro = batch[i:i + self.microbatch].to(dev)
            micro_lc = layer_condition[i:i + self.microbatch].to(dev) if self.use_cond else None
            micro_cond = {k: v[i:i + self.microbatch].to(dev) for k, v in cond.items()}
            last = (i + self.microbatch) >= batch.shape[0]
            t, weights = self.schedule_sampler.sample(micro.shape[0], dev)
            with th.autocast("cuda", dtype=th.float16, enabled=self.use_amp):
                if last or not self.use_ddp:
                    losses = self.diffusion.training_losses(self.ddp_model, micro, micro_lc, t, model_kwargs=micro_cond)
                else:
                    with self.ddp_model.no_sync():
                        losses = self.diffusion.training_losses(self.ddp_model, micro, micro_lc, t, model_kwargs=micro_cond)
                if isinstance(self.schedule_sampler, LossAwareSampler):
                    self.schedule_sampler.update_with_local_losses(t, losses["loss"].detach())
                loss = (losses["loss"] * weights).mean()
                self._log_loss_dict(t, {k: v * weights for k, v in losses.items()})
            if self.use_amp:
                (loss * AMP_LOSS_SCALE).backward()            # GradScaler.scale(loss) at its initial scale; never unscaled
            else:
                loss.backward()
        if self.writer is not None and (self.step + self.resume_step) % 100 == 0 and _rank() == 0:
            self.writer.add_scalar("loss", loss.item(), self.step + self.resume_step)

    def _log_loss_dict(self, ts, losses):
        """log_loss_dict: the mean of every key per microbatch, and per sample into the quartile of its timestep - on the device."""
        q = (4 * ts // self.diffusion.num_timesteps).clamp(0, 3)
        onehot = (q[:, None] == th.arange(4, device=ts.device)[None]).double()
        for key, values in losses.items():
            v = values.detach().double()
            self.log.mean(key, v.mean())
            qs, qc = onehot.t() @ v, onehot.sum(0)
            for j in range(4):
                self.log.mean(f"{key}_q{j}", qs[j], qc[j])

    def optimize_normal(self):
        # grad norm (unclipped), _anneal_lr, clip_grad_value_(0.5), AdamW, EMA: _anneal_lr sets the lr the fused step reads
        self._anneal_lr()
        self.opt.step(clip_value=CLIP_VALUE)
        self.log.mean("grad_norm", self.opt.grad_sqsum.sqrt())

    def _anneal_lr(self):
        s = self.step + self.resume_step
        if s < ANNEAL_STEPS:
            frac = (ANNEAL_STEPS - s) / ANNEAL_STEPS
            lr = ANNEAL_LR_END + (self.lr - ANNEAL_LR_END) * frac
            for g in self.opt.param_groups:
                g["lr"] = lr

    def log_step(self):
        self.log.kv("step", self.step + self.resume_step)
        self.log.kv("samples", (self.step + self.resume_step + 1) * self.global_batch)


def parse_resume_step_from_filename(filename):
    """path/to/modelNNNNNN.pt -> NNNNNN (0 if the name does not have that form)."""
    parts = filename.split("model")
    if len(parts) < 2:
        return 0
    try:
        return int(parts[-1].split(".")[0])
    except ValueError:
        return 0


def find_ema_checkpoint(main_checkpoint, step, rate):
    if not main_checkpoint:
        return None
    path = os.path.join(os.path.dirname(main_checkpoint), f"ema_{rate}_{step:06d}.pt")
    return path if os.path.exists(path) else None


def checkpoint_names(step, rates):
    """The files save() writes at global step `step`."""
    return [f"model{step:06d}.pt"] + [f"ema_{r}_{step:06d}.pt" for r in rates] + [f"opt{step:06d}.pt"]
