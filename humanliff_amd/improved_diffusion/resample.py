"""Timestep samplers of the training loop (human_diffusion/improved_diffusion/resample.py), on numpy 2 and without a process group.

Same semantics as the reference: `sample` draws t with np.random.choice from p = w / sum(w) and returns the importance weights
1 / (T p_t); LossSecondMomentResampler keeps the last 10 losses per timestep, stays uniform until every timestep has 10, then weights
t by the root mean square of its history, mixed with 0.001 of uniform.  update_with_local_losses all-gathers (t, loss) over the ranks
of the default process group when one is initialised, and treats the process as a world of one otherwise.
"""
from abc import ABC, abstractmethod

import numpy as np
import torch as th
import torch.distributed as dist


def create_named_schedule_sampler(name, diffusion):
    if name == "uniform":
        return UniformSampler(diffusion)
    if name == "loss-second-moment":
        return LossSecondMomentResampler(diffusion)
    raise NotImplementedError(f"unknown schedule sampler: {name}")


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class ScheduleSampler(ABC):
    @abstractmethod
    def weights(self):
        """Unnormalised positive numpy weights, one per diffusion step."""

    def sample(self, batch_size, device):
        """(timesteps int64, importance weights float32) on `device`, importance-sampled from weights()."""
        w = self.weights()
        p = w / np.sum(w)
        idx = np.random.choice(len(p), size=(batch_size,), p=p)
        wts = 1 / (len(p) * p[idx])
        return th.from_numpy(idx).long().to(device), th.from_numpy(wts).float().to(device)


class UniformSampler(ScheduleSampler):
    def __init__(self, diffusion):
        self.diffusion = diffusion
        self._weights = np.ones([diffusion.num_timesteps])

    def weights(self):
        return self._weights


class LossAwareSampler(ScheduleSampler):
    def update_with_local_losses(self, local_ts, local_losses):
        """Gather every rank's (t, loss) pairs - rank order, each rank's batch in order - and hand them to update_with_all_losses, so
        that every rank keeps the same reweighting.  One host read of the losses per call."""
        world = _world()
        if world == 1:
            ts = [int(x) for x in local_ts.tolist()]
            losses = [float(x) for x in local_losses.tolist()]
            self.update_with_all_losses(ts, losses)
            return
        dev = local_ts.device
        sizes = [th.zeros(1, dtype=th.int32, device=dev) for _ in range(world)]
        dist.all_gather(sizes, th.tensor([len(local_ts)], dtype=th.int32, device=dev))
        sizes = [int(s.item()) for s in sizes]
        mx = max(sizes)
        tb = [th.zeros(mx).to(local_ts) for _ in sizes]
        lb = [th.zeros(mx).to(local_losses) for _ in sizes]
        pad_t = th.zeros(mx).to(local_ts)
        pad_t[:len(local_ts)] = local_ts
        pad_l = th.zeros(mx).to(local_losses)
        pad_l[:len(local_losses)] = local_losses
        dist.all_gather(tb, pad_t)
        dist.all_gather(lb, pad_l)
        ts = [int(x) for y, n in zip(tb, sizes) for x in y[:n].tolist()]
        losses = [float(x) for y, n in zip(lb, sizes) for x in y[:n].tolist()]
        self.update_with_all_losses(ts, losses)

    @abstractmethod
    def update_with_all_losses(self, ts, losses):
        """Update the reweighting from every rank's (t, loss) pairs; deterministic, so the ranks stay in step."""


class LossSecondMomentResampler(LossAwareSampler):
    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        self.diffusion = diffusion
        self.history_per_term = history_per_term
        self.uniform_prob = uniform_prob
        self._loss_history = np.zeros([diffusion.num_timesteps, history_per_term], dtype=np.float64)
        self._loss_counts = np.zeros([diffusion.num_timesteps], dtype=np.int64)   # (the reference's np.int: gone in numpy >= 1.24)

    def weights(self):
        if not self._warmed_up():
            return np.ones([self.diffusion.num_timesteps], dtype=np.float64)
        w = np.sqrt(np.mean(self._loss_history ** 2, axis=-1))
        w /= np.sum(w)
        w *= 1 - self.uniform_prob
        w += self.uniform_prob / len(w)
        return w

    def update_with_all_losses(self, ts, losses):
        for t, loss in zip(ts, losses):
            n = self._loss_counts[t]
            if n == self.history_per_term:                 # full: drop the oldest, append
                self._loss_history[t, :-1] = self._loss_history[t, 1:]
                self._loss_history[t, -1] = loss
            else:
                self._loss_history[t, n] = loss
                self._loss_counts[t] += 1

    def _warmed_up(self):
        return (self._loss_counts == self.history_per_term).all()
