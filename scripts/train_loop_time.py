"""The training step's tail on the production net (bench.py's F4 UNet, 497 M parameters): the reference's eager tail against FusedAdamW.

    python scripts/train_loop_time.py [--tail-iters N] [--repeats R] [--loop-steps S] [--skip-loop] [--tail-only fused|eager]

1. tail alone: the reference-equivalent eager tail - per-tensor (p.grad ** 2).sum().item(), clip_grad_value_(0.5), torch AdamW
   (foreach, torch's default on the device), update_ema per tensor - against FusedAdamW.step(clip_value=0.5) with one EMA rate.
   Device events around N steps after a warm-up, R repeats: median / min / max ms per step.
2. a whole TrainLoop step at batch 8, microbatch 2, use_amp=True, against the same loop with the eager tail (wall time per step,
   torch.cuda.synchronize() at both ends of S steps after two warm-up steps).
--tail-only runs only that tail (for a rocprofv3 --kernel-trace --stats run).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_legs import build_unet  # noqa: E402
from humanliff_amd.improved_diffusion import train_util  # noqa: E402
from humanliff_amd.improved_diffusion.nn import update_ema  # noqa: E402
from humanliff_amd.optim import FusedAdamW  # noqa: E402

BYTES_PER_PARAM_1EMA = 36      # reads g, p, m, v, e (20 B), writes p, m, v, e (16 B)


class EagerTail:
    """train_util.py optimize_normal as the reference runs it on this stack (grad norm with one host read per tensor)."""

    def __init__(self, params, rates, lr=1e-4, wd=0.0):
        self.params = params
        self.rates = rates
        self.opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd)
        self.ema = [[p.detach().clone() for p in params] for _ in rates]
        self.last_norm = None

    def step(self):
        sq = 0.0
        for p in self.params:
            sq += (p.grad ** 2).sum().item()
        self.last_norm = float(np.sqrt(sq))
        torch.nn.utils.clip_grad_value_(self.params, 0.5)
        self.opt.step()
        for r, el in zip(self.rates, self.ema):
            update_ema(el, self.params, rate=r)


def time_tail(kind, params, iters, repeats, warm=3):
    if kind == "fused":
        opt = FusedAdamW(params, lr=1e-4, weight_decay=0.0)
        opt.attach_ema([[p.detach().clone() for p in params]], [0.9999])
        fn = lambda: opt.step(clip_value=0.5)   # noqa: E731
    else:
        tail = EagerTail(params, [0.9999])
        fn = tail.step
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) / iters)
    return res


class EagerLoop(train_util.TrainLoop):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.eager = EagerTail(self.master_params, self.ema_rate, lr=self.lr, wd=self.weight_decay)

    def optimize_normal(self):
        self._anneal_lr()
        for g in self.eager.opt.param_groups:
            g["lr"] = self.opt.param_groups[0]["lr"]
        self.eager.step()
        self.log.kv("grad_norm", self.eager.last_norm)


def time_loop(cls, dev, steps):
    model, diffusion, _ = build_unet(dev)
    model.train()
    g = torch.Generator().manual_seed(0)

    def data():
        while True:
            x = torch.randn((8, 27, 256, 256), generator=g).clamp(-1, 1)
            c = torch.randn((8, 27, 256, 256), generator=g).clamp(-1, 1) * 0.7
            yield x, c, {"y": torch.randint(0, 4, (8,), generator=g)}

    import tempfile
    loop = cls(model=model, diffusion=diffusion, data=data(), batch_size=8, microbatch=2, lr=1e-4, ema_rate="0.9999", log_interval=10 ** 9,
               save_interval=10 ** 9, resume_checkpoint="", use_amp=True, use_cond=True, log_dir=tempfile.mkdtemp())
    it = loop.data
    for _ in range(2):
        loop.run_step(*next(it))
        loop.step += 1
    torch.cuda.synchronize()
    batches = [next(it) for _ in range(steps)]
    t0 = time.perf_counter()
    for b in batches:
        loop.run_step(*b)
        loop.step += 1
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    del loop, model
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=5)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--tail-only", choices=["fused", "eager"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, _ = build_unet(dev)
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    gg = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gg) * 0.3
    out = dict(params=n, tensors=len(params), bytes_1ema=n * BYTES_PER_PARAM_1EMA)
    kinds = [a.tail_only] if a.tail_only else ["fused", "eager"]
    for kind in kinds:
        r = time_tail(kind, params, a.tail_iters if kind == "fused" else max(2, a.tail_iters // 4), a.repeats)
        out[f"tail_{kind}_ms"] = dict(median=statistics.median(r), min=min(r), max=max(r), repeats=r)
    if "tail_fused_ms" in out:
        out["fused_TBps"] = n * BYTES_PER_PARAM_1EMA / (out["tail_fused_ms"]["median"] * 1e-3) / 1e12
    del model, params
    torch.cuda.empty_cache()
    if not a.skip_loop and not a.tail_only:
        out["loop_step_fused_ms"] = time_loop(train_util.TrainLoop, dev, a.loop_steps)
        out["loop_step_eager_ms"] = time_loop(EagerLoop, dev, a.loop_steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
