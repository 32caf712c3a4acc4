"""Training step of the 3-D-aware and cross-attention UNets at production width (the F4 network of bench.py: 192 channels, 3 ResBlocks
per level, attention at 32 / 16 / 8, class-conditional), microbatch 2: GaussianDiffusion.training_losses -> backward -> fused AdamW step.

    python scripts/unet_train_variants_time.py [--net aware3d|xattn ...] [--impl hip|twin ...] [--arith fp32|bf16 ...] [--iters N]

  aware3d  use_3d_aware=True, cond_type='controlnet', 9-channel planes: the network runs at 256 x 768
  xattn    cond_type='cross_attention' at 256 x 256 (SpatialTransformer blocks, one context token per image)
  hip      the HIP training path (unet_train.py);  twin: the PyTorch-op twin (tests/unet_autograd_twin.py) on MIOpen / rocBLAS
  fp32     plain fp32;  bf16: the step under torch.autocast(bfloat16) (the HIP convolutions take bf16 operands where they do)
Prints one JSON line per combination: ms per step (median over --iters after one warm-up step), peak memory."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_legs import F4  # noqa: E402

NETS = {"aware3d": dict(in_channels=9, out_channels=9, use_3d_aware=True, cond_type="controlnet"),
        "xattn": dict(cond_type="cross_attention")}


def build(net, dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion
    a = dict(F4)
    a.update(NETS[net])
    model, diffusion = create_model_and_diffusion(**a)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(syn.state_from_shapes(keys, seed=1))
    return model.to(dev).train(), diffusion


def time_step(net, impl, arith, iters, dev):
    model, diffusion = build(net, dev)
    B = 2
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.randn((B, 27, 256, 256), device=dev, generator=g).clamp(-1, 1)
    xc = torch.randn((B, 27, 256, 256), device=dev, generator=g).clamp(-1, 1) * 0.7
    y = torch.zeros((B,), dtype=torch.int64, device=dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.0, fused=True)
    fwd = model
    if impl == "twin":
        import functools
        from tests.unet_autograd_twin import forward_autograd
        fwd = functools.partial(forward_autograd, model)

    def step():
        t = torch.randint(0, 1000, (B,), device=dev, generator=g)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=arith == "bf16"):
            loss = diffusion.training_losses(fwd, x0, xc, t, model_kwargs={"y": y})["loss"].mean()
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    return {"net": net, "impl": impl, "arith": arith, "batch": B, "ms_per_step": round(times[len(times) // 2] * 1e3, 2),
            "ms_min": round(times[0] * 1e3, 2), "iters": iters, "loss": round(float(loss), 5),
            "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", nargs="+", default=["aware3d", "xattn"], choices=list(NETS))
    ap.add_argument("--impl", nargs="+", default=["hip", "twin"], choices=["hip", "twin"])
    ap.add_argument("--arith", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for net in args.net:
        for impl in args.impl:
            for arith in args.arith:
                print(json.dumps(time_step(net, impl, arith, args.iters, dev)), flush=True)
                torch.cuda.empty_cache()
