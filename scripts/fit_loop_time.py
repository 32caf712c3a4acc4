"""Times one tri-plane fitting iteration and its tail (everything after the render backward) at the reference's configurations:

    main  num_instances 100, 256 x 256 x 27 planes, batch 2 x 2048 rays x 128+128 samples, tv 1e-2, l1 5e-4, clamp on
    ft    run_nerf_batch_ft.py: num_instances 1, batch 8, frozen decoder (--ft_triplane_only --lrate 0)

in two modes, both in this one process: FitLoop (hl_fit_reg + hl_fit_adam_planes) and --torch-tail's code path, the loop INTEGRATION.md
prescribed before FitLoop (the same HIP render forward / backward, torch TV / L1, torch.optim.Adam(fused=True), clamp_, zero_grad).
HIP events around every iteration; FitLoop's tail also between its own events.  For both modes the tail is ALSO given as the whole
iteration minus a render-only iteration (forward + backward into the gathered leaf, no optimizer) measured in the same process: the
torch loop's tail is interleaved with its backward (the dense gradient is materialised inside loss.backward()) and has no other
boundary.  Prints one JSON line per (configuration, mode) and a markdown table.

    python scripts/fit_loop_time.py [--config main|ft|both] [--mode both|fused|torch-tail] [--torch-tail] [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from humanliff_amd import synthetic as syn                                  # noqa: E402
from humanliff_amd.NeRF.renderer import render as nerf_render               # noqa: E402
from humanliff_amd.recon_NeRF import Renderer, render                       # noqa: E402
from humanliff_amd.recon_NeRF.fit import FitLoop, split_parameters          # noqa: E402
from humanliff_amd.recon_NeRF.run_nerf_batch import _Bare                   # noqa: E402

CONFIGS = {"main": dict(num_instances=100, bs=2, ft=False, lrate=5e-4), "ft": dict(num_instances=1, bs=8, ft=True, lrate=0.0)}
KW = dict(tri_plane_lrate=1e-1, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4, use_clamp=True, n_samples=128, n_importance=128,
          perturb=1., chunk=1024 * 64)


def make_model(cfg, dev):
    torch.manual_seed(0)
    m = Renderer(use_canonical_space=False, num_instances=1, triplane_dim=256, triplane_ch=27, test=False)
    m.load_state_dict(syn.render_mlp_state(3), strict=False)
    m = m.to(dev)
    m.tri_planes = torch.nn.Parameter(0.1 * torch.randn((cfg["num_instances"], 4, 3, 9, 256, 256), device=dev))   # (N(0, 0.1) like the module's init, drawn on the device)
    return m


def timed(fn, warmup, iters, mid=None):
    """ms per call (mean of per-iteration HIP event times), and from `mid` (an event fn records) to the end when given."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, m, b in ev:
        a.record()
        fn(m) if mid else fn()
        b.record()
    torch.cuda.synchronize()
    whole = sum(a.elapsed_time(b) for a, _, b in ev) / iters
    tail = sum(m.elapsed_time(b) for _, m, b in ev) / iters if mid else None
    return whole, tail


def render_only(model, tps, cfg):
    it = [0]

    def fn():
        tp = tps[it[0] % len(tps)]
        it[0] += 1
        planes = model.tri_planes.detach()[tp['instance_idx'], tp['cloth_layer_index']].requires_grad_(True)
        rgb, acc, _, _ = nerf_render(chunk=KW["chunk"], rays_o=tp['ray_o_all'][:, 0], rays_d=tp['ray_d_all'][:, 0], near=tp['near_all'][:, 0],
                                     far=tp['far_all'][:, 0], tri_planes=planes, tp_input=tp, renderer=_Bare(model), n_samples=KW["n_samples"],
                                     perturb=KW["perturb"], n_importance=KW["n_importance"])
        (torch.mean((rgb - tp['rgb_all'][:, 0]) ** 2) + 0.1 * torch.mean((tp['bkgd_msk_all'][:, 0].squeeze(2) - acc) ** 2)).backward()
        for p in model.parameters():
            p.grad = None
    return fn


def run_fused(cfg, tps, dev, warmup, iters):
    model = make_model(cfg, dev)
    loop = FitLoop(model, tps, lrate=cfg["lrate"], ft_triplane_only=cfg["ft"], **KW)
    it = [0]

    def fn(mid=None):
        loop.tail_event = mid
        loop.step(tps[it[0] % len(tps)])
        it[0] += 1
    torch.cuda.reset_peak_memory_stats(dev)
    whole, tail = timed(fn, warmup, iters, mid=True)
    peak = torch.cuda.max_memory_allocated(dev)
    loop.tail_event = None
    ronly, _ = timed(render_only(model, tps, cfg), warmup, iters)
    return dict(ms_per_iteration=whole, tail_ms_events=tail, render_only_ms=ronly, tail_ms=whole - ronly, peak_allocated_bytes=peak)


def run_torch(cfg, tps, dev, warmup, iters):
    model = make_model(cfg, dev)
    mlp, tri = split_parameters(model)
    if cfg["ft"]:
        for p in mlp:
            p.requires_grad_(False)
    opt = torch.optim.Adam([{'params': mlp, 'lr': cfg["lrate"]}, {'params': [tri], 'lr': KW["tri_plane_lrate"]}], betas=(0.9, 0.999), fused=True)
    it = [0]

    def fn():
        tp = tps[it[0] % len(tps)]
        it[0] += 1
        rgb, acc, _, _ = render(chunk=KW["chunk"], rays_o=tp['ray_o_all'][:, 0], rays_d=tp['ray_d_all'][:, 0], tp_input=tp, near=tp['near_all'][:, 0],
                                far=tp['far_all'][:, 0], renderer=model, n_samples=KW["n_samples"], perturb=KW["perturb"], n_importance=KW["n_importance"])
        ii, ll = tp['instance_idx'], tp['cloth_layer_index']
        img_loss = torch.mean((rgb - tp['rgb_all'][:, 0]) ** 2)
        acc_loss = torch.mean((tp['bkgd_msk_all'][:, 0].squeeze(2) - acc) ** 2)
        tv_loss = F.l1_loss(tri[ii, ll, :, :, 0:-1, :], tri[ii, ll, :, :, 1:, :]) + F.l1_loss(tri[ii, ll, :, :, :, 0:-1], tri[ii, ll, :, :, :, 1:])
        l1_loss = F.l1_loss(tri[ii, ll], torch.zeros_like(tri[ii, ll]))
        loss = img_loss + 0.1 * acc_loss + KW["tv_loss_coef"] * tv_loss + KW["l1_loss_coef"] * l1_loss
        loss.backward()
        opt.step()
        opt.zero_grad()
        tri.data.clamp_(-1.0, 1.0)
    torch.cuda.reset_peak_memory_stats(dev)
    whole, _ = timed(fn, warmup, iters)
    peak = torch.cuda.max_memory_allocated(dev)
    ronly, _ = timed(render_only(model, tps, cfg), warmup, iters)
    return dict(ms_per_iteration=whole, tail_ms_events=None, render_only_ms=ronly, tail_ms=whole - ronly, peak_allocated_bytes=peak)


def algorithmic_bytes(cfg):
    """What the fused tail has to move: p, m, v read and written over the whole parameter, the selected entries' gradient read by the Adam
    launch, and hl_fit_reg's read of the planes plus read and write of the gradient.  The torch tail's count adds the dense gradient
    (zero fill, scatter, Adam's read, zero_grad is set_to_none), clamp_'s read and write and the regularisers' temporaries."""
    slice_b = 27 * 256 * 256 * 4
    param = cfg["num_instances"] * 4 * slice_b
    fused = 6 * param + cfg["bs"] * slice_b + 3 * cfg["bs"] * slice_b
    torch_tail = 6 * param + 2 * param + param + 2 * param + 30 * cfg["bs"] * slice_b
    return fused, torch_tail


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--config", default="both", choices=["main", "ft", "both"])
    a.add_argument("--mode", default="both", choices=["both", "fused", "torch-tail"])
    a.add_argument("--torch-tail", action="store_true", help="the same as --mode torch-tail")
    a.add_argument("--iters", type=int, default=30)
    a.add_argument("--warmup", type=int, default=5)
    args = a.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_loop_time.py needs a HIP device")
    dev = torch.device("cuda", torch.cuda.current_device())
    modes = ["torch-tail"] if args.torch_tail else (["fused", "torch-tail"] if args.mode == "both" else [args.mode])
    rows = []
    for name in (["main", "ft"] if args.config == "both" else [args.config]):
        cfg = CONFIGS[name]
        tps = [{k: v.to(dev) for k, v in syn.fit_batch(cfg["bs"], 2048, cfg["num_instances"], seed=100 + i).items()} for i in range(4)]
        fused_b, torch_b = algorithmic_bytes(cfg)
        for mode in modes:
            r = (run_fused if mode == "fused" else run_torch)(cfg, tps, dev, args.warmup, args.iters)
            torch.cuda.empty_cache()
            r.update(config=name, mode=mode, iters=args.iters, algorithmic_bytes=fused_b if mode == "fused" else torch_b)
            r["tail_GBps"] = r["algorithmic_bytes"] / (r["tail_ms"] * 1e-3) / 1e9
            rows.append(r)
            print(json.dumps(r), flush=True)
    print("| config | mode | ms / iteration | render only ms | tail ms (whole - render) | tail ms (events) | algorithmic GB | tail GB/s | peak allocated GB |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        ev = "-" if r["tail_ms_events"] is None else f"{r['tail_ms_events']:.3f}"
        print(f"| {r['config']} | {r['mode']} | {r['ms_per_iteration']:.3f} | {r['render_only_ms']:.3f} | {r['tail_ms']:.3f} | {ev} | "
              f"{r['algorithmic_bytes'] / 1e9:.2f} | {r['tail_GBps']:.0f} | {r['peak_allocated_bytes'] / 1e9:.2f} |")


if __name__ == "__main__":
    main()
