"""Times the native LPIPS (humanliff_amd.lpips.LpipsVGG, csrc/hl_lpips.hip) against the hook a user would otherwise pass to
evaluate_views: the same network in float32 on the device through torch's own convolutions.  Seeded random weights.

    python scripts/lpips_time.py [--sizes 512x512 400x200] [--warmup 3] [--reps 20] [--json out.json]

Per size: the median of `reps` runs between stream events after `warmup` runs, for both; the native call's fraction of --peak-tflops
(the fp32 matrix peak bench.py prints) on the 13 convolutions' 612 kFLOP per input pixel per image; and the two scores.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def random_weights(seed, dev):
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for block in BLOCKS:
        for cout in block:
            convs.append(((torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev), ((torch.rand((cout,), generator=g) - 0.5) * 0.1).to(dev)))
            cin = cout
    return convs, [torch.rand((1, b[-1], 1, 1), generator=g).to(dev) for b in BLOCKS]


def torch_hook(convs, lins):
    """LPIPS(net='vgg') from torch's convolutions, float32 on the device: the two images as one batch of two, like the native call."""
    shift, scale = (torch.tensor(v, device=lins[0].device).view(1, 3, 1, 1) for v in (SHIFT, SCALE))

    def norm(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)

    def fn(in0, in1):
        with torch.no_grad():
            x = (torch.stack([in0, in1]) - shift) / scale
            val, it = 0, iter(convs)
            for k, block in enumerate(BLOCKS):
                if k:
                    x = F.max_pool2d(x, 2, 2)
                for _ in block:
                    w, b = next(it)
                    x = F.relu(F.conv2d(x, w, b, padding=1))
                n = norm(x)
                val = val + F.conv2d((n[:1] - n[1:]) ** 2, lins[k]).mean([2, 3], keepdim=True)
        return val
    return fn


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times)


def flops_per_pair(h, w):
    total, cin = 0, 3
    for k, block in enumerate(BLOCKS):
        for cout in block:
            total += 2 * 9 * cin * cout * (h >> k) * (w >> k)
            cin = cout
    return 2 * total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["512x512", "400x200"], help="h x w of the crops")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--peak-tflops", dest="peak", type=float, default=155.0)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd.lpips import LpipsVGG
    dev = torch.device("cuda:0")
    convs, lins = random_weights(1, dev)
    native, hook = LpipsVGG(convs, lins, device=dev), torch_hook(convs, lins)
    rows = []
    for size in a.sizes:
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(h * 10007 + w)
        in0, in1 = torch.rand((3, h, w), generator=g).to(dev), torch.rand((3, h, w), generator=g).to(dev)
        native_ms = median_ms(lambda: native(in0, in1), a.warmup, a.reps)
        hook_ms = median_ms(lambda: hook(in0, in1), a.warmup, a.reps)
        gflop = flops_per_pair(h, w) / 1e9
        row = dict(h=h, w=w, native_ms=round(native_ms, 3), torch_hook_ms=round(hook_ms, 3), conv_gflop_per_pair=round(gflop, 1),
                   native_tflops=round(gflop / native_ms, 1), fraction_of_fp32_matrix_peak=round(gflop / native_ms / a.peak, 3),
                   native_score=float(native(in0, in1)), torch_hook_score=float(hook(in0, in1)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
