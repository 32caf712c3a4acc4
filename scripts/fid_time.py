"""Times the native FID network (humanliff_amd.fid.InceptionFID, csrc/hl_fid.hip) against the same network in float32 on the device
through torch's own convolutions, and the moment update (FidStatistics.update).  Seeded random weights, BatchNorm already folded.

    python scripts/fid_time.py [--batches 1 16 64] [--size 299] [--features 10000] [--warmup 3] [--reps 10] [--json out.json]

Per batch size: the median of `reps` runs between stream events after `warmup` runs, for both, as ms per image; the native call's
fraction of --peak-tflops (the fp32 matrix peak bench.py prints) on the 94 convolutions' FLOP; the largest difference of the two
feature sets.  Then the time of one update of `features` rows of 2048 features.
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


def random_convs(seed, layers):
    g = torch.Generator().manual_seed(seed)
    convs = []
    for _, (cin, cout, kh, kw, *_) in layers:
        convs.append((torch.randn((cout, cin, kh, kw), generator=g) * (2.0 / (cin * kh * kw)) ** 0.5, 0.1 * torch.randn((cout,), generator=g)))
    return convs


def torch_network(layers, convs, dev):
    """pool3 features from torch's convolutions, float32 on the device; the layers are taken in the order of humanliff_amd.fid.LAYERS.
    Returns (forward, flop counter): the counter holds the convolutions' FLOP of the last forward."""
    convs = [(w.to(dev), b.to(dev)) for w, b in convs]
    flop = [0]

    def fn(x):
        it = iter(zip(layers, convs))
        flop[0] = 0

        def c(x):
            (_, d), (w, b) = next(it)
            y = F.relu(F.conv2d(x, w, b, stride=d[4], padding=(d[6], d[7])))
            flop[0] += 2 * w.numel() * y.shape[0] * y.shape[2] * y.shape[3]
            return y

        def avg(x):
            return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

        with torch.no_grad():
            x = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
            x = F.max_pool2d(c(c(c(x))), 3, 2)
            x = F.max_pool2d(c(c(x)), 3, 2)
            for _ in range(3):
                x = torch.cat([c(x), c(c(x)), c(c(c(x))), c(avg(x))], 1)
            x = torch.cat([c(x), c(c(c(x))), F.max_pool2d(x, 3, 2)], 1)
            for _ in range(4):
                x = torch.cat([c(x), c(c(c(x))), c(c(c(c(c(x))))), c(avg(x))], 1)
            x = torch.cat([c(c(x)), c(c(c(c(x)))), F.max_pool2d(x, 3, 2)], 1)
            for last in (False, True):
                b1, t = c(x), c(x)
                b3 = torch.cat([c(t), c(t)], 1)
                t = c(c(x))
                bd = torch.cat([c(t), c(t)], 1)
                x = torch.cat([b1, b3, bd, c(F.max_pool2d(x, 3, 1, 1) if last else avg(x))], 1)
            return x.mean([2, 3])
    return fn, flop


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", type=int, default=[1, 16, 64])
    ap.add_argument("--size", type=int, default=299)
    ap.add_argument("--features", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--peak-tflops", dest="peak", type=float, default=155.0)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd.fid import DIMS, LAYERS, FidStatistics, InceptionFID
    dev = torch.device("cuda:0")
    convs = random_convs(1, LAYERS)
    native = InceptionFID(convs, dev)
    hook, flop = torch_network(LAYERS, convs, dev)
    rows = []
    for n in a.batches:
        g = torch.Generator().manual_seed(n)
        x = torch.rand((n, 3, a.size, a.size), generator=g).to(dev)
        native_ms = median_ms(lambda: native(x), a.warmup, a.reps)
        hook_ms = median_ms(lambda: hook(x), a.warmup, a.reps)
        got, want = native(x), hook(x)
        gflop = flop[0] / 1e9
        row = dict(batch=n, size=a.size, native_ms_per_image=round(native_ms / n, 3), torch_ms_per_image=round(hook_ms / n, 3),
                   conv_gflop_per_image=round(gflop / n, 2), native_tflops=round(gflop / native_ms, 1),
                   fraction_of_fp32_matrix_peak=round(gflop / native_ms / a.peak, 3),
                   max_abs_difference=float((got - want).abs().max()), max_abs_feature=float(want.abs().max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    feats = torch.rand((a.features, DIMS), generator=torch.Generator().manual_seed(2)).to(dev)
    stats = FidStatistics(dev)
    update_ms = median_ms(lambda: stats.update(feats), 1, max(3, a.reps // 2))
    finalize_ms = median_ms(stats.finalize, 1, 3)
    row = dict(moment_update_features=a.features, update_ms=round(update_ms, 3), update_fp64_tflops=round(2.0 * a.features * DIMS * (DIMS + 64) / 2 / update_ms / 1e9, 2),
               finalize_ms=round(finalize_ms, 3))
    rows.append(row)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
