"""Times the feature metrics (humanliff_amd.feature_metrics, csrc/hl_feature_metrics.hip) against the same quantities formed with torch's
float64 operations on the device (x.double() @ y.double().T, topk, comparisons; chunked over rows to fit memory).

    python scripts/feature_metrics_time.py [--n 10000] [--dims 2048] [--subsets 100] [--subset-size 1000] [--k 3] [--warmup 2] [--reps 10]
                                           [--json profiles/feature_metrics_time.json]

Seeded random ReLU features, N = M = n.  Per quantity (the default KID, knn_radii, the manifold pass, the whole precision_recall): the
median of `reps` runs between stream events after `warmup` runs, for both; the float64 TFLOP/s each achieves on the nominal work of the
definition (2 D flop per pair: 3 S m^2 pairs for KID, N^2 for the radii, N M for the manifold pass - the native KID forms only the upper
triangle of its two same-set blocks, its rate is still quoted on the nominal pairs); the ratio torch / native; and how far the two
results are apart.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CHUNK = 2048


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


def torch_kid(x, y, xi, yi):
    d, out = x.shape[1], []
    for s in range(xi.shape[0]):
        a, b = x[xi[s]].double(), y[yi[s]].double()
        m = a.shape[0]
        kxx, kyy, kxy = ((p @ q.T / d + 1.0) ** 3 for p, q in ((a, a), (b, b), (a, b)))
        out.append((kxx.sum() - kxx.diagonal().sum()) / (m * (m - 1)) + (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1)) - 2.0 * kxy.sum() / (m * m))
    return torch.stack(out)


def torch_d2(xc, nc, yd, ny):
    return (nc[:, None] + ny[None, :] - 2.0 * (xc.double() @ yd.T)).clamp_min(0.0)


def torch_knn(x, k):
    xd = x.double()
    nx = (xd * xd).sum(1)
    out = []
    for i0 in range(0, x.shape[0], CHUNK):
        dd = torch_d2(x[i0:i0 + CHUNK], nx[i0:i0 + CHUNK], xd, nx)
        r = torch.arange(dd.shape[0], device=x.device)
        dd[r, r + i0] = float("inf")
        out.append(dd.topk(k, dim=1, largest=False).values[:, k - 1])
    return torch.cat(out)


def torch_manifold(real, fake, r2_real, r2_fake):
    fd = fake.double()
    nf, rd = (fd * fd).sum(1), real.double()
    nr = (rd * rd).sum(1)
    hits_fake = torch.zeros(fake.shape[0], dtype=torch.int64, device=real.device)
    hits_real, nearest = [], []
    for i0 in range(0, real.shape[0], CHUNK):
        dd = torch_d2(real[i0:i0 + CHUNK], nr[i0:i0 + CHUNK], fd, nf)
        hits_fake += (dd <= r2_real[i0:i0 + CHUNK, None]).sum(0)
        hits_real.append((dd <= r2_fake[None, :]).sum(1))
        nearest.append(dd.min(1).values)
    return hits_fake, torch.cat(hits_real), torch.cat(nearest)


def torch_prc(real, fake, k):
    r2_real, r2_fake = torch_knn(real, k), torch_knn(fake, k)
    return (r2_real, r2_fake) + torch_manifold(real, fake, r2_real, r2_fake)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    from humanliff_amd import feature_metrics as hm
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    real = (torch.randn((a.n, a.dims), generator=g) + 0.3).clamp_min(0.0).to(dev)
    fake = (1.1 * torch.randn((a.n, a.dims), generator=g) + 0.35).clamp_min(0.0).to(dev)
    n, d, m, s = a.n, a.dims, a.subset_size, a.subsets
    xi, yi = hm.subset_indices(n, n, s, m)
    dxi, dyi = torch.from_numpy(xi.astype(np.int64)).to(dev), torch.from_numpy(yi.astype(np.int64)).to(dev)
    r2_real, r2_fake = hm.knn_radii(real, a.k), hm.knn_radii(fake, a.k)
    rows = []

    def row(name, pairs, native, reference, difference):
        native_ms, torch_ms = median_ms(native, a.warmup, a.reps), median_ms(reference, a.warmup, a.reps)
        flop = 2.0 * d * pairs
        r = dict(quantity=name, n=n, dims=d, native_ms=round(native_ms, 3), torch_ms=round(torch_ms, 3), nominal_gflop=round(flop / 1e9, 1),
                 native_fp64_tflops=round(flop / native_ms / 1e9, 2), torch_fp64_tflops=round(flop / torch_ms / 1e9, 2),
                 torch_over_native=round(torch_ms / native_ms, 3), **difference())
        rows.append(r)
        print(json.dumps(r), flush=True)

    def kid_difference():
        got, want = hm.kid_subsets(real, fake, xi, yi), torch_kid(real, fake, dxi, dyi)
        return dict(subsets=s, subset_size=m, kid_mean=float(got.mean()), max_abs_difference=float((got - want).abs().max()))

    def knn_difference():
        got, want = hm.knn_radii(real, a.k), torch_knn(real, a.k)
        return dict(k=a.k, split=hm._split_of(n, n, 0), max_rel_difference=float(((got - want).abs() / want).max()))

    def manifold_difference():
        got, want = hm.manifold(real, fake, r2_real, r2_fake), torch_manifold(real, fake, r2_real, r2_fake)
        return dict(split=hm._split_of(n, n, 0), hits_fake_unequal=int((got[0] != want[0]).sum()), hits_real_unequal=int((got[1] != want[1]).sum()),
                    nearest_max_rel_difference=float(((got[2] - want[2]).abs() / want[2]).max()))

    def prc_difference():
        p = hm.precision_recall(real, fake, a.k)
        return dict(k=a.k, precision=p["precision"], recall=p["recall"], density=p["density"], coverage=p["coverage"])

    row("kid", 3.0 * s * m * m, lambda: hm.kid_subsets(real, fake, xi, yi), lambda: torch_kid(real, fake, dxi, dyi), kid_difference)
    row("knn_radii", float(n) * n, lambda: hm.knn_radii(real, a.k), lambda: torch_knn(real, a.k), knn_difference)
    row("manifold", float(n) * n, lambda: hm.manifold(real, fake, r2_real, r2_fake), lambda: torch_manifold(real, fake, r2_real, r2_fake),
        manifold_difference)
    row("precision_recall", 3.0 * n * n, lambda: hm.precision_recall(real, fake, a.k), lambda: [t.cpu() for t in torch_prc(real, fake, a.k)[2:]],
        prc_difference)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
