"""Seeded inputs shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: a smooth ground truth, a prediction that is the ground
truth plus clipped noise (both float32), and a mask that is a rectangle with random holes and its two corners forced on - or a
one-pixel-wide diagonal line - so that its bounding rectangle is known.  The restatement's results and its own summation-order noise are
computed once per process and shared."""
import functools

import numpy as np

from tests import metrics_restatement as mr

# name: (H, W, box (h, w, y, x) or "full" / "diagonal")
CASES = {
    "7x7": (37, 53, (7, 7, 5, 11)),               # one interior position
    "8x7": (37, 53, (8, 7, 5, 11)),
    "23x39": (37, 53, (23, 39, 5, 11)),           # crosses the 16 x 16 tile edges in both axes, ragged
    "borders": (37, 53, (37, 53, 0, 0)),          # the box touches all four image borders
    "full64": (64, 64, "full"),
    "diagonal": (48, 80, "diagonal"),             # a large box almost all of which is masked out
}
SMALL = (37, 53, (6, 9, 5, 11))                   # lower than the window: no SSIM


def images(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    gt = np.stack([0.5 + 0.4 * np.sin(0.21 * xx + 0.13 * yy + c) * np.cos(0.17 * yy - 0.05 * xx * c) for c in range(3)], -1)
    gt = gt.astype(np.float32)
    noise = np.clip(rng.normal(0.0, 0.05, size=gt.shape), -0.15, 0.15).astype(np.float32)
    pred = (gt + noise).astype(np.float32)          # (slightly outside [0, 1] here and there: to8b clips)
    return pred, gt, rng


def make(H, W, box, seed):
    """pred, gt (H, W, 3) float32, mask (H, W) bool, and the bounding rectangle (x, y, w, h) the mask was built to have."""
    pred, gt, rng = images(H, W, seed)
    mask = np.zeros((H, W), dtype=bool)
    if box == "full":
        mask[:] = True
        want = (0, 0, W, H)
    elif box == "diagonal":
        n = min(H, W) - 8
        idx = np.arange(n)
        mask[4 + idx, 3 + idx] = True
        want = (3, 4, n, n)
    else:
        h, w, y, x = box
        mask[y:y + h, x:x + w] = rng.random((h, w)) > 0.25
        mask[y, x] = mask[y + h - 1, x + w - 1] = True
        want = (x, y, w, h)
    return pred, gt, mask, want


@functools.lru_cache(maxsize=None)
def case(name):
    H, W, box = CASES[name]
    pred, gt, mask, want_box = make(H, W, box, seed=1000 + sorted(CASES).index(name))
    for a in (pred, gt, mask):
        a.setflags(write=False)
    return pred, gt, mask, want_box


@functools.lru_cache(maxsize=None)
def reference(name, data_range=2.0):
    """The restatement's record of a case (computed once, read-only)."""
    pred, gt, mask, _ = case(name)
    return mr.view_metrics(pred, gt, mask, data_range)


@functools.lru_cache(maxsize=None)
def ordering_noise():
    """The restatement's own summation-order noise over the cases: SSIM with a cumulative-sum box filter against uniform_filter
    (absolute), and the MSE's pairwise np.mean against a sequential cumulative sum (relative).  Returns (ssim_noise, mse_noise)."""
    ssim_noise, mse_noise = 0.0, 0.0
    for name in CASES:
        pred, gt, mask, _ = case(name)
        other = mr.view_metrics(pred, gt, mask, 2.0, filter_func=mr.box_filter_cumsum)["ssim"]
        ssim_noise = max(ssim_noise, abs(other - reference(name)["ssim"]))
        a, b = mr.masked_values(pred, gt, mask)
        sq = ((a - b).astype(np.float64) ** 2).reshape(-1)
        mse_noise = max(mse_noise, abs(np.cumsum(sq)[-1] / sq.size - reference(name)["mse"]) / reference(name)["mse"])
    return ssim_noise, mse_noise


def device_bounds():
    """(absolute bound on ssim, relative bound on mse) for the device against the restatement: 100 x the restatement's own ordering
    noise - room for another reduction tree and for float64 FMA contraction differences - capped at 1e-10 and 1e-12."""
    ssim_noise, mse_noise = ordering_noise()
    return min(100.0 * ssim_noise, 1e-10), min(100.0 * mse_noise, 1e-12)


def psnr_bound(psnr, mse_rel):
    """psnr = -10 ln(mse) / ln 10: a relative error e of mse moves it by 10 e / ln 10.  On top of that the device's and numpy's ln are
    each good to about an ulp, so the two may differ by 2 ulp of ln(mse); 10 / ln 10 = 4.34 lies in [4, 8), which makes an ulp of
    ln(mse) at most 4.34 / 4 = 1.09 ulp of psnr: 2.2 ulp.  The product and the quotient that follow round once each on values that
    already differ: 2 more.  6 ulp of psnr's magnitude covers it."""
    return 10.0 / np.log(10.0) * mse_rel + 6.0 * np.spacing(abs(psnr))
