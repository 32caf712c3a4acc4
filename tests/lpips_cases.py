"""Seeded weights, inputs, references and bounds shared by tests/test_lpips_cpu.py and tests/test_lpips_gpu.py.

Weights: convolutions N(0, 2 / (9 Cin)), biases uniform +-0.05, lin_k uniform [0, 1), one fixed generator seed; float32 values (the
float64 reference uses the same values, widened).  Each case's pair is two independent uniform [0, 1) images, so every tap
contributes (the CPU test asserts that each of the five terms is at least 2 % of the total on the float64 restatement).

Bounds: the device may differ from the float64 restatement by a small multiple of what the same restatement run in float32 on the
CPU - the arithmetic of the `lpips` package itself - differs from it, pooled (the largest) over all cases.  Both are exact-fp32
evaluations that differ only in summation order.  The constants below are the device's bounds: 3.5 x the pooled float32-CPU figures
measured with

    python -c "from tests import lpips_cases as lc; print(lc.float32_noise())"

and rounded to two digits.  The device is allowed at most 4 x the pooled figure; tests/test_lpips_cpu.py recomputes the figures and
asserts figure <= constant <= 4 x figure, and 3.5 leaves that window a margin on both sides for another CPU's summation order.
The margin upwards is 14 %: a torch build whose float32 CPU convolutions sum in another order and come out more than 12 % more accurate
fails that CPU assertion; the constants are then to be re-derived with the command above, not the window widened."""
import functools

import numpy as np
import torch

from tests import lpips_restatement as lr

SEED = 20240517
# name: (h, w, masked)
CASES = {
    "16x16": (16, 16, False),       # the minimum: the last tap is 1 x 1 and every tile is ragged
    "17x19": (17, 19, False),       # floor pooling drops a row or column at several levels
    "37x50": (37, 50, False),       # neither side is a multiple of any tile; 37 -> 18 -> 9 -> 4 -> 2
    "64x48": (64, 48, False),       # tile-aligned
    "72x100": (72, 100, True),      # several workgroups per dimension at the 64-channel layers, full K loop at 512; a disc mask
}

# the device's bounds (see the module docstring): feature error over the tap's abs-max, per tap; relative error of each d_k; of the total
FEATURE_BOUND = (1.5e-6, 1.8e-6, 2.5e-6, 2.3e-6, 2.5e-6)     # figures 4.44e-7, 5.26e-7, 7.24e-7, 6.52e-7, 7.30e-7
TERM_BOUND = 6.0e-6                                        # figure 1.70e-6
TOTAL_BOUND = 3.4e-7                                       # figure 9.95e-8
MIN_SHARE = 0.02


@functools.lru_cache(maxsize=None)
def weights():
    """(convs, lins) in float32: 13 (weight, bias) and 5 (1, C, 1, 1)."""
    g = torch.Generator().manual_seed(SEED)
    convs, cin = [], 3
    for block in lr.BLOCKS:
        for cout in block:
            w = torch.randn((cout, cin, 3, 3), generator=g) * float(np.sqrt(2.0 / (9 * cin)))
            b = (torch.rand((cout,), generator=g) - 0.5) * 0.1
            convs.append((w, b))
            cin = cout
    lins = [torch.rand((1, c, 1, 1), generator=g) for c in lr.TAP_CHANNELS]
    return convs, lins


@functools.lru_cache(maxsize=None)
def weights64():
    return lr.cast(*weights(), torch.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """in0, in1 (1, 3, h, w) float32 in [0, 1]."""
    h, w, masked = CASES[name]
    g = torch.Generator().manual_seed(SEED + 1 + sorted(CASES).index(name))
    pair = torch.rand((2, 1, 3, h, w), generator=g)
    if masked:                      # smooth content times noise inside a disc, zeros around it: like the reference's masked crops
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        smooth = torch.stack([0.6 + 0.4 * torch.sin(0.21 * xx + 0.13 * yy + c) * torch.cos(0.17 * yy - 0.05 * xx * c) for c in range(3)])
        disc = (((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0).float()
        pair = pair * smooth * disc
    return pair[0].contiguous(), pair[1].contiguous()


def _run(convs, lins, in0, in1):
    with torch.no_grad():
        f0, f1 = lr.taps(convs, in0), lr.taps(convs, in1)
        terms, val = lr.head(lins, f0, f1)
    return {"f0": f0, "f1": f1, "terms": [float(t) for t in terms], "total": float(val)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of a case, computed once per process: taps f0, f1 (lists of (1, C, h_k, w_k) float64), terms, total."""
    in0, in1 = case(name)
    return _run(*weights64(), in0.double(), in1.double())


def errors(got_f0, got_f1, got_terms, got_total, want):
    """(feature error over abs-max per tap, largest relative error of a d_k, relative error of the total) against a reference."""
    feat = []
    for k in range(5):
        e = max(float((got_f0[k].double() - want["f0"][k]).abs().max()), float((got_f1[k].double() - want["f1"][k]).abs().max()))
        feat.append(e / max(float(want["f0"][k].abs().max()), float(want["f1"][k].abs().max())))
    term = max(abs(float(got_terms[k]) - want["terms"][k]) / want["terms"][k] for k in range(5))
    return feat, term, abs(float(got_total) - want["total"]) / want["total"]


@functools.lru_cache(maxsize=None)
def float32_noise():
    """The restatement in float32 on the CPU against float64, pooled over the cases: (per-tap feature figures, term figure, total figure)."""
    feat, term, total = [0.0] * 5, 0.0, 0.0
    convs, lins = weights()
    for name in CASES:
        in0, in1 = case(name)
        got = _run(convs, lins, in0, in1)
        f, t, tt = errors(got["f0"], got["f1"], got["terms"], got["total"], reference(name))
        feat = [max(a, b) for a, b in zip(feat, f)]
        term, total = max(term, t), max(total, tt)
    return tuple(feat), term, total
