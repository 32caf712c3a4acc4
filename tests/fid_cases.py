"""Seeded weights, inputs, references and bounds shared by tests/test_fid_cpu.py and tests/test_fid_gpu.py.

Weights: tests/fid_restatement.py's Seeded (convolutions N(0, 2 / fan_in), gamma and var U(0.75, 1.25), beta and mean 0.1 N(0, 1)), one
fixed seed; with them the 2048 features have a mean of 0.1 - 0.5, a maximum of 1 - 5 and 14 - 49 % zeros: the network neither dies
nor explodes.  Inputs: uniform [0, 1), seeded per case.

Bounds: per block output k, the error is max|got - f64| / max|f64|, pooled (the largest) over the cases.  The device may differ from
the float64 restatement by a small multiple of what the same restatement run in float32 on the CPU - the arithmetic of pytorch-fid
itself - differs from it.  The constants below are the device's bounds: 3.5 x the pooled float32-CPU figures measured with

    python -c "from tests import fid_cases as fc; print(fc.float32_noise(), fc.float32_pipeline_noise())"

and rounded to two digits.  The device is allowed at most 4 x the pooled figure; tests/test_fid_cpu.py recomputes the figures and
asserts figure <= constant <= 4 x figure, and 3.5 leaves that window a margin on both sides for another CPU's summation order.  If
that CPU assertion fails on another torch build, the constants are to be re-derived with the command above, not the window widened."""
import functools

import numpy as np
import torch

from tests import fid_restatement as fr

SEED = 20241021
# name: (N, h, w, resize_input)
CASES = {
    "107x139": (2, 107, 139, False),        # odd, non-square maps 11 x 15, 5 x 7, 2 x 3: every tap shape straddles an edge; 7-tap rows on 5 x 7 maps
    "75x75": (1, 75, 75, False),            # the smallest legal input: maps 7, 3, 1; 7-tap kernels wider than the map; the global pool over 1 pixel
    "40x52->299": (1, 40, 52, True),        # enlarging, and the production map sizes 35, 17, 8
    "330x301->299": (1, 330, 301, True),    # shrinking without antialiasing
}
BLOCK_SHAPES = {"107x139": ((64, 25, 33), (192, 11, 15), (768, 5, 7), (2048, 1, 1)), "75x75": ((64, 17, 17), (192, 7, 7), (768, 3, 3), (2048, 1, 1)),
                "40x52->299": ((64, 73, 73), (192, 35, 35), (768, 17, 17), (2048, 1, 1)),
                "330x301->299": ((64, 73, 73), (192, 35, 35), (768, 17, 17), (2048, 1, 1))}

# the device's bounds (see the module docstring): block output error over the block's abs-max, per block
# (the two resized cases set the figures of blocks 0 - 2: F.interpolate in float32 computes its source coordinates in float32; without
# them the figures are 4.2e-7, 3.6e-7, 7.2e-7)
BLOCK_BOUND = (6.4e-5, 4.0e-5, 1.9e-5, 2.1e-6)      # figures 1.82e-5, 1.15e-5, 5.31e-6, 6.10e-7
# the end-to-end pipeline (two sets of 6 images of 40 x 52 -> features -> moments -> distance): relative error of the distance
PIPELINE_BOUND = 2.1e-6                             # figure 5.98e-7
PIPELINE_SETS = (6, 40, 52)


@functools.lru_cache(maxsize=None)
def weights():
    """The seeded parameter source, with every layer generated (in the network's order, by one small forward)."""
    P = fr.Seeded(SEED)
    with torch.no_grad():
        fr.blocks(P, torch.zeros((1, 3, 75, 75)), resize_input=False)
    assert len(P.rows) == 94
    return P


@functools.lru_cache(maxsize=None)
def case(name):
    """x (N, 3, h, w) float32 in [0, 1)."""
    n, h, w, _ = CASES[name]
    g = torch.Generator().manual_seed(SEED + 1 + sorted(CASES).index(name))
    return torch.rand((n, 3, h, w), generator=g)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of a case, computed once per process: the four block outputs."""
    with torch.no_grad():
        return tuple(fr.blocks(weights(), case(name).double(), resize_input=CASES[name][3]))


def errors(got, want):
    """max|got - want| / max|want| per block."""
    return [float((g.double().cpu() - w).abs().max()) / float(w.abs().max()) for g, w in zip(got, want)]


@functools.lru_cache(maxsize=None)
def float32_noise():
    """The restatement in float32 on the CPU against float64, pooled over the cases: the four per-block figures."""
    fig = [0.0] * 4
    for name in CASES:
        with torch.no_grad():
            got = fr.blocks(weights(), case(name), resize_input=CASES[name][3])
        fig = [max(a, b) for a, b in zip(fig, errors(got, reference(name)))]
    return tuple(fig)


# ---- the end-to-end pipeline ----
@functools.lru_cache(maxsize=None)
def pipeline_sets():
    """Two sets of 6 uniform random 40 x 52 images; the second set is darker, so the two statistics differ."""
    n, h, w = PIPELINE_SETS
    g = torch.Generator().manual_seed(SEED + 100)
    return torch.rand((n, 3, h, w), generator=g), 0.6 * torch.rand((n, 3, h, w), generator=g)


def pipeline_distance(feats_a, feats_b):
    """fp32 feature rows of the two sets -> the library's moment rule (numpy restatement) -> frechet_distance; also tr sigma of set a."""
    from humanliff_amd.fid import frechet_distance
    (mu_a, sig_a), (mu_b, sig_b) = fr.moments(feats_a), fr.moments(feats_b)
    return frechet_distance(mu_a, sig_a, mu_b, sig_b), float(np.trace(sig_a))


def _features(dtype):
    out = []
    for x in pipeline_sets():
        with torch.no_grad():
            out.append(fr.blocks(weights(), x.to(dtype))[3].reshape(x.shape[0], -1))
    return out


@functools.lru_cache(maxsize=None)
def pipeline_reference():
    """The distance of the two sets from the float64 restatement's features (moments in float64 of those values, not rounded to fp32)."""
    from humanliff_amd.fid import frechet_distance
    stats = []
    for f in _features(torch.float64):
        f = f.numpy()
        stats += [f.mean(0), np.cov(f, rowvar=False)]
    return frechet_distance(*stats)


@functools.lru_cache(maxsize=None)
def float32_pipeline_noise():
    """Relative difference of the float32-CPU pipeline's distance from the float64 one."""
    a, b = (f.numpy() for f in _features(torch.float32))
    return abs(pipeline_distance(a, b)[0] - pipeline_reference()) / pipeline_reference()
