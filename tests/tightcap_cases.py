"""Seeded sources of the layered view ingest shared by tests/golden/gen_golden_tightcap.py, tests/test_tightcap_dataset_cpu.py and
tests/test_tightcap_ingest_gpu.py, their restated results (computed once, read only) and the reduction shapes the GPU tests run."""
import functools

import numpy as np

from tests import tightcap_restatement as tr

PLANES = tr.PLANES

# name -> (V, Hs, Ws, H, W, layers): the shapes of tests/view_ingest_cases.py and of test_more_than_one_tile_and_unaligned_rows
REDUCTIONS = {
    "int2": (4, 32, 48, 16, 24, (0, 1, 2, 3)),
    "ragged": (4, 37, 53, 18, 26, (3, 2, 1, 0)),
    "frac": (4, 50, 40, 20, 16, (1, 0, 3, 2)),
    "tiny": (4, 7, 9, 3, 4, (0, 1, 2, 3)),              # 63 pixels a view: the 32 combinations still all occur
    "tiles": (1, 5, 1031, 2, 515, (0,)),                # three 256-pixel tiles in a row, source rows that start at odd addresses
}
# scale one: 5 views of 9 x 15 - V Hs Ws = 675 is odd, so groups of four pixels straddle views and the last three go bytewise
COPY = (5, 9, 15, (0, 1, 2, 3, 1))


def source(V, Hs, Ws, seed):
    """(img_u8 (V, Hs, Ws, 3), {plane: (V, Hs, Ws) uint8}): random photographs of which a quarter of the pixels are (0, 0, 0); the five
    planes take every one of their 32 combinations in every view - the black pixels cycle through them on their own and so do the others,
    where a view has 32 of each (7 x 9 has too few black ones) - with non-zero bytes of 1, 128 and 255: "binary" means byte != 0."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (V, Hs, Ws, 3), dtype=np.uint8)
    img[rng.random((V, Hs, Ws)) < 0.25] = 0
    n = Hs * Ws
    combo = np.empty((V, n), dtype=np.int64)
    for v in range(V):
        c = np.arange(n) % 32
        # black pixels and others must both meet every combination: give the black ones a full cycle of their own
        black = np.flatnonzero(~img[v].reshape(n, 3).any(axis=-1))
        c[black] = np.arange(len(black)) % 32
        other = np.setdiff1d(np.arange(n), black)
        c[other] = rng.permutation(len(other)) % 32
        combo[v] = c
    values = np.array([1, 128, 255], dtype=np.uint8)
    planes = {}
    for b, name in enumerate(PLANES):
        on = ((combo >> b) & 1).astype(bool).reshape(V, Hs, Ws)
        planes[name] = np.where(on, values[rng.integers(0, 3, (V, Hs, Ws))], np.uint8(0)).astype(np.uint8)
    return img, planes


def combinations(planes):
    """(V, Hs, Ws) int64: bit b is set where plane PLANES[b] is non-zero."""
    return sum(((planes[n] != 0).astype(np.int64) << b) for b, n in enumerate(PLANES))


@functools.lru_cache(maxsize=None)
def case(name):
    """(img_u8, planes, layers (V,) int64, H, W) of a REDUCTIONS entry or of 'copy'; read only."""
    if name == "copy":
        V, Hs, Ws, layers = COPY
        H, W = Hs, Ws
    else:
        V, Hs, Ws, H, W, layers = REDUCTIONS[name]
    img, planes = source(V, Hs, Ws, 300 + sorted(list(REDUCTIONS) + ["copy"]).index(name))
    img.setflags(write=False)
    for p in planes.values():
        p.setflags(write=False)
    return img, planes, np.asarray(layers, dtype=np.int64), H, W


@functools.lru_cache(maxsize=None)
def reference(name):
    """tightcap_restatement.ingest of the case; read only."""
    img, planes, layers, H, W = case(name)
    out = tr.ingest(img, planes, layers, H, W)
    for a in out.values():
        a.setflags(write=False)
    return out


def own_bound(ref):
    """The rule of tests/view_ingest_cases.py for one shape: twice the measured gap between the float32 and the float64 restatement."""
    return 2 * float(np.abs(ref["f32"].astype(np.float64) - ref["f64"]).max())
