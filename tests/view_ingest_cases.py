"""Seeded cases of the view ingest shared by tests/test_view_ingest_cpu.py and tests/test_view_ingest_gpu.py, their restated results (computed
once, read only) and the device bound derived from them."""
import functools

import numpy as np

from tests import view_ingest_restatement as vr

# name -> (Hs, Ws, image_scaling)
CASES = {
    "int2": (32, 48, 0.5),          # integer factors
    "int4": (32, 48, 0.25),
    "ragged": (37, 53, 0.5),        # 18 x 26: both axes fractional
    "frac": (50, 40, 0.4),          # 20 x 16: factor 2.5
    "tiny": (7, 9, 0.5),            # 3 x 4
    "copy": (24, 24, 1.0),
}
VIEWS = 3

# max |float32 restatement - float64 restatement| over CASES is 9.24e-08 (test_bound_is_twice_the_measured_gap recomputes it); the device
# may sum a window in another order and contract to fma, and both orders fall under the same n 2^-24 analysis, so it gets twice that.
DEVICE_BOUND = 1.85e-07


def target_size(name):
    Hs, Ws, s = CASES[name]
    return int(Hs * s), int(Ws * s)


@functools.lru_cache(maxsize=None)
def case(name):
    """(img_u8 (3, Hs, Ws, 3), msk_u8 (3, Hs, Ws)): random images; each view's mask is a disc of 255 (the third view's holds other non-zero
    values too) whose edge cuts through output windows and leaves some windows wholly outside."""
    Hs, Ws, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    img = rng.integers(0, 256, (VIEWS, Hs, Ws, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    msk = np.zeros((VIEWS, Hs, Ws), dtype=np.uint8)
    for v in range(VIEWS):
        cy, cx = Hs * (0.45 + 0.05 * v), Ws * (0.5 - 0.04 * v)
        r = min(Hs, Ws) * (0.42 - 0.07 * v)
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        msk[v][disc] = 255
    msk[2][msk[2] != 0] = rng.integers(1, 256, int((msk[2] != 0).sum()), dtype=np.uint8)
    img.setflags(write=False)
    msk.setflags(write=False)
    return img, msk


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict: 'source' (masked float32 source), 'f64', 'f32' (3, H, W, 3), 'body' (3, H, W) uint8, 'dark' (3, H, W) bool."""
    img, msk = case(name)
    H, W = target_size(name)
    src = vr.masked_source(img, msk)
    out = {"source": src, "f64": vr.resize_area_f64(src, H, W), "f32": vr.resize_area_f32(src, H, W), "body": vr.resize_nearest(msk, H, W),
           "dark": vr.window_fully_masked(msk, H, W)}
    for a in out.values():
        a.setflags(write=False)
    return out


def measured_gap():
    """max |float32 restatement - float64 restatement| over the committed cases."""
    return max(float(np.abs(reference(n)["f32"].astype(np.float64) - reference(n)["f64"]).max()) for n in CASES)
