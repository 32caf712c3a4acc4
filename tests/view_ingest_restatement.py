"""numpy restatement of the view ingest (recon_NeRF/lib/SynBody_dataset.py:266-278 of the reference): the resize rule of one
axis written out from the contract, the masked float source, and the two reductions - float64, and float32 accumulating in table order as
the kernel does.  OpenCV is not available, so the rule as the contract states it is the yardstick."""
import math

import numpy as np


def area_rule(src, dst):
    """Per output: the list of (source index, float64 weight) taps in table order."""
    scale = src / dst
    out = []
    for dx in range(dst):
        f1 = dx * scale
        f2 = f1 + scale
        cell = min(scale, src - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), src - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, (s1 - f1) / cell))
        for s in range(s1, s2):
            taps.append((s, 1.0 / cell))
        if f2 - s2 > 1e-3:
            taps.append((s2, min(min(f2 - s2, 1.0), cell) / cell))
        out.append(taps)
    return out


def tap_arrays(src, dst, dtype=np.float32):
    """area_rule as arrays: idx (dst, T) int32, w (dst, T) `dtype`, count (dst) int32; unused slots are (0, 0)."""
    rule = area_rule(src, dst)
    T = max(len(t) for t in rule)
    idx, w, count = np.zeros((dst, T), dtype=np.int32), np.zeros((dst, T), dtype=dtype), np.zeros((dst,), dtype=np.int32)
    for d, taps in enumerate(rule):
        count[d] = len(taps)
        for k, (s, wt) in enumerate(taps):
            idx[d, k], w[d, k] = s, dtype(wt)
    return idx, w, count


def nearest_rule(src, dst):
    """min(floor(d * (src / dst)), src - 1) in float64, as the contract words it."""
    scale = src / dst
    return np.array([min(math.floor(d * scale), src - 1) for d in range(dst)], dtype=np.int64)


def nearest_rule_int(src, dst):
    """The same in integers: floor(d * src / dst) exactly."""
    return np.array([min(d * src // dst, src - 1) for d in range(dst)], dtype=np.int64)


def masked_source(img_u8, msk_u8):
    """fp32(u8) / 255 in float32 true division, zero where the mask is zero: (..., Hs, Ws, 3) float32."""
    img = img_u8.astype(np.float32) / np.float32(255)
    img[msk_u8 == 0] = 0
    return img


def _reduce(src, H, W, dtype):
    """sum over the row taps of beta * (sum over the column taps of alpha * p), every product and sum in `dtype`, taps in table order."""
    Hs, Ws = src.shape[-3], src.shape[-2]
    xi, xw, _ = tap_arrays(Ws, W, np.float32)
    yi, yw, _ = tap_arrays(Hs, H, np.float32)
    src = src.astype(dtype)
    xw, yw = xw.astype(dtype), yw.astype(dtype)                     # the float32 weights, exactly
    rows = np.zeros(src.shape[:-2] + (W, 3), dtype=dtype)           # (..., Hs, W, 3)
    for k in range(xi.shape[1]):
        rows = rows + xw[:, k, None] * src[..., xi[:, k], :]
    out = np.zeros(src.shape[:-3] + (H, W, 3), dtype=dtype)
    for k in range(yi.shape[1]):
        out = out + yw[:, k, None, None] * rows[..., yi[:, k], :, :]
    return out


def resize_area_f64(src_f32, H, W):
    return _reduce(src_f32, H, W, np.float64)


def resize_area_f32(src_f32, H, W):
    out = _reduce(src_f32, H, W, np.float32)
    assert out.dtype == np.float32
    return out


def resize_nearest(msk_u8, H, W):
    """(..., H, W) uint8 of 0 / 1: the nearest source mask pixel != 0, indices by the integer rule."""
    Hs, Ws = msk_u8.shape[-2:]
    yi, xi = nearest_rule_int(Hs, H), nearest_rule_int(Ws, W)
    return (msk_u8[..., yi[:, None], xi[None, :]] != 0).astype(np.uint8)


def window_fully_masked(msk_u8, H, W):
    """(..., H, W) bool: every source pixel under the output pixel's taps is masked out."""
    Hs, Ws = msk_u8.shape[-2:]
    xr, yr = area_rule(Ws, W), area_rule(Hs, H)
    on = msk_u8 != 0
    out = np.zeros(msk_u8.shape[:-2] + (H, W), dtype=bool)
    for y in range(H):
        ys = [s for s, _ in yr[y]]
        for x in range(W):
            xs = [s for s, _ in xr[x]]
            out[..., y, x] = ~on[..., ys, :][..., :, xs].any(axis=(-1, -2))
    return out
