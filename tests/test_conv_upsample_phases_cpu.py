"""The Upsample convolutions as four 2x2-tap phase convolutions (k_conv_h2s_ph), without a GPU: the phase / tap table of hl_conv_h16.hip
(h2p_taps) against the nearest-x2 + 3x3 convolution in float64, the kernel's register budget, and the plans of the shapes the GPU tests run."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_h2s_tiles_cpu import _kernel_metadata

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "humanliff_amd", "csrc", "hl_conv_h16.hip")

K_H2S, K_H2S_PH = 7, 10      # hl_conv2d_plan's kernel numbers (include/humanliff_hip.h)


# ---- the device helper, line for line
def h2p_taps(q, t):
    """the 3x3 rows (or columns) that tap t of parity q sums, as a bit mask"""
    return (1 if t == 0 else 6) if q == 0 else (3 if t == 0 else 4)


def test_table_is_the_one_in_the_source():
    text = open(SRC).read()
    assert re.search(r"h2p_taps\(int q, int t\) \{ return q == 0 \? \(t == 0 \? 1u : 6u\) : \(t == 0 \? 3u : 4u\); \}", text)


def phase_weights(w, ph):
    """(Cout, Cin, 2, 2): the summed taps of phase ph = 2 py + px, in the dtype of w"""
    out = torch.zeros(w.shape[:2] + (2, 2), dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            rows, cols = h2p_taps(ph >> 1, a), h2p_taps(ph & 1, b)
            for ky in range(3):
                for kx in range(3):
                    if rows >> ky & 1 and cols >> kx & 1:
                        out[:, :, a, b] += w[:, :, ky, kx]
    return out


def test_every_3x3_tap_lands_on_exactly_one_phase_tap():
    for q in range(2):
        assert h2p_taps(q, 0) | h2p_taps(q, 1) == 7 and h2p_taps(q, 0) & h2p_taps(q, 1) == 0


def test_phase_convolutions_are_the_upsampled_3x3_convolution():
    """Output pixel (2i + py, 2j + px) = sum over a, b in {0, 1} of the phase weights times source pixel (i - 1 + py + a, j - 1 + px + b), the source
    zero outside the image - on a 5x7 source, so every border and both parities of either axis are inside the comparison."""
    g = torch.Generator().manual_seed(57)
    x = torch.randn((2, 3, 5, 7), generator=g, dtype=torch.float64)
    w = torch.randn((4, 3, 3, 3), generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = torch.zeros_like(want)
    xp = F.pad(x, (1, 1, 1, 1))                      # source pixel (i, j) at (i + 1, j + 1)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        # rows i - 1 + py + a of the source = rows i + py + a of the padded one: a plain 2x2 correlation from offset (py, px)
        got[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + 6, px:px + 8], phase_weights(w, ph))
    assert float((got - want).abs().max()) < 1e-13


def test_conv_h2s_ph_register_and_lds_budget():
    """two workgroups per CU, like k_conv_h2s: <= 256 registers per lane, no scratch, no static LDS"""
    md = _kernel_metadata("k_conv_h2s_ph")
    assert md["vgpr_count"] + md["agpr_count"] <= 256, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["group_segment_fixed_size"] == 0, md


@pytest.fixture(scope="module", autouse=True)
def _library():
    from humanliff_amd.build import build
    build()


def plan(N, H, W, Cin, Cout, ups=1, mode=None):
    """(kernel, split-K slabs) of the single-op 3x3 / stride-1 convolution: hl_conv2d_plan, host arithmetic"""
    from humanliff_amd import _lib
    L = _lib.lib()
    k, s = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(L.hl_conv2d_plan(_lib.HL_CONV_FP32 if mode is None else mode, N, H, W, Cin, Cout, 3, 1, ups, 0, ctypes.byref(k), ctypes.byref(s)))
    return k.value, s.value


@pytest.mark.parametrize("shape,want", [
    ((1, 40, 80, 96, 384), (K_H2S_PH, 1)),       # 100 workgroups' worth: exactly the unsplit threshold
    ((1, 40, 80, 32, 384), (K_H2S_PH, 1)),
    ((1, 40, 80, 64, 384), (K_H2S_PH, 1)),
    ((4, 8, 16, 160, 192), (K_H2S_PH, 2)),       # the split-K floor: five chunks in slabs of 3 + 2
    ((4, 32, 32, 384, 384), (K_H2S_PH, 1)),      # the ups row of test_conv3x3_fp16x2_products_match_float64
    ((8, 8, 8, 128, 192), (K_H2S, 2)),           # source width 8: the nine-tap kernel keeps the layer
])
def test_plans_of_the_upsample_shapes(shape, want):
    assert plan(*shape) == want


def test_only_the_default_mode_and_only_upsample_layers_take_the_phases():
    from humanliff_amd import _lib
    assert plan(1, 80, 160, 96, 384, ups=0) == (K_H2S, 1)
    for mode in (_lib.HL_CONV_FP32_DIRECT, _lib.HL_CONV_FP32_MFMA, _lib.HL_CONV_FP32_F23, _lib.HL_CONV_BF16X3, _lib.HL_CONV_FP16):
        assert plan(1, 40, 80, 96, 384, mode=mode)[0] != K_H2S_PH, mode
    # below the split-K floor / with a single slab possible the layer never reached k_conv_h2s and does not reach the phases either
    assert plan(2, 8, 8, 64, 192)[0] not in (K_H2S, K_H2S_PH)
    assert plan(2, 16, 32, 64, 192)[0] not in (K_H2S, K_H2S_PH)
