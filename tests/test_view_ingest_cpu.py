"""The view ingest without a GPU: the host tap tables (hl_area_taps, hl_nearest_taps, hl_view_ingest_table) against the rule written out
in tests/view_ingest_restatement.py, the restatement on cases with a known answer, the device bound against the figure it is derived
from, the new C-ABI symbols and the kernels' scratch budget."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import view_ingest_cases as vc
from tests import view_ingest_restatement as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (src, dst): the sizes the rule was checked on by hand, the axes of the committed cases, and the benchmark's 1024 -> 512 / 409
SIZES = [(37, 18), (53, 26), (32, 16), (48, 12), (101, 50), (50, 20), (7, 3), (5, 4), (48, 24), (32, 8), (40, 16), (9, 4), (24, 24), (1, 1),
         (1024, 512), (1024, 409), (640, 1)]
SYMBOLS = ("hl_area_max_taps", "hl_area_taps", "hl_nearest_taps", "hl_view_ingest_table_words", "hl_view_ingest_table", "hl_view_ingest")


@pytest.fixture(scope="module")
def vi():
    from humanliff_amd import view_ingest
    from humanliff_amd.build import build
    build()
    return view_ingest


# ---- the host tables --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SIZES)
def test_area_taps_equal_the_rule_tap_for_tap(vi, src, dst):
    idx, w, count = vi.area_taps(src, dst)
    ri, rw, rc = vr.tap_arrays(src, dst)
    T = ri.shape[1]
    assert idx.dtype == np.int32 and w.dtype == np.float32 and count.dtype == np.int32
    assert idx.shape == w.shape == (dst, -(-src // dst) + 1) and T <= idx.shape[1]
    assert np.array_equal(count, rc)
    assert np.array_equal(idx[:, :T], ri) and np.array_equal(w[:, :T], rw)                 # the float32 weights bit for bit
    assert not idx[:, T:].any() and not w[:, T:].any()
    for d in range(dst):
        assert not idx[d, count[d]:].any() and not w[d, count[d]:].any()
        assert (w[d, :count[d]] > 0).all()
        assert (np.diff(idx[d, :count[d]]) == 1).all()                                     # a window is a run of neighbours
    # taps are in range and the weights of an output sum to 1
    assert count.min() >= 1 and idx.min() >= 0 and max(idx[d, :count[d]].max() for d in range(dst)) < src
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    rule = vr.area_rule(src, dst)
    # (float64 weights: 2e-15 on the small sizes; the cell of 1024 -> 409 is no dyadic number and f1 is near 1000, so a few ulp of f1 show)
    assert max(abs(sum(wt for _, wt in taps) - 1.0) for taps in rule) <= (2e-15 if src <= 101 else 1e-13)
    assert np.array_equal(vi.nearest_taps(src, dst), vr.nearest_rule(src, dst))
    assert np.array_equal(vr.nearest_rule(src, dst), vr.nearest_rule_int(src, dst))


@pytest.mark.parametrize("src,dst", [(32, 16), (48, 12), (48, 24), (32, 8), (1024, 512), (24, 24)])
def test_integer_factors_give_uniform_weights(vi, src, dst):
    f = src // dst
    idx, w, count = vi.area_taps(src, dst)
    assert (count == f).all()
    assert np.array_equal(idx[:, :f], np.arange(src, dtype=np.int32).reshape(dst, f))
    assert (w[:, :f] == np.float32(1.0 / f)).all()
    assert np.array_equal(vi.nearest_taps(src, dst), np.arange(dst) * f)


def test_scale_four_has_at_most_four_taps(vi):
    assert vi.area_taps(48, 12)[2].max() == 4 and vi.area_taps(50, 20)[2].max() == 3
    from humanliff_amd import _lib
    L = _lib.lib()
    assert L.hl_area_max_taps(48, 12) == 5 and L.hl_area_max_taps(24, 24) == 2 and L.hl_area_max_taps(7, 3) == 4
    assert L.hl_area_max_taps(3, 7) == 0 and L.hl_area_max_taps(0, 0) == 0


def test_packed_table_layout(vi):
    for src, dst in ((7, 3), (53, 26), (48, 12)):
        idx, w, count = vi.area_taps(src, dst)
        T = idx.shape[1]
        table = vi.packed_table(src, dst)
        assert table.dtype == np.int32 and table.shape == (dst * (2 + 2 * T),)
        assert np.array_equal(table[:dst], count) and np.array_equal(table[dst:2 * dst], vr.nearest_rule(src, dst))
        assert np.array_equal(table[2 * dst:(2 + T) * dst].reshape(dst, T), idx)
        assert np.array_equal(table[(2 + T) * dst:].view(np.float32).reshape(dst, T), w)


def test_enlarging_raises_before_any_launch(vi):
    from humanliff_amd import _lib
    with pytest.raises(ValueError):
        vi.area_taps(4, 5)
    with pytest.raises(ValueError):
        vi.packed_table(4, 5)
    with pytest.raises(ValueError):
        vi.check_sizes(32, 48, 33, 48)
    with pytest.raises(ValueError):
        vi.check_sizes(32, 48, 16, 49)
    with pytest.raises(ValueError):
        vi.check_sizes(32, 48, 0, 24)
    assert vi.check_sizes(32, 48, 32, 48) == (32, 48, 32, 48)
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data
    assert L.hl_area_taps(4, 5, 4, p, p, p) < 0 and b"hl_area_taps" in L.hl_last_error()
    assert L.hl_view_ingest_table(4, 5, p) < 0 and L.hl_view_ingest_table_words(4, 5) == 0
    assert L.hl_area_taps(5, 4, 1, p, p, p) < 0 and b"max_taps" in L.hl_last_error()        # a table too small is refused, not overrun
    # arguments are checked before anything is launched (the pointers are never read: 16 is only an aligned non-NULL value)
    assert L.hl_view_ingest(16, 16, 1, 8, 8, 9, 8, 16, 16, 16, 16, None) < 0 and b"enlarges" in L.hl_last_error()
    assert L.hl_view_ingest(None, None, 1, 8, 8, 4, 4, None, None, None, None, None) < 0 and b"hl_view_ingest" in L.hl_last_error()
    assert L.hl_view_ingest(16, 16, 1, 8, 8, 4, 4, 16, 16, 24, 16, None) < 0 and b"aligned" in L.hl_last_error()
    assert L.hl_view_ingest(16, 16, 1, 8, 64000, 4, 100, 16, 16, 16, 16, None) < 0 and b"LDS" in L.hl_last_error()
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        vi.ingest_views(x, x[..., 0], 4, 4)                                                  # no CPU path


# ---- the restatement and the bound ------------------------------------------------------------------------------------------------
def test_restatement_on_cases_with_a_known_answer():
    img, msk = vc.case("int2")
    ref = vc.reference("int2")
    H, W = vc.target_size("int2")
    assert (H, W) == (16, 24) and vc.target_size("ragged") == (18, 26) and vc.target_size("frac") == (20, 16) and vc.target_size("tiny") == (3, 4)
    want = ref["source"].astype(np.float64).reshape(3, H, 2, W, 2, 3).mean(axis=(2, 4))      # an integer factor is the block mean
    assert np.abs(ref["f64"] - want).max() <= 4 * np.spacing(1.0)
    assert np.array_equal(ref["body"], (msk[:, ::2, ::2] != 0).astype(np.uint8))
    copy = vc.reference("copy")
    assert np.array_equal(copy["f32"], copy["source"]) and np.array_equal(copy["f64"], copy["source"].astype(np.float64))
    assert np.array_equal(copy["body"], (vc.case("copy")[1] != 0).astype(np.uint8))
    for name in vc.CASES:
        ref = vc.reference(name)
        dark, body = ref["dark"], ref["body"]
        assert 0 < dark.sum() < dark.size and 0 < body.sum() < body.size, name               # the mask's edge runs through the image
        assert not ref["f32"][dark].any() and not ref["f64"][dark].any(), name                 # exact zeros
        inside = vr.window_fully_masked((vc.case(name)[1] == 0).astype(np.uint8), *vc.target_size(name))
        assert (~dark & ~inside).any() or name == "copy", name                                  # windows the edge cuts through (one pixel at 1.0)
        assert ref["f64"].min() >= 0.0 and ref["f64"].max() <= 1.0 + 1e-12


def test_bound_is_twice_the_measured_gap():
    gap = vc.measured_gap()
    print(f"max |float32 - float64 restatement| over the cases: {gap:.4e}; device bound {vc.DEVICE_BOUND:.4e}")
    assert gap > 0.0
    assert gap <= vc.DEVICE_BOUND <= 4 * gap
    assert abs(vc.DEVICE_BOUND / gap - 2.0) < 0.05
    # within the n 2^-24 analysis: at most 5 x 5 products and sums of values below 1
    assert vc.DEVICE_BOUND < 50 * 2.0 ** -24


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_view_ingest_symbols_are_declared_bound_and_exported(vi):
    from humanliff_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    from humanliff_amd import build
    assert "hl_view_ingest.hip" in [os.path.basename(s) for s in build._sources()]


def test_view_ingest_kernels_use_no_scratch():
    from humanliff_amd import build
    src = os.path.join(build.CSRC, "hl_view_ingest.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "view_ingest.s")
        r = subprocess.run([build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        text = open(out).read()
    meta = text[text.index(".amdgpu_metadata"):]
    seen = []
    for entry in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+\S*(k_view_[a-z_]+?)E", entry)
        if m:
            md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
            assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (m.group(1), md)
            assert md["group_segment_fixed_size"] == 0, (m.group(1), md)                       # (the staging area is dynamic LDS)
            seen.append(m.group(1))
    assert sorted(seen) == ["k_view_convert", "k_view_ingest"]
