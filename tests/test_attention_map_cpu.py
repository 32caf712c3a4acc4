"""The attention kernels' block id -> (image-head, query tile) map (csrc/hl_xcd_map.h) without a GPU: the header is compiled as plain C++ into a small
shared library and called through ctypes.  The map must be a bijection (every tile computed exactly once, wherever a block really runs), and the blocks
congruent mod 8 - one XCD's - must cover one contiguous run of work items, so that an XCD sees a contiguous run of heads."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "humanliff_amd", "csrc")

_SRC = r"""
#include "hl_xcd_map.h"
extern "C" void map_all(int total, int inner_count, int *group, int *inner, int *item) {
    for (int b = 0; b < total; ++b) {
        hl::xcd_group_item(b, total, inner_count, true, group[b], inner[b]);
        item[b] = hl::xcd_work_item(b, total);
    }
}
"""


@pytest.fixture(scope="module")
def maplib(tmp_path_factory):
    from humanliff_amd import build
    tmp = tmp_path_factory.mktemp("xcd_map")
    src, lib = str(tmp / "map.cpp"), str(tmp / "libmap.so")
    with open(src, "w") as f:
        f.write(_SRC)
    r = subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I", CSRC, src, "-o", lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    L = ctypes.CDLL(lib)
    L.map_all.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.map_all.restype = None
    return L


def _grids():
    """(inner items per group, groups) of the launches tests/test_attention_tiles_gpu.py makes, with one and two query tiles per workgroup, and of
    512- and 256-block grids (the 32-pixel level at B = 4)."""
    out = []
    for N, T, heads in [(1, 64, 4), (3, 96, 4), (1, 100, 4), (5, 160, 4), (3, 72, 4), (16, 1024, 4), (4, 1024, 4)]:
        qtiles = (T + 31) // 32
        for qt in (1, 2):
            out.append(((qtiles + qt - 1) // qt, N * heads))
    return sorted(set(out))


@pytest.mark.parametrize("inner_count,groups", _grids())
def test_block_map_is_a_bijection_with_contiguous_runs_per_xcd(maplib, inner_count, groups):
    total = inner_count * groups
    group, inner, item = (np.full(total, -1, dtype=np.int32) for _ in range(3))
    maplib.map_all(total, inner_count, group.ctypes.data, inner.ctypes.data, item.ctypes.data)
    assert (inner >= 0).all() and (inner < inner_count).all() and (group >= 0).all() and (group < groups).all()
    assert (item == group * inner_count + inner).all()
    assert sorted(item.tolist()) == list(range(total))                    # every (group, inner) exactly once
    prev_end = 0
    for xcd in range(8):
        run = item[xcd::8]                                                # the blocks the dispatcher gives one XCD, in launch order
        if len(run) == 0:
            continue
        assert (np.diff(run) == 1).all(), xcd                             # consecutive work items: inner fastest, then the next group
        assert run[0] == prev_end, xcd                                    # ... and the runs of XCD 0, 1, ... follow each other
        prev_end = run[-1] + 1
        assert len(np.unique(group[xcd::8])) <= (len(run) + inner_count - 2) // inner_count + 1
    assert prev_end == total


def test_block_map_grid_sizes():
    """The grids this file means: 512 and 256 blocks are among them (B = 4, T = 1024 with one and two query tiles per workgroup)."""
    totals = {a * b for a, b in _grids()}
    assert {512, 256, 4, 36, 100}.issubset(totals)
