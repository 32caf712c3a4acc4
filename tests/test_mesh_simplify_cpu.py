"""Simplifying the mesh without a device: the numpy restatement (tests/mesh_simplify_restatement.py) against the properties the rule
promises, and the refusals of simplify_mesh that need no launch.  DESIGN.md "Simplifying the mesh"."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_simplify_restatement as ms  # noqa: E402


@pytest.fixture(scope="module")
def coarse():
    v, t, n = ms.ellipsoid(24, 32)
    return v, t, n, ms.simplify(v, t, 0.06, normals=n)


def test_restatement_on_the_ellipsoid(coarse):
    v, t, n, r = coarse
    assert len(t) == 1472 and len(v) == 2 + 23 * 32
    out_v, out_t, ids = r["vertices"], r["triangles"], r["ids"]
    print(f"ellipsoid 24 x 32, cell 0.06: {len(t)} -> {len(out_t)} triangles, {len(v)} -> {len(out_v)} vertices, {len(r['ckey'])} clusters, "
          f"largest condition number {r['cond']:.1f}")
    assert 0 < len(out_t) < len(t) and 0 < len(out_v) < len(v)
    # no triangle with two equal ids, no duplicate oriented key
    assert (out_t[:, 0] != out_t[:, 1]).all() and (out_t[:, 1] != out_t[:, 2]).all() and (out_t[:, 0] != out_t[:, 2]).all()
    assert (out_t[:, 0] < out_t[:, 1]).all() and (out_t[:, 0] < out_t[:, 2]).all()            # the smallest id leads
    keys = (out_t[:, 0] << 42) | (out_t[:, 1] << 21) | out_t[:, 2]
    assert len(np.unique(keys)) == len(keys)
    # every vertex referenced, every index in range
    assert out_t.min() >= 0 and out_t.max() < len(out_v)
    assert np.array_equal(np.unique(out_t), np.arange(len(out_v)))
    # every vertex inside its cell, and vertex_map consistent with the cells
    ckey, g = r["ckey"][r["used"]], r["g"]
    ci = np.stack([ckey % g[0], (ckey // g[0]) % g[1], ckey // (g[0] * g[1])], axis=1)
    rel = (out_v - r["origin"][None]) / r["cell"][None] - ci
    assert (rel >= -1e-12).all() and (rel <= 1 + 1e-12).all()
    assert (np.abs(r["p"]) <= 0.5).all()
    assert (np.diff(ckey) > 0).all()                                                     # ascending key order
    vm = r["vertex_map"]
    assert vm.shape == (len(v),) and vm.max() == len(out_v) - 1
    inside = vm >= 0
    cell_of_input = np.floor((v - r["origin"][None]) / r["cell"][None]).astype(np.int64)
    assert np.array_equal(cell_of_input[inside], ci[vm[inside]])
    assert np.array_equal(vm < 0, ~r["used"][ids])
    # the condition number stays under 3 / lambda + 1, the vertices near the surface, the normals unit
    assert 1.0 < r["cond"] <= (3.0 / ms.LAMBDA + 1.0) * (1 + 1e-9)                     # (reached by a cluster whose planes are parallel)
    level = ms.ellipsoid_level(out_v)
    print(f"implicit function at the output vertices: {level.min():.4f} .. {level.max():.4f}")
    assert np.abs(level - 1.0).max() < 0.03
    assert np.abs(np.linalg.norm(r["normals"], axis=1) - 1.0).max() < 1e-12
    # orientation kept: the flat normals still point away from the centre
    a, b, c = (out_v[out_t[:, k]] for k in range(3))
    outward = np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3.0 - np.asarray(ms.ELLIPSOID_CENTRE)[None])
    assert (outward > 0).mean() > 0.99


def test_restatement_compacts_vertices_on_the_fine_ellipsoid():
    v, t, _ = ms.ellipsoid(96, 128)
    r = ms.simplify(v, t, 0.04)
    assert len(t) == 24320
    print(f"ellipsoid 96 x 128, cell 0.04: {len(r['triangles'])} triangles, {len(r['vertices'])} vertices of {len(r['ckey'])} clusters")
    assert (~r["used"]).sum() >= 1 and len(r["vertices"]) == r["used"].sum()
    assert np.array_equal(np.unique(r["triangles"]), np.arange(len(r["vertices"])))


def test_simplify_mesh_refuses_without_a_device():
    from humanliff_amd.NeRF.simplify import simplify_mesh
    v, t, n, c = ms.sheet(4)
    ok = dict(cell=0.02)
    with pytest.raises(ValueError, match="vertices"):
        simplify_mesh(v[:, :2], t, **ok)
    with pytest.raises(ValueError, match="vertices"):
        simplify_mesh(v.astype(np.int64), t, **ok)
    with pytest.raises(ValueError, match="triangles"):
        simplify_mesh(v, t[:, :2], **ok)
    with pytest.raises(ValueError, match="triangles"):
        simplify_mesh(v, t.astype(np.float32), **ok)
    with pytest.raises(ValueError, match="triangles"):
        simplify_mesh(v, t[:0], **ok)
    with pytest.raises(ValueError, match="missing"):
        simplify_mesh(v, **ok)
    with pytest.raises(ValueError, match="not both"):
        simplify_mesh({"vertices": v, "triangles": t}, t, **ok)
    for bad in (0.0, -1.0, float("nan"), float("inf"), (0.02, 0.0, 0.02), (0.02, 0.02)):
        with pytest.raises(ValueError, match="cell"):
            simplify_mesh(v, t, cell=bad)
    for bad in ((0.0, float("nan"), 0.0), (0.0, 0.0, float("inf")), (0.0, 0.0)):
        with pytest.raises(ValueError, match="origin"):
            simplify_mesh(v, t, cell=0.02, origin=bad)
    with pytest.raises(ValueError, match="normals"):
        simplify_mesh(v, t, normals=n[:-1], **ok)
    with pytest.raises(ValueError, match="colors"):
        simplify_mesh(v, t, colors=c[:-1], **ok)
    with pytest.raises(ValueError, match="colors"):
        simplify_mesh(v, t, colors=c.astype(np.float32), **ok)
    with pytest.raises(ValueError, match="normals"):
        simplify_mesh({"vertices": v, "triangles": t, "normals": n[:3], "colors": None}, **ok)
    # a grid beyond 2^31 cells: the sheet spans about 0.04 x 0.04 x 0.03 world units, some 4000 x 4000 x 3000 cells of 1e-5
    with pytest.raises(ValueError, match="2\\^31"):
        simplify_mesh(v, t, cell=1e-5)
    with pytest.raises(ValueError, match="2\\^31"):
        simplify_mesh(v, t, cell=0.02, origin=(-1e9, 0.0, -1.0))


def test_exports_and_signatures():
    from humanliff_amd import _lib
    header = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    names = ("hl_mesh_simplify_bounds", "hl_mesh_simplify_scratch_bytes", "hl_mesh_simplify_count", "hl_mesh_simplify_emit")
    for name in names:
        assert name + "(" in header and name in _lib.SIGNATURES
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_mesh_simplify")) == sorted(names)
    assert int(re.search(r"#define HL_SIMPLIFY_ACC_WORDS (\d+)", header).group(1)) == _lib.HL_SIMPLIFY_ACC_WORDS == len(ms.ACC_FIELDS)
    assert _lib.HL_SIMPLIFY_BOUNDS_WORDS == 6 + 6 * int(re.search(r"#define HL_SIMPLIFY_BOUNDS_BLOCKS (\d+)", header).group(1))


def test_size_query_refuses_bad_sizes():
    """Host arithmetic of the library: the refusals that come before any launch."""
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    q = L.hl_mesh_simplify_scratch_bytes
    assert q(100, 200, 4, 5, 6) > 0 and q(100, 200, 4, 5, 6) % 16 == 0
    for bad in ((0, 200, 4, 5, 6), (100, 0, 4, 5, 6), (1 << 31, 200, 4, 5, 6), (100, 1 << 31, 4, 5, 6), (100, 200, 0, 5, 6), (100, 200, 4, -1, 6),
                (100, 200, 1 << 11, 1 << 11, (1 << 9) + 1), (100, 200, 1 << 40, 1 << 40, 1 << 40)):
        assert q(*bad) == 0, bad
    assert q(100, 200, 1 << 11, 1 << 11, 1 << 9) > 0                                     # exactly 2^31 cells
    import ctypes as C
    cell, org = (C.c_double * 3)(0.1, 0.1, 0.1), (C.c_double * 3)(0.0, 0.0, 0.0)
    # (the pointers are never touched: every one of these is refused before a launch)
    assert L.hl_mesh_simplify_count(None, 0, 5, cell, org, 2, 2, 2, None, None, None, 0, None) == -1
    assert L.hl_mesh_simplify_count(None, 5, 5, (C.c_double * 3)(0.1, 0.0, 0.1), org, 2, 2, 2, None, None, None, 0, None) == -1
    assert L.hl_mesh_simplify_count(None, 5, 5, cell, (C.c_double * 3)(0.0, float("nan"), 0.0), 2, 2, 2, None, None, None, 0, None) == -1
    assert L.hl_mesh_simplify_count(None, 5, 5, cell, org, 1 << 11, 1 << 11, 1 << 10, None, None, None, 0, None) == -1
    assert b"2^31" in L.hl_last_error()
    assert L.hl_mesh_simplify_emit(None, None, None, 5, None, 5, cell, org, 1 << 11, 1 << 10, 1 << 10, (1 << 21) + 1, None, None, None, None, None, None,
                                   None, None, 0, None) == -1
    assert b"2^21" in L.hl_last_error()
    assert L.hl_mesh_simplify_bounds(None, 0, None, None, None) == -1
