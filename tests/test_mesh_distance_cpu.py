"""Measuring mesh distance without a device: the numpy restatement (tests/mesh_distance_restatement.py) against the properties the rules
promise, and the refusals that need no launch.  DESIGN.md "Measuring mesh distance"."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_distance_restatement as md  # noqa: E402

SPACING = 0.01


def sheet_queries(v, t, seed=3):
    """On, near and far outside the sheet: some vertices, some edge midpoints, jittered vertices, points in a box three times the bounds."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid = (lo + hi) / 2.0
    return np.concatenate([v[::31], (v[t[::57, 0]] + v[t[::57, 1]]) / 2.0, v[rng.integers(0, len(v), 40)] + rng.normal(size=(40, 3)) * 0.4 * SPACING,
                           mid[None] + (rng.random((20, 3)) - 0.5) * 3.0 * (hi - lo)[None]])


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_grid_walk_equals_brute_force_on_the_sheet(offset):
    v, t, _, _ = md.sheet(24, SPACING, seed=1, offset=(offset,) * 3)
    q = sheet_queries(v, t)
    ref = md.brute(q, v, t)
    tg = ref["target"]
    a, _, total, u = md.areas(tg)
    h = max(2.0 * np.sqrt(total * u / len(t)), float((tg["hi"] - tg["origin"]).max()) / 1024.0)
    for cell in (h, 0.6 * h, 5.0 * h) if offset == 0.0 else (h,):
        grid = md.build_grid(tg, cell)
        d2, tri, rings = md.grid_walk(q, tg, grid)
        print(f"sheet at {offset}: cell {cell:.4g}, grid {grid['g'].tolist()}, {len(q)} queries, up to {rings} rings, "
              f"{int((tri != ref['triangle']).sum())} differing ids, largest difference in d2 {np.abs(d2 - ref['sqdist']).max():.1e}")
        assert np.array_equal(tri, ref["triangle"]) and np.array_equal(d2, ref["sqdist"])
    assert rings >= 1
    # with a bound: inf / -1 exactly where the distance exceeds it, the same answer elsewhere
    bound = 2.0 * SPACING
    d2, tri, _ = md.grid_walk(q, tg, md.build_grid(tg, h), max_distance=bound)
    far = np.sqrt(ref["sqdist"]) > bound
    assert far.any() and (~far).any()
    assert np.array_equal(tri, np.where(far, -1, ref["triangle"])) and np.array_equal(d2, np.where(far, np.inf, ref["sqdist"]))


def test_wide_triangles_stay_exact():
    v, t, _, _ = md.sheet(24, SPACING, seed=1)
    n = 25
    lifted = v[[0, n * (n - 1), n * n - 1]] + np.asarray([0.0, 0.0, 0.05])[None]
    v2, t2 = np.concatenate([v, lifted]), np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]])
    tg = md.target(v2, t2)
    grid = md.build_grid(tg, 0.004)
    assert grid["wide"] == [len(t2) - 1]
    q = np.concatenate([v[::40] + np.asarray([0.0, 0.0, 0.06])[None], v[::40] - np.asarray([0.0, 0.0, 0.02])[None]])
    ref = md.brute(q, v2, t2)
    d2, tri, _ = md.grid_walk(q, tg, grid)
    assert (ref["triangle"] == len(t2) - 1).any() and (ref["triangle"] != len(t2) - 1).any()
    assert np.array_equal(tri, ref["triangle"]) and np.array_equal(d2, ref["sqdist"])


def test_branch_free_rule_on_degenerate_triangles():
    rng = np.random.default_rng(0)
    p = rng.normal(size=(2000, 3))
    a, b = rng.normal(size=(2000, 3)), rng.normal(size=(2000, 3))
    s = rng.random((2000, 1)) * 3.0 - 1.0
    for name, (ta, tb, tc) in {"a == b": (a, a, b), "b == c": (a, b, b), "collinear": (a, b, a + s * (b - a)), "point": (a, a, a)}.items():
        d2, win, x, bary = md.closest(p, ta, tb, tc)
        want = np.minimum(np.minimum(md.seg(p, ta, tb - ta)[0], md.seg(p, tb, tc - tb)[0]), md.seg(p, tc, ta - tc)[0])
        assert np.isfinite(d2).all() and np.isfinite(x).all() and np.isfinite(bary).all(), name
        if name != "collinear":                     # (collinear corners in floating point may leave a sliver with an interior)
            assert (win < 3).all(), name
        assert (d2 <= want).all() and np.abs(d2 - want).max() <= 1e-12 * 40.0, name
        assert np.abs(bary.sum(axis=1) - 1.0).max() <= 1e-15 * 4 and (bary >= 0.0).all(), name
        assert np.abs(x - (bary[:, :1] * ta + bary[:, 1:2] * tb + bary[:, 2:] * tc)).max() <= 1e-13, name


def test_branch_free_rule_against_ericson():
    """The region algorithm of Real-Time Collision Detection 5.1.5, written out: another route to the same closest point."""
    rng = np.random.default_rng(1)

    def ericson(p, a, b, c):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = ab @ ap, ac @ ap
        if d1 <= 0 and d2 <= 0:
            return a
        bp = p - b
        d3, d4 = ab @ bp, ac @ bp
        if d3 >= 0 and d4 <= d3:
            return b
        vc = d1 * d4 - d3 * d2
        if vc <= 0 and d1 >= 0 and d3 <= 0:
            return a + d1 / (d1 - d3) * ab
        cp = p - c
        d5, d6 = ab @ cp, ac @ cp
        if d6 >= 0 and d5 <= d6:
            return c
        vb = d5 * d2 - d1 * d6
        if vb <= 0 and d2 >= 0 and d6 <= 0:
            return a + d2 / (d2 - d6) * ac
        va = d3 * d6 - d5 * d4
        if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
            return b + (d4 - d3) / ((d4 - d3) + (d5 - d6)) * (c - b)
        den = 1.0 / (va + vb + vc)
        return a + ab * (vb * den) + ac * (vc * den)

    p, a, b, c = (rng.normal(size=(3000, 3)) for _ in range(4))
    d2 = md.closest(p, a, b, c)[0]
    want = np.asarray([((pi - ericson(pi, ai, bi, ci)) ** 2).sum() for pi, ai, bi, ci in zip(p, a, b, c)])
    print(f"branch-free rule against Ericson's regions on 3000 random triangles: largest difference in d2 {np.abs(d2 - want).max():.1e}")
    assert np.abs(d2 - want).max() <= 1e-12


def test_invalid_triangles_take_no_part():
    v, t, _, _ = md.sheet(4, SPACING)
    v2 = np.concatenate([v, [[np.nan, 0.0, 0.0]]])
    t2 = np.concatenate([t, [[0, 1, len(v)], [0, 1, len(v2)], [0, -1, 2]]])
    tg = md.target(v2, t2)
    assert tg["status"] == md.STATUS_INDEX | md.STATUS_CORNER and tg["valid"].sum() == len(t) and np.isfinite(tg["origin"]).all()
    ref = md.brute(v[:5] + 0.001, v2, t2)
    assert np.array_equal(ref["sqdist"], md.brute(v[:5] + 0.001, v, t)["sqdist"]) and np.isinf(ref["matrix"][:, len(t):]).all()


@pytest.mark.parametrize("mesh", ["sheet", "ellipsoid"])
def test_sampler_counts_follow_the_areas(mesh):
    v, t = md.sheet(24, SPACING, seed=1)[:2] if mesh == "sheet" else md.ellipsoid(24, 32)[:2]
    t = np.concatenate([t, [[0, 0, 1], [2, 2, 2]]])                   # two triangles without area, the last ones included
    tg = md.target(v, t)
    for S, seed in ((4096, 0), (1000, 7)):
        s = md.sample(tg, S, seed)
        counts = np.bincount(s["triangle"], minlength=len(t))
        want = S * s["area"].astype(np.float64) / s["total"]
        assert s["total"] > 0 and np.abs(counts - want).max() <= 1.0 + 1e-9
        assert (counts[s["area"] == 0] == 0).all() and (s["area"][-2:] == 0).all()
        assert (s["barycentric"] >= 0.0).all() and np.abs(s["barycentric"].sum(axis=1) - 1.0).max() <= 4e-16
        assert np.abs(np.linalg.norm(s["normals"], axis=1) - 1.0).max() <= 1e-15 * 4
        # the points lie on their triangles
        d2 = md.hit(s["points"], tg, s["triangle"])[0]
        L = float((tg["hi"] - tg["origin"]).max())
        assert d2.max() <= (1e-12 * L) ** 2
    assert not np.array_equal(md.sample(tg, 64, 0)["barycentric"], md.sample(tg, 64, 7)["barycentric"])
    # the constants are 2^64 / rho and 2^64 / rho^2 of the plastic number
    rho = 1.32471795724474602596
    assert abs(md.R2_A / 2.0 ** 64 - 1.0 / rho) < 1e-15 and abs(md.R2_B / 2.0 ** 64 - 1.0 / rho ** 2) < 1e-15


def test_validate_refuses_without_a_device():
    import torch
    from humanliff_amd.NeRF import distance as ds
    v, t, n, _ = md.sheet(4)
    q = v[:7] + 0.001
    ok = ds._validate(q, v, t, normals=n[:7], cell=0.01, max_distance=0.5, thresholds=(0.1, 0.2))
    assert ok[4] == 0.01 and ok[5] == 0.5 and ok[6] == [0.1, 0.2]
    assert ds._validate(q.astype(np.float32), {"vertices": v, "triangles": t.astype(np.int32)})[4] is None
    with pytest.raises(ValueError, match="vertices"):
        ds._validate(q, v[:, :2], t)
    with pytest.raises(ValueError, match="vertices"):
        ds._validate(q, v.astype(np.int64), t)
    with pytest.raises(ValueError, match="triangles"):
        ds._validate(q, v, t[:, :2])
    with pytest.raises(ValueError, match="triangles"):
        ds._validate(q, v, t.astype(np.float32))
    with pytest.raises(ValueError, match="triangles"):
        ds._validate(q, v, t[:0])
    with pytest.raises(ValueError, match="missing"):
        ds._validate(q, v)
    with pytest.raises(ValueError, match="not both"):
        ds._validate(q, {"vertices": v, "triangles": t}, t)
    with pytest.raises(ValueError, match="points"):
        ds._validate(q[:, :2], v, t)
    with pytest.raises(ValueError, match="points"):
        ds._validate(q.astype(np.int32), v, t)
    with pytest.raises(ValueError, match="normals"):
        ds._validate(q, v, t, normals=n[:6])
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="cell"):
            ds._validate(q, v, t, cell=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            ds._validate(q, v, t, max_distance=bad)
    with pytest.raises(ValueError, match="thresholds"):
        ds._validate(q, v, t, thresholds=[0.1] * 9)
    with pytest.raises(ValueError, match="thresholds"):
        ds._validate(q, v, t, thresholds=[-0.1])
    for what, args in (("points", (torch.zeros(3, 3), v, t)), ("vertices", (q, torch.zeros(5, 3), t)), ("triangles", (q, v, torch.zeros(5, 3, dtype=torch.int64)))):
        with pytest.raises(RuntimeError, match=f"`{what}` is a CPU tensor"):
            ds._validate(*args)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ds.point_mesh_distance(torch.zeros(3, 3), v, t)
    # the public functions refuse the same way, before a device is needed
    with pytest.raises(ValueError, match="cell"):
        ds.point_mesh_distance(q, v, t, cell=0.0)
    with pytest.raises(ValueError, match="thresholds"):
        ds.mesh_distance((v, t), (v, t), thresholds=[0.1] * 9)
    with pytest.raises(ValueError, match="samples"):
        ds.sample_surface(v, 0, t)
    with pytest.raises(ValueError, match="samples"):
        ds.sample_surface(v, 1 << 31, t)
    with pytest.raises(ValueError, match="samples"):
        ds.mesh_distance((v, t), (v, t), samples=-1)


def test_default_cell():
    from humanliff_amd.NeRF.distance import DEFAULT_CELLS, default_cell
    lo, hi = np.zeros(3), np.asarray([1.0, 2.0, 0.5])
    assert default_cell(4.0, 100, 2.0, lo, hi) == 2.0 * np.sqrt(4.0 / 100)
    h = default_cell(1e-12, 100, 2.0, lo, hi)                           # tiny triangles: the bounds decide, and the cap on the cells
    g = np.floor(hi / h) + 1
    assert h >= 2.0 / 1024 and g.prod() <= DEFAULT_CELLS < (np.floor(hi / (h / 1.25)) + 1).prod()
    assert default_cell(0.0, 1, 0.0, lo, lo) == 1.0


def test_exports_and_signatures():
    from humanliff_amd import _lib
    header = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    names = ("hl_mesh_distance_scratch_bytes", "hl_mesh_distance_areas", "hl_mesh_distance_count", "hl_mesh_distance_fill", "hl_mesh_distance_query",
             "hl_mesh_distance_sample", "hl_mesh_distance_reduce")
    for name in names:
        assert name + "(" in header and name in _lib.SIGNATURES
        decl = re.search(name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_mesh_distance")) == sorted(names)
    for macro in ("WIDE_CELLS", "MAX_WIDE", "REDUCE_FIELDS"):
        assert int(re.search(rf"#define HL_DISTANCE_{macro} (\d+)", header).group(1)) == getattr(_lib, "HL_DISTANCE_" + macro)
    assert md.WIDE_CELLS == _lib.HL_DISTANCE_WIDE_CELLS
    assert _lib.HL_DISTANCE_REDUCE_WORDS == 16 + 16 * int(re.search(r"#define HL_DISTANCE_REDUCE_BLOCKS (\d+)", header).group(1))


def test_size_query_refuses_bad_sizes():
    """Host arithmetic of the library: the refusals that come before any launch."""
    from humanliff_amd import _lib
    from humanliff_amd.build import build
    build()
    L = _lib.lib()
    q = L.hl_mesh_distance_scratch_bytes
    assert q(200, 4, 5, 6) > 0 and q(200, 4, 5, 6) % 16 == 0
    assert q(200, 4, 5, 6) >= 200 * 80 + 200 * 4 + 121 * 4 + 120 * 4 + 65536 * 4
    assert q(200, 1 << 9, 1 << 9, 1 << 9) > 0
    for bad in ((0, 4, 5, 6), (1 << 31, 4, 5, 6), (-1, 4, 5, 6), (200, 0, 5, 6), (200, 4, -1, 6), (200, 1 << 9, 1 << 9, (1 << 9) + 1),
                (200, 1 << 40, 1 << 40, 1 << 40)):
        assert q(*bad) == 0, bad
    # every entry refuses before a launch: sizes, cell, grid, references, wide list, thresholds (NULL pointers are never reached)
    o = (_lib.C.c_double * 3)(0.0, 0.0, 0.0)
    bad_o = (_lib.C.c_double * 3)(0.0, float("nan"), 0.0)
    inf = float("inf")
    assert L.hl_mesh_distance_count(None, 0, None, 10, o, 1.0, 1, 1, 1, None, None, None, 0, None) < 0 and b"sizes" in L.hl_last_error()
    assert L.hl_mesh_distance_count(None, 10, None, 10, o, 0.0, 1, 1, 1, None, None, None, 0, None) < 0 and b"cell" in L.hl_last_error()
    assert L.hl_mesh_distance_count(None, 10, None, 10, o, inf, 1, 1, 1, None, None, None, 0, None) < 0
    assert L.hl_mesh_distance_count(None, 10, None, 10, bad_o, 1.0, 1, 1, 1, None, None, None, 0, None) < 0
    assert L.hl_mesh_distance_count(None, 10, None, 10, o, 1.0, 1 << 10, 1 << 10, 1 << 8, None, None, None, 0, None) < 0 and b"2^27" in L.hl_last_error()
    assert L.hl_mesh_distance_fill(10, o, 1.0, 1, 1, 1, None, (1 << 31) + 1, None, 0, None) < 0 and b"2^31" in L.hl_last_error()
    assert L.hl_mesh_distance_query(None, None, 1 << 31, 10, o, 1.0, 1, 1, 1, None, 0, 0, inf, None, None, None, None, None, None, None, None, 0, None) < 0
    assert L.hl_mesh_distance_query(None, None, 5, 10, o, 1.0, 1, 1, 1, None, 0, 65537, inf, None, None, None, None, None, None, None, None, 0, None) < 0
    assert b"wide" in L.hl_last_error()
    assert L.hl_mesh_distance_sample(None, 10, None, 10, o, None, 5, 0, 0, None, None, None, None, None) < 0
    assert L.hl_mesh_distance_sample(None, 10, None, 10, o, None, 0, 5, 0, None, None, None, None, None) < 0 and b"area" in L.hl_last_error()
    assert L.hl_mesh_distance_areas(None, 10, None, 10, o, 0.0, None, None, None, 0, None) < 0
    assert L.hl_mesh_distance_reduce(None, None, None, 5, None, 9, None, None) < 0 and b"thresholds" in L.hl_last_error()
    assert L.hl_mesh_distance_reduce(None, None, None, 0, None, 0, None, None) < 0
