"""Measuring mesh distance on the MI355X (hl_mesh_distance.hip) against the numpy restatement (tests/mesh_distance_restatement.py, which
states the closest-point rule, the grid walk and the sampler once more).  DESIGN.md "Measuring mesh distance".

Bounds.  Per query, judged by the restatement alone: |sqdist_dev - d2_ref(q, triangle_dev)| <= 1e-12 Lq^2 and d2_ref(q, triangle_dev) <=
min_t d2_ref(q, t) + 1e-12 Lq^2, with Lq the largest absolute coordinate relative to the origin among queries and target vertices: about
30 roundings at 2^-53 on magnitudes up to 3 Lq^2 give about 1e-14, which leaves two orders of margin.  No query is excused.  What is
expected is equal bits and equal ids (the same IEEE operations in the same order); every case prints how many differ.  `distance` is
within 2 ulp of sqrt(sqdist_dev).  normal_dot within 1e-12.  Sample points within 1e-12 L.  The score sums within Q 2^-53 relative, the
worst case of any order of non-negative summands."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_distance_restatement as md  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-12
SPACING = 0.01
KEYS = ("sqdist", "triangle", "barycentric", "point")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def run(q, v, t, **kw):
    """point_mesh_distance -> its outputs as numpy (status as an int)."""
    from humanliff_amd.NeRF.distance import point_mesh_distance
    out = point_mesh_distance(q, v, t, **kw)
    return {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in out.items()} | {"status": int(out["status"].item())}


def same_bytes(a, b, keys=KEYS + ("distance",)):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in keys)


def against_restatement(name, got, q, v, t, normals=None, matrix=None):
    """The comparison every case goes through -> the restatement's matrix of squared distances (Q,T)."""
    q = np.asarray(q, dtype=np.float64)
    tg = md.target(v, t)
    m = md.sqdist_matrix(q, tg) if matrix is None else matrix
    fin = np.isfinite(q).all(axis=1)
    vfin = np.asarray(v, dtype=np.float64)[np.isfinite(v).all(axis=1)]
    Lq = max(np.abs(q[fin] - tg["origin"][None]).max(), np.abs(vfin - tg["origin"][None]).max())
    tol = REL * Lq * Lq
    tri = got["triangle"]
    assert got["sqdist"].dtype == np.float64 and tri.dtype == np.int64 and got["sqdist"].shape == (len(q),) and tri.shape == (len(q),), name
    assert np.array_equal(got["origin"], tg["origin"]), name
    assert (tri[fin] >= 0).all() and (tri[fin] < len(t)).all() and tg["valid"][tri[fin]].all(), name
    assert (tri[~fin] == -1).all() and np.isnan(got["sqdist"][~fin]).all() and np.isnan(got["distance"][~fin]).all(), name
    rows = np.nonzero(fin)[0]
    at_dev = m[rows, tri[fin]]
    best, arg = m[rows].min(axis=1), m[rows].argmin(axis=1)
    err, gap = np.abs(got["sqdist"][fin] - at_dev), at_dev - best
    d_ref, x_ref, b_ref = md.hit(q[fin], tg, tri[fin])
    assert np.array_equal(d_ref, at_dev)
    print(f"{name}: {len(q)} queries, {len(t)} triangles, grid {got['info']['extents']}, {got['info']['wide']} wide, {got['info']['references']} references; "
          f"ids that differ from the restatement's: {int((tri[fin] != arg).sum())}, sqdist not bit-equal: {int((got['sqdist'][fin] != best).sum())} "
          f"(largest difference {err.max():.3e}, bound {tol:.3e}); barycentrics not bit-equal: {int((got['barycentric'][fin] != b_ref).any(axis=1).sum())}, "
          f"points: {int((got['point'][fin] != x_ref).any(axis=1).sum())}")
    assert (err <= tol).all(), name
    assert (gap <= tol).all(), name
    ulp = np.spacing(np.sqrt(got["sqdist"][fin]))
    assert (np.abs(got["distance"][fin] - np.sqrt(got["sqdist"][fin])) <= 2 * ulp).all(), name
    assert np.abs(got["point"][fin] - x_ref).max() <= REL * max(Lq, np.abs(tg["origin"]).max()), name
    cn = tg["corners"][tri[fin]]
    rebuilt = (got["barycentric"][fin][:, :, None] * cn).sum(axis=1) + tg["origin"][None]
    assert np.abs(rebuilt - got["point"][fin]).max() <= REL * max(Lq, np.abs(tg["origin"]).max()), name
    assert (got["barycentric"][fin] >= 0.0).all() and np.abs(got["barycentric"][fin].sum(axis=1) - 1.0).max() <= 1e-15 * 4, name
    if normals is not None:
        want = md.normal_dot(np.asarray(normals)[fin], tg, tri[fin])
        nd = got["normal_dot"][fin]
        assert np.array_equal(np.isnan(nd), np.isnan(want)), name
        ok = ~np.isnan(want)
        print(f"{name}: normal_dot against the restatement: max {np.abs(nd[ok] - want[ok]).max():.3e} (bound {REL:g}), {int((nd[ok] != want[ok]).sum())} not bit-equal")
        assert np.abs(nd[ok] - want[ok]).max() <= REL, name
    return m


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def lattice(x):
    return np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** 20) / 2.0 ** 20


def _sheet_case():
    """Case 1, on a 2^-20 lattice (the midpoints on 2^-21) so that case 3 can move it exactly: the vertices, the edge midpoints, 1 000
    jittered vertices and 100 points in a box three times the bounds."""
    v, t, _, _ = md.sheet(24, SPACING, seed=1)
    v = lattice(v)
    rng = np.random.default_rng(5)
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    lo, hi = v.min(axis=0), v.max(axis=0)
    q = np.concatenate([v, (v[edges[:, 0]] + v[edges[:, 1]]) / 2.0, lattice(v[rng.integers(0, len(v), 1000)] + rng.normal(size=(1000, 3)) * 0.4 * SPACING),
                        lattice((lo + hi)[None] / 2.0 + (rng.random((100, 3)) - 0.5) * 3.0 * (hi - lo)[None])])
    return v, t, q


@pytest.fixture(scope="module")
def sheet_case(dev):
    v, t, q = _sheet_case()
    assert len(t) == 1152 and len(v) == 625
    got = run(q, v, t)
    return v, t, q, got, against_restatement("sheet 24 x 24", got, q, v, t)


def test_sheet(sheet_case):
    v, t, q, got, m = sheet_case
    ties = (m == m.min(axis=1, keepdims=True)).sum(axis=1)
    assert ties[:625].max() == 6 and (ties[:625] >= 2).sum() >= 623 and (got["sqdist"][:625] == 0.0).all()   # a vertex: every triangle around it
    E = 3 * 24 * 24 + 2 * 24                                                                                # edges; all but the 96 of the border have two triangles
    assert (ties[625:625 + E] >= 2).sum() >= E - 96 and (got["sqdist"][625:625 + E] == 0.0).all()
    assert got["info"]["wide"] == 0 and got["info"]["valid"] == len(t) and got["status"] == 0 and got["normal_dot"] is None
    assert min(got["info"]["extents"]) >= 2                                                               # more than one cell: rings happen


def test_ellipsoid_with_normals(dev):
    v, t, _ = md.ellipsoid(24, 32)
    fine, _, nrm = md.ellipsoid(48, 64)
    c = np.asarray(md.ELLIPSOID_CENTRE)
    q = np.concatenate([c[None] + 1.02 * (fine - c[None]), c[None] + 0.9 * (fine - c[None])])
    n = np.concatenate([nrm, nrm])
    n[5] = 0.0                                       # a zero query normal: NaN
    assert len(t) == 1472
    got = run(q, v, t, normals=n)
    against_restatement("ellipsoid 24 x 32", got, q, v, t, normals=n)
    assert np.isnan(got["normal_dot"][5]) and np.nanmin(got["normal_dot"]) > 0.5


def test_far_from_the_origin(sheet_case):
    v, t, q, near, m = sheet_case
    off = np.full(3, 1000.0)
    assert np.array_equal((v + off) - off, v) and np.array_equal((q + off) - off, q)
    far = run(q + off, v + off, t)
    against_restatement("sheet at (1000, 1000, 1000)", far, q + off, v + off, t)
    assert same_bytes(near, far, ("sqdist", "distance", "triangle", "barycentric"))
    assert np.array_equal(far["origin"], near["origin"] + off)


def test_wide_triangle(dev):
    v, t, _, _ = md.sheet(24, SPACING, seed=1)
    n = 25
    lifted = v[[0, n * (n - 1), n * n - 1]] + np.asarray([0.0, 0.0, 0.05])[None]
    v2, t2 = np.concatenate([v, lifted]), np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]])
    rng = np.random.default_rng(2)
    base = v[rng.integers(0, len(v), 300)]
    q = np.concatenate([base + np.asarray([0.0, 0.0, 0.06])[None], base - np.asarray([0.0, 0.0, 0.02])[None], base + rng.normal(size=base.shape) * 0.02])
    got = run(q, v2, t2, cell=0.004)
    against_restatement("sheet plus a wide triangle", got, q, v2, t2)
    assert got["info"]["wide"] == 1 and got["info"]["valid"] == len(t2)
    assert (got["triangle"] == len(t2) - 1).any() and (got["triangle"] != len(t2) - 1).any()


def test_degenerate_and_invalid(dev):
    from humanliff_amd.NeRF.distance import STATUS_CORNER, STATUS_INDEX, STATUS_QUERY
    v, t, _, _ = md.sheet(6, SPACING, seed=1)
    N = len(v)
    extra = np.asarray([[0.0, 0.0, 0.1], [0.03, 0.0, 0.1], [0.06, 0.0, 0.1],          # N .. N+2: collinear
                        [0.0, 0.05, 0.1], [0.04, 0.05, 0.12],                          # N+3, N+4: a segment through a repeated index
                        [0.03, 0.03, 0.15],                                            # N+5: a point
                        [np.nan, 0.0, 0.0]])                                           # N+6
    v2 = np.concatenate([v, extra])
    degenerate = np.asarray([[N, N + 1, N + 2], [N + 3, N + 3, N + 4], [N + 5, N + 5, N + 5]])
    rng = np.random.default_rng(4)
    q = np.concatenate([v[::3] + 0.002, extra[:6] + rng.normal(size=(6, 3)) * 0.005, extra[:6], rng.random((40, 3)) * 0.08 + np.asarray([0.0, 0.0, 0.08])])
    good = np.concatenate([t, degenerate])
    got = run(q, v2, good)                                                             # the NaN vertex is referenced by nobody: fine
    m = against_restatement("degenerate triangles", got, q, v2, good)
    assert got["status"] == 0 and np.isfinite(got["sqdist"]).all() and (got["triangle"] >= len(t)).sum() >= 12
    tg = md.target(v2, good)
    p = q - tg["origin"][None]
    tol = REL * max(np.abs(p).max(), np.abs(tg["corners"]).max()) ** 2
    for k in range(3):                                                                 # the segment / point distances
        cn = tg["corners"][len(t) + k]
        seg3 = np.minimum(np.minimum(md.seg(p, cn[0], cn[1] - cn[0])[0], md.seg(p, cn[1], cn[2] - cn[1])[0]), md.seg(p, cn[2], cn[0] - cn[2])[0])
        hit = got["triangle"] == len(t) + k
        assert hit.any() and np.abs(got["sqdist"][hit] - seg3[hit]).max() <= tol
    bad_corner, bad_index = np.asarray([[0, 1, N + 6]]), np.asarray([[0, 1, N + 7], [0, -1, 2]])
    everything = np.concatenate([good, bad_corner, bad_index])
    qn = np.concatenate([q, [[0.0, np.nan, 0.0]]])
    loose = run(qn, v2, everything, check=False)
    against_restatement("degenerate and invalid, check=False", loose, qn, v2, everything)
    assert loose["status"] == STATUS_INDEX | STATUS_CORNER | STATUS_QUERY and loose["info"]["valid"] == len(good)
    assert same_bytes({k: x[:-1] for k, x in loose.items() if k in KEYS}, got, KEYS) and (loose["triangle"] < len(good)).all()
    assert np.isnan(loose["barycentric"][-1]).all() and np.isnan(loose["point"][-1]).all()
    with pytest.raises(ValueError, match="non-finite corner"):
        run(q, v2, np.concatenate([good, bad_corner]))
    with pytest.raises(ValueError, match="index outside"):
        run(q, v2, np.concatenate([good, bad_index]))
    with pytest.raises(ValueError, match="non-finite coordinate"):
        run(qn, v2, good)
    with pytest.raises(ValueError, match="no valid triangle"):
        run(q, v2, bad_index, check=False)


def test_tiny(dev):
    v = np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    t = np.asarray([[0, 1, 2]])
    q = np.asarray([[0.25, 0.25, 2.0]])
    got = run(q, v, t, cell=4.0)
    against_restatement("one triangle, one query", got, q, v, t)
    assert got["info"]["extents"] == (1, 1, 1) and got["sqdist"][0] == 4.0 and got["distance"][0] == 2.0 and got["triangle"][0] == 0
    assert np.array_equal(got["point"][0], [0.25, 0.25, 0.0]) and np.array_equal(got["barycentric"][0], [0.5, 0.25, 0.25])
    empty = run(np.zeros((0, 3)), v, t, normals=np.zeros((0, 3)))
    assert empty["sqdist"].shape == (0,) and empty["triangle"].shape == (0,) and empty["triangle"].dtype == np.int64
    assert empty["barycentric"].shape == (0, 3) and empty["point"].shape == (0, 3) and empty["normal_dot"].shape == (0,)
    same = np.tile(np.asarray([[0.9, 0.8, -0.3]]), (300, 1))                          # more than one workgroup of identical queries
    got = run(same, v, t)
    against_restatement("three vertices, identical queries", got, same, v, t)
    assert len(np.unique(got["sqdist"])) == 1 and (got["triangle"] == 0).all()


def test_independent_of_the_grid(sheet_case):
    v, t, q, got, _ = sheet_case
    h = got["cell"]
    extents = {got["info"]["extents"]}
    for cell in (0.5 * h, 4.0 * h, 100.0 * h):
        other = run(q, v, t, cell=cell)
        extents.add(other["info"]["extents"])
        assert other["cell"] == cell and same_bytes(got, other), cell
    assert len(extents) == 4 and (1, 1, 1) in extents


def test_independent_of_order_and_run(sheet_case):
    v, t, q, got, m = sheet_case
    assert same_bytes(got, run(q, v, t))
    perm = np.random.default_rng(6).permutation(len(t))                              # new triangle k is old triangle perm[k]
    shuffled = run(q, v, t[perm])
    assert same_bytes(got, shuffled, ("sqdist", "distance"))
    unique = (m == m.min(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique.sum() > 500 and np.array_equal(perm[shuffled["triangle"]][unique], got["triangle"][unique])
    assert same_bytes({k: x[unique] for k, x in got.items() if k in KEYS}, {k: x[unique] for k, x in shuffled.items() if k in KEYS}, ("barycentric", "point"))
    # device tensors of another float dtype in: the same answer as the same values from the host
    q32, v32 = q.astype(np.float32), v.astype(np.float32)
    assert same_bytes(run(q32, v32, t), run(torch.from_numpy(q32).cuda(), torch.from_numpy(v32).cuda(), torch.from_numpy(t).cuda()))


def test_max_distance(sheet_case):
    v, t, q, got, m = sheet_case
    bound = 1.5 * SPACING
    far = np.sqrt(m.min(axis=1)) > bound
    assert far.sum() >= 50 and (~far).sum() >= 1000
    for cell in (None, 0.3 * got["cell"]):
        cut = run(q, v, t, max_distance=bound, cell=cell)
        assert np.array_equal(cut["triangle"] == -1, far) and np.isposinf(cut["sqdist"][far]).all() and np.isposinf(cut["distance"][far]).all()
        assert np.isnan(cut["point"][far]).all() and np.isnan(cut["barycentric"][far]).all()
        assert same_bytes({k: x[~far] for k, x in cut.items() if k in KEYS + ("distance",)}, {k: x[~far] for k, x in got.items() if k in KEYS + ("distance",)})


@pytest.mark.parametrize("mesh", ["sheet", "ellipsoid"])
def test_sampler(dev, mesh):
    from humanliff_amd.NeRF.distance import sample_surface
    v, t = md.sheet(24, SPACING, seed=1)[:2] if mesh == "sheet" else md.ellipsoid(24, 32)[:2]
    t = np.concatenate([t[:100], [[0, 0, 1], [3, 3, 3]], t[100:], [[5, 6, 5]]])      # triangles without area, the last one included
    tg = md.target(v, t)
    L = float((tg["hi"] - tg["origin"]).max())
    for seed in (0, 7):
        got = {k: x.cpu().numpy() for k, x in sample_surface({"vertices": v, "triangles": t}, 4096, seed=seed).items()}
        want = md.sample(tg, 4096, seed)
        assert got["triangle"].dtype == np.int64 and np.array_equal(got["triangle"], want["triangle"])
        assert np.array_equal(got["barycentric"], want["barycentric"])
        err = np.abs(got["points"] - want["points"]).max()
        print(f"sampler, {mesh}, seed {seed}: points bit-equal to the restatement: {int((got['points'] == want['points']).all(axis=1).sum())} of 4096 "
              f"(largest difference {err:.3e}, bound {REL * L:.3e}); normals bit-equal: {int((got['normals'] == want['normals']).all(axis=1).sum())}")
        assert err <= REL * L and np.abs(got["normals"] - want["normals"]).max() <= REL
        assert (want["area"][got["triangle"]] > 0).all() and not np.isin(got["triangle"], [100, 101, len(t) - 1]).any()
    with pytest.raises(ValueError, match="no area"):
        sample_surface(v, 16, np.asarray([[0, 0, 1], [2, 2, 2]]))


def _regular_sheet(T):
    """The first T triangles of an n x n sheet of quads over the xy plane with a smooth bump in z, n the smallest with 2 n^2 >= T."""
    n = int(np.ceil(np.sqrt(T / 2.0)))
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i.reshape(-1).astype(np.float64), j.reshape(-1).astype(np.float64)
    v = np.stack([x, y, 0.25 * n * np.sin(x / n * 2.0) * np.cos(y / n * 3.0)], axis=1) * SPACING
    a, b = (k.reshape(-1) for k in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    at = lambda p, q: p * (n + 1) + q  # noqa: E731
    quads = np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1), at(a, b), at(a + 1, b + 1), at(a, b + 1)], axis=1)
    return v, quads.reshape(-1, 3)[:T].astype(np.int64)


@pytest.mark.parametrize("T", [1, 4095, 4096, 4097, 4096 * 256 + 1])
def test_area_prefix_at_the_scan_tile_edges(dev, T):
    """Every exclusive scan of the mesh path goes through scan_exclusive (hl_scan.h): a tile is 256 x 16 = 4096 values, and from
    4096 x 256 + 1 values on a thread of k_scan_top owns more than one tile sum.  The area prefix and total are integer sums: equal."""
    from humanliff_amd.NeRF import distance as ds
    v, t = _regular_sheet(T)
    assert len(t) == T
    verts, tri, _ = ds._device_mesh("test", v, t)
    lo, hi = ds._bounds(verts)
    ar = ds._Areas(verts, tri, lo, hi)
    a, P, total, u = md.areas(md.target(v, t))
    prefix = ar.prefix.cpu().numpy()
    print(f"area prefix, T {T}: total {ar.total} against {total}, {int((prefix != P).sum())} of {T} prefix words differ; areas {a.min()} .. {a.max()}")
    assert ar.unit == u and a.min() > 0
    assert prefix.dtype == np.int64 and np.array_equal(prefix, P)
    assert ar.total == total and ar.area == total * u


def test_scores(dev):
    from humanliff_amd.NeRF import distance as ds
    va, ta, na = md.ellipsoid(24, 32)
    vb, tb, nb = md.ellipsoid(48, 64)
    a, b = {"vertices": va, "triangles": ta, "normals": na}, {"vertices": vb, "triangles": tb, "normals": nb}
    th = (0.01, 0.03)
    score = ds.mesh_distance(a, b, samples=2048, thresholds=th)
    assert score == ds.mesh_distance(a, b, samples=2048, thresholds=th)              # equal Python floats
    # the same queries once more, piece by piece: the reduction against numpy on the device's own per-query arrays
    for name, src, dst in (("a_to_b", a, b), ("b_to_a", b, a)):
        verts, tri, nrm = ds._device_mesh("test", src, None)
        pts, pn = ds._side_queries(verts, tri, nrm, 2048, 0)
        assert pts.shape == (len(src["vertices"]) + 2048, 3)
        hit = ds.build_index(dst).query(pts, pn)
        got = ds.reduce_queries(hit, th)
        assert {k: x for k, x in got.items()} == score[name]
        d, d2, nd = hit["distance"].cpu().numpy(), hit["sqdist"].cpu().numpy(), hit["normal_dot"].cpu().numpy()
        want = md.side(d, d2, nd, th)
        Q = len(d)
        rel = Q * 2.0 ** -53
        assert got["count"] == want["count"] == Q and got["max"] == want["max"]
        assert [round(w * Q) for w in got["within"]] == [round(w * Q) for w in want["within"]] and 0.0 < got["within"][0] <= got["within"][1] <= 1.0
        assert abs(got["mean"] - want["mean"]) <= rel * want["mean"] and abs(got["mean_sq"] - want["mean_sq"]) <= rel * want["mean_sq"]
        assert abs(got["rms"] - want["rms"]) <= rel * want["rms"]
        assert np.isfinite(nd).all() and abs(got["normal_consistency"] - want["normal_consistency"]) <= rel * np.abs(nd).sum() / Q
        print(f"scores, {name}: {Q} queries, mean {got['mean']:.6e}, rms {got['rms']:.6e}, max {got['max']:.6e}, within {got['within']}, "
              f"normal consistency {got['normal_consistency']:.6f}; mean against numpy: {abs(got['mean'] - want['mean']) / want['mean']:.1e} relative")
    ab, ba = score["a_to_b"], score["b_to_a"]
    assert score["chamfer"] == ab["mean"] + ba["mean"] and score["chamfer_sq"] == ab["mean_sq"] + ba["mean_sq"] and score["hausdorff"] == max(ab["max"], ba["max"])
    assert score["fscore"] == [2.0 * p * r / (p + r) for p, r in zip(ab["within"], ba["within"])]
    # a mesh against itself
    itself = ds.mesh_distance(a, a, samples=2048, thresholds=(0.01,))
    L = float((va.max(axis=0) - va.min(axis=0)).max())
    assert itself["hausdorff"] ** 2 <= REL * L * L and itself["fscore"] == [1.0]
    assert itself["a_to_b"]["normal_consistency"] > 0.99
    assert ds.mesh_distance((va, ta), (vb, tb))["a_to_b"]["normal_consistency"] is None


def test_pipeline(dev):
    import test_mesh_finish_gpu as finish
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.NeRF.distance import mesh_distance, point_mesh_distance
    planes, mlp = finish._planted_scene()
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(mlp, strict=False)
    r = r.to(dev)
    bounds = torch.tensor(syn.WORLD_BOUNDS)
    tp, pl, res = {"world_bounds": bounds[None].to(dev)}, planes.to(dev), 32
    full = r.extract_mesh(tp, pl, resolution=res)
    small = r.extract_mesh(tp, pl, resolution=res, simplify=2)
    cell = 2 * (bounds[1] - bounds[0]).double().numpy() / 31
    diagonal = float(np.linalg.norm(cell))
    kept = small["vertex_map"] >= 0
    hit = point_mesh_distance(full["vertices"][kept], small)
    worst = float(hit["distance"].max())
    score = mesh_distance(full, small, samples=2048, thresholds=(0.25 * diagonal, 0.5 * diagonal))
    print(f"extract_mesh at {res}^3, simplify=2: {len(full['triangles'])} -> {len(small['triangles'])} triangles, cell diagonal {diagonal:.4f}; "
          f"{int(kept.sum())} kept vertices at most {worst / diagonal:.3f} diagonals from the simplified surface; full -> small mean "
          f"{score['a_to_b']['mean'] / diagonal:.4f} max {score['a_to_b']['max'] / diagonal:.4f}, small -> full mean {score['b_to_a']['mean'] / diagonal:.4f} "
          f"max {score['b_to_a']['max'] / diagonal:.4f} diagonals, chamfer {score['chamfer'] / diagonal:.4f}, hausdorff {score['hausdorff'] / diagonal:.4f}, "
          f"f-score at 1/4 and 1/2 diagonal {score['fscore']}, normal consistency {score['a_to_b']['normal_consistency']:.4f} / "
          f"{score['b_to_a']['normal_consistency']:.4f}")
    assert kept.sum() > 100 and worst <= diagonal
