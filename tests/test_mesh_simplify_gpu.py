"""Simplifying a mesh on the MI355X (hl_mesh_simplify.hip) against the numpy restatement (tests/mesh_simplify_restatement.py, which
states the rule - the Cramer order included - once more).  DESIGN.md "Simplifying the mesh".

Bounds.  Cluster ids, counts and colour sums are integers: equal.  A fixed-point sum may differ from the restatement's by one unit per
contribution, for an llrint tie (none is expected: the printed count goes into DESIGN.md).  The representative is compared on the
device's OWN integer sums, in cell units, within 1e-9: the regularised systems have a condition number of at most 3 / lambda + 1 ~ 3000,
float64 rounds at 1.1e-16, a solve is on the order of a hundred operations and |p| <= 1, which gives about 1e-11; two orders of margin.
Normals within 1e-12.  Colours, vertex_map and the triangles - values and order - are equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_simplify_restatement as ms  # noqa: E402

pytestmark = pytest.mark.gpu

VERTEX_TOL = 1e-9          # cell units
NORMAL_TOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def run(v, t, check=True, **kw):
    """simplify._simplify -> the outputs as numpy, plus ids (N,), acc (clusters, 20) and the info dict."""
    from humanliff_amd.NeRF import simplify as sp
    out, scratch, info = sp._simplify(v, t, check=check, **kw)
    got = {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in out.items()}
    if scratch is not None:
        got["ids"] = sp.scratch_cluster_ids(scratch, info["N"]).cpu().numpy()
        got["acc"] = sp.scratch_accumulators(scratch, info["N"], info["clusters"]).cpu().numpy()
    got["info"] = info
    return got


def same_bits(a, b, keys=("vertices", "triangles", "normals", "colors", "vertex_map")):
    return all((a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()) for k in keys)


def against_restatement(name, got, want, v, t):
    """The comparison every case goes through; `want` is ms.simplify of the same mesh."""
    assert got["info"]["clusters"] == len(want["ckey"]) and tuple(got["info"]["extents"]) == tuple(int(x) for x in want["g"]), name
    assert np.array_equal(got["origin"], want["origin"]) and np.array_equal(got["cell"], want["cell"])
    assert np.array_equal(got["ids"], want["ids"]), name
    acc, ref = got["acc"], want["acc"]
    exact = [0, 7, 8, 9]
    assert np.array_equal(acc[:, exact], ref[:, exact]), name
    diff = np.abs(acc - ref)
    room = ms.contributions({"ids": want["ids"], "ckey": want["ckey"]}, t)
    print(f"{name}: {len(t)} -> {len(got['triangles'])} triangles, {len(v)} -> {len(got['vertices'])} vertices of {len(want['ckey'])} clusters; "
          f"fixed-point sums that differ from the restatement: {int((diff != 0).sum())} of {diff.size} (largest {int(diff.max())})")
    assert (diff <= room).all(), name
    # the representatives, from the device's own sums
    p, verts, nrm, col, cond = ms.representatives(acc, want["ckey"], want["g"], want["origin"], want["cell"], got["normals"] is not None,
                                                  got["colors"] is not None)
    used = want["used"]
    assert got["vertices"].dtype == np.float64 and got["vertices"].shape == (int(used.sum()), 3), name
    err = np.abs((got["vertices"] - verts[used]) / want["cell"][None]).max() if used.any() else 0.0
    print(f"{name}: vertices against the restatement on the device's sums: max {err:.3e} cell units (bound {VERTEX_TOL:g}); largest condition number {cond:.1f}")
    assert err <= VERTEX_TOL, name
    if nrm is not None:
        nerr = np.abs(got["normals"] - nrm[used]).max() if used.any() else 0.0
        print(f"{name}: normals max {nerr:.3e} (bound {NORMAL_TOL:g})")
        assert got["normals"].dtype == np.float64 and nerr <= NORMAL_TOL, name
    if col is not None:
        assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], col[used]), name
    assert got["vertex_map"].dtype == np.int64 and np.array_equal(got["vertex_map"], want["vertex_map"]), name
    assert got["triangles"].dtype == np.int64 and np.array_equal(got["triangles"], want["triangles"]), name


# ---- the cases ------------------------------------------------------------------------------------------------------------------
SPACING = 0.01


def _sheet_case():
    v, t, n, c = ms.sheet(24, SPACING, seed=1)
    return v, t, dict(cell=4 * SPACING, normals=n, colors=c)


def _ellipsoid_case(n_lat, n_lon, cell):
    v, t, n = ms.ellipsoid(n_lat, n_lon)
    return v, t, dict(cell=cell, normals=n)


def _doubled_case():
    """(c) the sheet, a copy of it with every vertex moved to another place inside its cell, and the sheet again with every triangle
    reversed: each oriented triple of cells now has at least two triangles, and both orientations occur."""
    v, t, n, c = ms.sheet(24, SPACING, seed=2)
    cell, origin = 4 * SPACING, v.min(axis=0) - 0.001
    rng = np.random.default_rng(12)
    ci = np.floor((v - origin[None]) / cell)
    v2 = origin[None] + (ci + 0.05 + 0.9 * rng.random(v.shape)) * cell
    assert np.array_equal(np.floor((v2 - origin[None]) / cell), ci)
    return (np.concatenate([v, v2]), np.concatenate([t, t + len(v), t[:, ::-1]]),
            dict(cell=cell, origin=origin, normals=np.concatenate([n, n]), colors=np.concatenate([c, c[::-1]])))


def _far_case():
    v, t, n, c = ms.sheet(24, SPACING, seed=3, offset=(1000.0, 1000.0, 1000.0))
    return v, t, dict(cell=(0.04, 0.03, 0.05), origin=(1000.0 - 0.013, 1000.0 - 0.02, 1000.0 - 0.05), normals=n, colors=c)


def _large_triangle_case():
    """(e) a triangle over the sheet's corners, ten cells along each leg: 50 cell areas, so its weight is capped at 1."""
    v, t, n, c = ms.sheet(24, SPACING, seed=4)
    big = np.asarray([[0, 24 * 25, 24]], dtype=np.int64)
    return v, np.concatenate([t[:500], big, t[500:]]), dict(cell=2.4 * SPACING, normals=n, colors=c)


CASES = {"sheet": _sheet_case, "ellipsoid_24x32": functools.partial(_ellipsoid_case, 24, 32, 0.06),
         "ellipsoid_96x128": functools.partial(_ellipsoid_case, 96, 128, 0.04), "doubled": _doubled_case, "far": _far_case,
         "large_triangle": _large_triangle_case}


@pytest.fixture(scope="module")
def restated():
    """(vertices, triangles, keyword arguments, ms.simplify of them) per case, computed once."""
    out = {}
    for name, make in CASES.items():
        v, t, kw = make()
        out[name] = (v, t, kw, ms.simplify(v, t, kw["cell"], kw.get("origin"), kw.get("normals"), kw.get("colors")))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_equals_restatement(name, restated, dev):
    v, t, kw, want = restated[name]
    got = run(v, t, **kw)
    assert got["info"]["status"] == 0 and want["status"] == 0
    against_restatement(name, got, want, v, t)
    out_t = got["triangles"]
    assert len(out_t) > 0 and (out_t[:, 0] < out_t[:, 1]).all() and (out_t[:, 0] < out_t[:, 2]).all() and (out_t[:, 1] != out_t[:, 2]).all()
    assert np.array_equal(np.unique(out_t), np.arange(len(got["vertices"])))
    if name == "ellipsoid_24x32":
        assert len(out_t) == 732
    if name == "ellipsoid_96x128":                 # a cluster no surviving triangle references: the vertices are compacted
        assert (len(out_t), len(got["vertices"])) == (2990, 1495) and got["info"]["clusters"] == 1496 and (~want["used"]).sum() == 1
    if name == "doubled":
        # exactly one survivor per oriented key, and both orientations are kept
        keys = {tuple(r) for r in out_t.tolist()}
        assert len(keys) == len(out_t)
        assert all((a, c, b) in keys for a, b, c in keys)
        _, rot, packed = ms.oriented_keys({"ids": want["ids"]}, t)
        assert len(out_t) == len(np.unique(packed)) < len(packed)
        repeats = np.bincount(np.unique(packed, return_inverse=True)[1])                 # the sheet and its moved copy share every key
        assert repeats.max() >= 2 and (repeats >= 2).sum() >= len(out_t) // 2
    if name == "large_triangle":
        ids = want["ids"]
        big = np.nonzero((t == np.asarray([0, 24 * 25, 24])).all(axis=1))[0]
        assert len(big) == 1 and big[0] in want["survivors"]
        q = (v[t[big[0]]] - want["origin"][None]) / want["cell"][None]
        assert np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0])) / 2.0 > 40.0 and np.ptp(np.floor(q), axis=0).max() >= 9
        assert len(set(ids[t[big[0]]].tolist())) == 3


def test_mesh_inside_one_cell_is_empty(dev):
    v, t, n, c = ms.sheet(4, SPACING, seed=5)
    got = run(v, t, cell=1.0, normals=n, colors=c)
    assert got["info"]["clusters"] == 1 and got["info"]["status"] == 0
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["colors"].shape == (0, 3)
    assert got["triangles"].dtype == np.int64 and got["colors"].dtype == np.uint8
    assert np.array_equal(got["vertex_map"], np.full(len(v), -1, dtype=np.int64))
    assert np.array_equal(got["acc"][0, [0, 7, 8, 9]], [len(v)] + c.astype(np.int64).sum(axis=0).tolist())
    want = ms.simplify(v, t, 1.0, None, n, c)
    assert len(want["ckey"]) == 1 and len(want["triangles"]) == 0 and not want["used"].any()
    assert np.abs(got["acc"] - want["acc"]).max() <= len(t) and got["acc"][0, [10, 13, 15]].sum() > 0      # (its triangles still add their planes)


def test_flagged_vertex_and_index(dev):
    from humanliff_amd.NeRF.simplify import simplify_mesh
    v, t, n, c = ms.sheet(24, SPACING, seed=6)
    N, bad_vertex, bad_triangle = len(v), 137, 300
    assert not (t[bad_triangle] == bad_vertex).any()
    vb, tb = v.copy(), t.copy()
    vb[bad_vertex, 1] = np.nan
    kw = dict(cell=4 * SPACING, normals=n, colors=c)
    with pytest.raises(ValueError, match="non-finite"):
        simplify_mesh(vb, t, **kw)
    for index in (N + 5, -1, 1 << 40):
        tb[bad_triangle, 2] = index
        with pytest.raises(ValueError, match="outside"):
            simplify_mesh(v, tb, **kw)
    got = run(vb, tb, check=False, **kw)
    assert got["info"]["status"] == ms.STATUS_VERTEX | ms.STATUS_INDEX
    # the mesh without them: the vertex deleted, its triangles and the triangle of the bad index removed, the rest renumbered
    keep_v = np.arange(N) != bad_vertex
    keep_t = (t != bad_vertex).all(axis=1) & (np.arange(len(t)) != bad_triangle)
    renumber = np.cumsum(keep_v) - 1
    v2, t2 = v[keep_v], renumber[t[keep_t]]
    want = ms.simplify(v2, t2, kw["cell"], None, n[keep_v], c[keep_v])
    assert got["vertex_map"][bad_vertex] == -1 and got["ids"][bad_vertex] == -1
    trimmed = dict(got, ids=got["ids"][keep_v], vertex_map=got["vertex_map"][keep_v])
    against_restatement("flagged", trimmed, want, v2, t2)
    # and the restatement of the flagged mesh itself says the same
    direct = ms.simplify(vb, tb, kw["cell"], None, n, c)
    assert direct["status"] == ms.STATUS_VERTEX | ms.STATUS_INDEX and np.array_equal(direct["triangles"], got["triangles"])
    assert np.array_equal(direct["vertex_map"], got["vertex_map"])
    # below the origin: the same flag
    with pytest.raises(ValueError, match="below"):
        simplify_mesh(v, t, origin=v.min(axis=0) + 0.05, **kw)


def test_order_independence(restated, dev):
    v, t, kw, _ = restated["doubled"]
    a, b = run(v, t, **kw), run(v, t, **kw)
    assert same_bits(a, b) and np.array_equal(a["acc"], b["acc"]) and np.array_equal(a["ids"], b["ids"])
    rng = np.random.default_rng(3)
    # a permuted triangle list: identical vertices, the same set of triangles
    shuffled = run(v, t[rng.permutation(len(t))], **kw)
    assert same_bits(a, shuffled, ("vertices", "normals", "colors", "vertex_map")) and np.array_equal(a["acc"], shuffled["acc"])
    rows = lambda x: sorted(map(tuple, x.tolist()))  # noqa: E731
    assert rows(a["triangles"]) == rows(shuffled["triangles"]) and not np.array_equal(a["triangles"], shuffled["triangles"])
    # relabelled input vertices: bit-identical vertices, normals and colours (and, the triangles' order being kept, triangles)
    perm = rng.permutation(len(v))                   # new index k holds old vertex perm[k]
    inverse = np.argsort(perm)
    relabelled = run(v[perm], inverse[t], cell=kw["cell"], origin=kw["origin"], normals=kw["normals"][perm], colors=kw["colors"][perm])
    assert same_bits(a, relabelled, ("vertices", "normals", "colors", "triangles"))
    assert np.array_equal(relabelled["vertex_map"], a["vertex_map"][perm])
    # device tensors of another float dtype in, the same bits out (the values are exactly representable)
    v32 = v.astype(np.float32)
    host = run(v32, t, **kw)
    there = run(torch.from_numpy(v32).to(dev), torch.from_numpy(t).to(dev), cell=kw["cell"], origin=kw["origin"],
                normals=torch.from_numpy(kw["normals"]).to(dev), colors=torch.from_numpy(kw["colors"]).to(dev))
    assert same_bits(host, there)


# ---- through the pipeline -----------------------------------------------------------------------------------------------------
def _dilate(mask, r):
    m = torch.from_numpy(mask.astype(np.float32))[None, None]
    return torch.nn.functional.max_pool2d(m, 2 * r + 1, stride=1, padding=r)[0, 0].numpy() > 0


def test_extract_mesh_simplify(dev):
    import test_mesh_finish_gpu as finish
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer, raster
    from humanliff_amd.NeRF.simplify import simplify_mesh
    from humanliff_amd.body import load_body_model
    planes, mlp = finish._planted_scene()
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(mlp, strict=False)
    r = r.to(dev)
    bounds = torch.tensor(syn.WORLD_BOUNDS)
    tp, pl, res = {"world_bounds": bounds[None].to(dev)}, planes.to(dev), 32
    full = r.extract_mesh(tp, pl, resolution=res)
    assert set(full) == {"vertices", "triangles", "normals", "colors", "component_sizes"} and len(full["triangles"]) > 1000
    assert finish._same(full, r.extract_mesh(tp, pl, resolution=res, simplify=None))
    small = r.extract_mesh(tp, pl, resolution=res, simplify=2)
    assert set(small) == set(full) | {"vertex_map"}
    ext, lo = (bounds[1] - bounds[0]).double().numpy(), bounds[0].double().numpy()
    cell = 2 * ext / 31
    want = simplify_mesh(full, cell=cell, origin=lo)
    for k in ("vertices", "triangles", "normals", "colors", "vertex_map"):
        assert small[k].dtype == want[k].dtype and np.array_equal(small[k], want[k]), k
    assert np.array_equal(small["component_sizes"], full["component_sizes"])
    assert 0 < len(small["triangles"]) < len(full["triangles"]) // 3 and small["vertex_map"].shape == (len(full["vertices"]),)
    print(f"extract_mesh at {res}^3: {len(full['triangles'])} triangles, simplify=2: {len(small['triangles'])}")
    with pytest.raises(ValueError, match="simplify"):
        r.extract_mesh(tp, pl, resolution=res, simplify=0.5)
    # bind -> repose -> rasterize takes the simplified mesh as it takes the full one
    model = load_body_model(syn.smpl_like_model(1200, 3), dev)
    poses = (torch.randn((2, 72), generator=syn._gen(5)) * 0.2).to(dev)
    posed = model.pose(poses, torch.zeros(10, device=dev), forward_rows=True)
    binding = r.bind_mesh(small, posed)
    H = W = 128
    K = np.array([[150.0, 0, W / 2.0], [0, 150.0, H / 2.0], [0, 0, 1.0]])
    cam = (K, np.eye(3), np.array([0.0, 0.0, 3.0]))
    moved = binding.rasterize(posed, H, W, *cam)
    assert moved["acc_map"].shape == (2, H, W) and bool(torch.isfinite(moved["rgb_map"]).all())
    # the silhouette: the simplified mesh differs from the full one only within 2 cells of the full mesh's outline
    def acc_of(mesh):
        out = raster.rasterize(mesh["vertices"], mesh["triangles"], H, W, *cam, normals=mesh["normals"], colors=mesh["colors"])
        return out["acc_map"][0].cpu().numpy() > 0, out["depth_map"][0].cpu().numpy()
    acc_full, depth = acc_of(full)
    radius = int(np.ceil(2 * cell.max() * K[0, 0] / depth[acc_full].min()))
    near_outline = _dilate(acc_full, radius) & _dilate(~acc_full, radius)
    restated = ms.simplify(full["vertices"], full["triangles"], cell, lo, full["normals"], full["colors"])
    for name, mesh in (("device", small), ("restatement", restated)):
        acc_small, _ = acc_of(mesh)
        differ = acc_small != acc_full
        print(f"{name}: {int(acc_full.sum())} covered pixels, {int(differ.sum())} differ, all within {radius} pixels of the outline: "
              f"{bool((differ & ~near_outline).sum() == 0)}")
        assert acc_small.sum() > 0.5 * acc_full.sum() and not (differ & ~near_outline).any(), name
