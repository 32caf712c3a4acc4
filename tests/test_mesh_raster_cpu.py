"""The mesh rasteriser without a device: the numpy restatement's own rules (tests/mesh_raster_restatement.py) on examples small enough
to check by hand, the names of the C ABI, and the argument checks of humanliff_amd/NeRF/raster.py that run before any launch.
DESIGN.md "Rasterising the mesh"."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from tests import mesh_raster_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_written_4x4():
    """Three triangles on pixel centres (coordinates in pixels, x right, y down):
         0: (0,0) (3,0) (3,3)   1: (0,0) (3,3) (0,3)   2: (3,0) (3,3) (6,0), wound the other way (A < 0: drawn with 1 and 2 swapped).
    The diagonal (1,1), (2,2) is the edge 0 and 1 share: its direction in triangle 0 is (-3,-3), dy < 0, owned there.  (0,0) is a vertex
    of both: triangle 0's edges through it are both owned (the diagonal, and the top edge (3,0): dy == 0, dx > 0).  Column x = 3 is the
    edge 0 and 2 share: direction (0,3) in triangle 0 (not owned), (0,-3) in triangle 2 (owned); (3,0) is a vertex of both and goes
    with the column.  Row y = 3 is a bottom edge (direction (-3,0)): nobody's, so (3,3), a vertex of all three, stays background."""
    P = np.array([[0, 0], [3, 0], [3, 3], [0, 3], [6, 0]], dtype=np.int64) * mr.SUB
    X, Y = P[:, 0].copy(), P[:, 1].copy()
    z = np.full(5, 2.0, np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 4]])
    c = mr.cover(X, Y, z, tri, 4, 4)
    want = np.array([[0, 0, 0, 2],
                     [1, 0, 0, 2],
                     [1, 1, 0, 2],
                     [-1, -1, -1, -1]])
    assert np.array_equal(c["id"], want)
    assert np.array_equal(c["hits"], (want >= 0).astype(np.int64))               # shared edges and vertices: one owner each
    assert np.array_equal(c["depth"], np.where(want >= 0, 2.0, 0.0))
    assert np.array_equal(mr.drawn(X, Y, np.zeros(5, bool), tri, cull="back"), [True, True, False])
    assert np.array_equal(mr.drawn(X, Y, np.zeros(5, bool), tri, cull="front"), [False, False, True])
    # weights: at (1,0) of triangle 0 - a third of the way along its top edge - they are (2/3, 1/3, 0) and sum to 1
    K = np.eye(3)
    r = mr.resolve(X, Y, z, tri, c["id"], c["depth"], np.zeros((5, 3), np.float32), K, np.eye(3), np.zeros(3), colors=None)
    assert np.allclose(r["barycentrics"][0, 1], [2 / 3, 1 / 3, 0.0], atol=1e-15)
    assert np.abs(r["barycentrics"][want >= 0].sum(axis=1) - 1.0).max() < 1e-15
    # triangle 2 was drawn with vertices 1 and 2 swapped; its weights come back in its own order: pixel (3,1) is a third of the way 1 -> 2
    assert np.allclose(r["barycentrics"][1, 3], [2 / 3, 1 / 3, 0.0], atol=1e-15)


def test_ownership_holds_for_exactly_one_direction():
    g = np.arange(-7, 8)
    dx, dy = np.meshgrid(g, g)
    nz = (dx != 0) | (dy != 0)
    assert (mr.owned(dx, dy)[nz] ^ mr.owned(-dx, -dy)[nz]).all()
    big = np.array([1 << 28, -(1 << 28), 1, -1, 0])
    dx, dy = np.meshgrid(big, big)
    nz = (dx != 0) | (dy != 0)
    assert (mr.owned(dx, dy)[nz] ^ mr.owned(-dx, -dy)[nz]).all()


def test_one_sheet_is_hit_once():
    """A wavy one-sheet grid of 3 200 micro-triangles at 67 x 48: no cracks (every pixel inside the outline is hit) and no double hits."""
    H, W = 48, 67
    K, R, T = mr.scene_camera(H, W)
    v, tri = mr.sheet(40, seed=3)
    X, Y, z, bad = mr.project(v, K, R, T)
    assert not bad.any()
    c = mr.cover(X, Y, z, tri, H, W, invalid=bad)
    assert set(np.unique(c["hits"])) == {0, 1}
    assert 900 < (c["hits"] == 1).sum() < H * W                                  # (0.9 m across at depth 2, focal 70: about 31 x 31 pixels)
    # no cracks: a covered pixel's four neighbours are covered unless the pixel is on the outline - the hit mask equals its own
    # fill, row by row (the sheet's image is convex enough in this camera: each row's hits are one run)
    for row in c["hits"]:
        xs = np.nonzero(row)[0]
        assert xs.size == 0 or row[xs[0]:xs[-1] + 1].all()
    c32 = mr.cover(X, Y, z, tri, H, W, dtype=np.float32, invalid=bad)
    assert np.array_equal(c32["id"], c["id"]) and c32["depth"].dtype == np.float32
    e = np.abs(c32["depth"].astype(np.float64) - c["depth"]).max()
    assert 0 < e < 2e-6                                                          # depths about 2: a few fp32 ulp of 2.4e-7


def test_projection_flags_and_convention():
    """A point on the ray of pixel (20, 10) - camera_rays' convention: K^-1 (px, py, 1), no half-pixel offset - at camera z 2 lands on
    (256 * 20, 256 * 10) with z 2 (to the fp32 rounding of the vertex); one behind the camera, a NaN and one outside the guard band
    are invalid and their records are zero."""
    H, W = 48, 67
    K, R, T = mr.scene_camera(H, W)
    o = mr.camera_centre(R, T)
    d = mr.ray_directions(H, W, K, R, T)
    pts = np.stack([o + 2.0 * d[10, 20] / (R @ d[10, 20])[2], o - 1.0 * d[10, 20], np.full(3, np.nan), o + 1e-2 * d[10, 20] + R.T @ np.array([1e5, 0, 0])])
    X, Y, z, bad = mr.project(pts.astype(np.float32), K, R, T)
    assert list(bad) == [False, True, True, True]
    assert abs(int(X[0]) - 20 * 256) <= 1 and abs(int(Y[0]) - 10 * 256) <= 1 and abs(float(z[0]) - 2.0) < 1e-6
    assert (X[1:] == 0).all() and (z[1:] == 0).all()


def test_the_interface_is_there():
    from humanliff_amd import _lib
    from humanliff_amd.NeRF import animate, raster, rasterize
    header = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in ("hl_mesh_raster", "hl_mesh_raster_scratch_bytes", "hl_mesh_raster_small_box"):
        assert name + "(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["hl_mesh_raster"][1]) == 25 and _lib.SIGNATURES["hl_mesh_raster_scratch_bytes"][1] == [_lib._i64, _lib._i64] + [_lib._i] * 3
    assert f"#define HL_RASTER_CAM_ROW {_lib.HL_RASTER_CAM_ROW}" in header
    assert rasterize is raster.rasterize
    assert list(inspect.signature(raster.rasterize).parameters)[:14] == [
        "vertices", "triangles", "H", "W", "K", "R", "T", "normals", "colors", "shade", "white_bkgd", "cull", "znear", "check_indices"]
    p = inspect.signature(raster.rasterize).parameters
    assert (p["shade"].default, p["white_bkgd"].default, p["cull"].default, p["znear"].default, p["check_indices"].default) == \
        ("colors", False, None, 1e-3, True)
    assert list(inspect.signature(animate.MeshBinding.rasterize).parameters)[:8] == ["self", "posed", "H", "W", "K", "R", "T", "frames"]


def test_rasterize_argument_errors():
    """All raised before the device is touched (this test runs without one)."""
    from humanliff_amd.NeRF import raster
    I3, Z3 = np.eye(3), np.zeros(3)
    v, tri = np.zeros((5, 3)), np.array([[0, 1, 2], [2, 3, 4]])
    ok = dict(H=4, W=6, K=I3, R=I3, T=Z3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.rasterize(torch.zeros((5, 3)), tri, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.rasterize(v, torch.from_numpy(tri), **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.rasterize(v, tri, normals=torch.zeros((5, 3)), **ok)
    for bad in (np.zeros((2, 4), np.int64), np.zeros((6,), np.int64), np.zeros((1, 2, 3), np.int64)):
        with pytest.raises(ValueError, match=r"\(T,3\)"):
            raster.rasterize(v, bad, **ok)
    with pytest.raises(ValueError, match="integer dtype"):
        raster.rasterize(v, tri.astype(np.float32), **ok)
    with pytest.raises(ValueError, match="triangles"):
        raster.rasterize(v, np.zeros((0, 3), np.int64), **ok)
    # F frames against C cameras: equal, or one of them 1
    for Fv, C in ((2, 3), (3, 2), (4, 3)):
        with pytest.raises(ValueError, match="frames and .* cameras"):
            raster.rasterize(np.zeros((Fv, 5, 3)), tri, 4, 6, np.stack([I3] * C), I3, Z3)
    with pytest.raises(ValueError, match="each must be one or all"):
        raster.rasterize(v, tri, 4, 6, np.stack([I3] * 3), np.stack([I3] * 2), Z3)
    with pytest.raises(ValueError, match="T must be"):
        raster.rasterize(v, tri, 4, 6, I3, I3, np.zeros(4))
    with pytest.raises(ValueError, match="vertices"):
        raster.rasterize(np.zeros((5, 2)), tri, **ok)
    with pytest.raises(ValueError, match="normals"):
        raster.rasterize(v, tri, normals=np.zeros((4, 3)), **ok)
    with pytest.raises(ValueError, match="colors"):
        raster.rasterize(v, tri, colors=np.zeros((5, 3), np.float32), **ok)
    with pytest.raises(ValueError, match="shade"):
        raster.rasterize(v, tri, shade="phong", **ok)
    with pytest.raises(ValueError, match="cull"):
        raster.rasterize(v, tri, cull="both", **ok)
    with pytest.raises(ValueError, match="znear"):
        raster.rasterize(v, tri, znear=0.0, **ok)
    with pytest.raises(ValueError, match="image size"):
        raster.rasterize(v, tri, 0, 6, I3, I3, Z3)
    with pytest.raises(np.linalg.LinAlgError):                                   # (a ValueError)
        raster.rasterize(v, tri, 4, 6, np.zeros((3, 3)), I3, Z3)
    assert issubclass(np.linalg.LinAlgError, ValueError)


def test_binding_without_triangles_raises():
    from humanliff_amd.NeRF import animate
    b = animate.MeshBinding()
    posed = types.SimpleNamespace()
    with pytest.raises(ValueError, match="no triangles"):
        b.rasterize(posed, 4, 6, np.eye(3), np.eye(3), np.zeros(3))
    b.triangles = np.zeros((0, 3), np.int64)
    with pytest.raises(ValueError, match="no triangles"):
        b.rasterize(posed, 4, 6, np.eye(3), np.eye(3), np.zeros(3))
