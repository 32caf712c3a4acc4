"""Mesh extraction, host side: the baked marching-cubes table against the restatement's independent face walk, closedness of the
restated meshes over every 2x2x2 corner configuration, the restatement's EDT against scipy, the PLY writer and the no-CPU rule."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_restatement as gr  # noqa: E402


@pytest.fixture(scope="module")
def baked():
    from humanliff_amd.build import build
    build()
    from humanliff_amd.NeRF import geometry
    return geometry.case_table()


def test_baked_table_equals_restated_face_walk(baked):
    want = gr.case_table()
    for c in range(256):
        assert baked[c] == want[c], f"case {c}: baked {baked[c]} restated {want[c]}"
    assert baked[0] == [] and baked[255] == []
    assert baked[1] == [(0, 8, 4)]                         # corner 0 alone: normal toward the corner
    assert max(len(t) for t in baked) == 5


def test_committed_table_header_is_generated():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_mc_table.py"), "--check"])
    assert r.returncode == 0, "humanliff_amd/csrc/hl_mc_table.h differs from scripts/gen_mc_table.py's output"


def _edge_uses(tris):
    directed = {}
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            directed[(int(a), int(b))] = directed.get((int(a), int(b)), 0) + 1
    return directed


def _block(cfg, outside):
    v = np.full((4, 4, 4), outside)
    for c in range(8):
        v[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + ((c >> 2) & 1)] = 1.0 if (cfg >> c) & 1 else -1.0
    return v


def _closed(tris, manifold):
    uses = _edge_uses(tris)
    for (a, b), k in uses.items():
        if manifold:
            assert k == 1 and uses.get((b, a)) == 1, f"edge {(a, b)} used {k} / {uses.get((b, a))} times"
        else:
            assert uses.get((b, a)) == k, f"edge {(a, b)} used {k} times, reversed {uses.get((b, a))}"


def test_restated_mesh_closed_for_every_block():
    """Each of the 256 corner configurations (ambiguous faces and checkers included) inside a 4^3 volume whose border is below:
    every undirected edge of the mesh is used exactly twice, once in each direction.  With the border above, every edge is still
    used as often in one direction as in the other (closed, consistently oriented); 18 configurations there meet the fan rule's
    pinch - a fan diagonal lying in a face that the neighbouring cube's fan also draws (mesh extraction)."""
    pinched = []
    for cfg in range(256):
        verts, tris = gr.marching_cubes(_block(cfg, -1.0), 0.0)
        assert len(tris) > 0 or cfg == 0
        _closed(tris, manifold=True)
        assert len(np.unique(tris)) == len(verts) or cfg == 0
        verts, tris = gr.marching_cubes(_block(cfg, 1.0), 0.0)
        _closed(tris, manifold=False)
        try:
            _closed(tris, manifold=True)
        except AssertionError:
            pinched.append(cfg)
    assert len(pinched) == 18


@pytest.mark.parametrize("outside", [-1.0, 1.0])
@pytest.mark.parametrize("parity", [0, 1])
def test_restated_mesh_closed_for_checker_blocks(outside, parity):
    """A 3^3 checkerboard (2x2x2 cubes, every face ambiguous) padded with below or above values: a closed 2-manifold."""
    v = np.full((5, 5, 5), outside)
    v[1:4, 1:4, 1:4] = np.where(np.indices((3, 3, 3)).sum(0) % 2 == parity, 1.0, -1.0)
    _, tris = gr.marching_cubes(v, 0.0)
    assert len(tris) > 0
    _closed(tris, manifold=True)


def test_restated_edt_equals_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(4)
    for shape, p in [((13, 9, 17), 0.05), ((20, 20, 20), 0.5), ((1, 11, 6), 0.2), ((16, 5, 9), 0.93)]:
        b = rng.random(shape) < p
        assert (gr.edt(b) == ndimage.distance_transform_edt(b)).all()
        assert (gr.edt(~b) == ndimage.distance_transform_edt(~b)).all()


def test_write_ply_round_trip(tmp_path):
    from humanliff_amd.NeRF import geometry
    rng = np.random.default_rng(1)
    v = rng.standard_normal((37, 3))
    t = rng.integers(0, 37, (50, 3))
    p = tmp_path / "m.ply"
    geometry.write_ply(str(p), v, t)
    v2, t2 = geometry.read_ply(str(p))
    assert np.array_equal(v, v2) and np.array_equal(t, t2)
    assert open(p, "rb").read(40).startswith(b"ply\nformat binary_little_endian 1.0\n")


def test_geometry_refuses_cpu_tensors():
    from humanliff_amd.NeRF import geometry
    v = torch.randn(8, 8, 8, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        geometry.smooth_constrained(v)
    with pytest.raises(RuntimeError):
        geometry.smooth(v)
    with pytest.raises(RuntimeError):
        geometry.marching_cubes(v, 0.0)
