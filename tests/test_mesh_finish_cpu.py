"""Mesh finishing without a GPU: the numpy restatement of the labelling against scipy, the contract of the component filter on the
restated marching cubes, and the PLY attributes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_restatement as gr  # noqa: E402
import mesh_finish_restatement as mf  # noqa: E402

def floaters(n=26):
    """A ball and three floaters of different sizes (one touching the volume face), as a min-of-distances field: above = outside."""
    p = np.indices((n, n + 1, n + 3)).astype(np.float64)
    d = lambda c, r: np.sqrt(sum((p[k] - c[k]) ** 2 for k in range(3))) - r  # noqa: E731
    return np.minimum.reduce([d((12.3, 13.1, 14.2), 7.4), d((3.2, 4.1, 3.3), 2.1), d((22.4, 22.2, 24.9), 2.6), d((21.7, 3.9, 27.6), 1.7)])


@pytest.mark.parametrize("shape,p", mf.BERNOULLI)
def test_restated_labels_equal_scipy(shape, p):
    from scipy import ndimage
    solid = mf.bernoulli(shape, p)
    labels, sizes = mf.label(solid)
    want, n = ndimage.label(solid, structure=np.ones((3, 3, 3)))
    assert n == len(sizes)
    assert np.array_equal(labels, want)
    assert np.array_equal(sizes, np.bincount(want.reshape(-1))[1:])


def test_bernoulli_volumes_do_not_percolate():
    """The densities keep 26-connectivity well below one giant component, so the labelling tests above and on the GPU show something."""
    assert [len(mf.label(mf.bernoulli(shape, p))[1]) for shape, p in mf.BERNOULLI] == [142, 2, 229]


@pytest.mark.parametrize("keep", ["largest", 2, 99, ("min_voxels", 40)])
def test_filter_keeps_exactly_the_triangles_of_kept_components(keep):
    vol = floaters()
    labels, sizes = mf.label_volume(vol, 0.0)
    assert len(sizes) == 4 and len(set(sizes.tolist())) == 4
    kept = mf.select(sizes, keep)
    assert len(kept) == {"largest": 1, 2: 2, 99: 4}.get(keep, int((sizes >= 40).sum()))
    filtered = mf.filter_volume(vol, 0.0, labels, kept)
    untouched = ~((labels > 0) & ~np.isin(labels, kept))
    assert np.array_equal(filtered[untouched], vol[untouched])
    assert (filtered[~untouched] > 0.0).all()
    expect = mf.expected_subset(vol, 0.0, labels, kept, mf.triangle_cells(vol, 0.0))
    full = gr.marching_cubes(vol, 0.0)
    assert 0 < expect.sum() and (keep == 99) == bool(expect.all())
    mf.check_subset(full, gr.marching_cubes(filtered, 0.0), expect)


def test_filter_rule_on_exact_iso_and_nan():
    vol = np.full((3, 3, 7), 1.0)
    vol[1, 1, 0] = 0.0            # solid, exactly iso: |v - iso| = 0 is not above, so the next double above iso
    vol[1, 1, 2] = np.nan         # solid by the corner rule
    vol[1, 1, 4] = -2.5
    vol[1, 1, 6] = -1.0           # two voxels: the largest, and the last label
    vol[1, 2, 6] = -1.0
    out, kept = mf.keep_components(vol, 0.0, "largest")
    assert kept.tolist() == [4]
    assert out[1, 1, 0] == np.nextafter(0.0, 1.0) and out[1, 1, 2] == np.nextafter(0.0, 1.0) and out[1, 1, 4] == 2.5
    assert out[1, 1, 6] == -1.0 and out[1, 2, 6] == -1.0
    assert mf.select(np.array([3, 5, 5, 1]), "largest").tolist() == [2]          # a tie goes to the lower label
    assert mf.select(np.array([3, 5, 5, 1]), 3).tolist() == [1, 2, 3]


def test_restated_normals_of_a_plane_and_a_sphere():
    p = np.indices((12, 13, 14)).astype(np.float64)
    plane = 0.3 * p[0] - 0.5 * p[1] + 0.8 * p[2] - 4.05
    n = mf.vertex_normals(plane, 0.0)
    want = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    assert len(n) > 50 and np.abs(n - want).max() < 1e-12          # differences of a linear field are exact up to roundoff
    n = mf.vertex_normals(plane, 0.0, extent=(2.0, 1.0, 0.5))
    want = np.array([0.15, -0.5, 1.6]) / np.linalg.norm([0.15, -0.5, 1.6])
    assert np.abs(n - want).max() < 1e-12
    assert np.array_equal(mf.vertex_normals(np.where(p[0] < 5, 0.0, 0.0), -1.0), np.zeros((0, 3)))


def test_write_ply_round_trip_with_attributes(tmp_path):
    from humanliff_amd.NeRF import geometry
    rng = np.random.default_rng(0)
    v = rng.standard_normal((50, 3))
    t = rng.integers(0, 50, (80, 3))
    nrm = rng.standard_normal((50, 3))
    col = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    plain, positional = str(tmp_path / "plain.ply"), str(tmp_path / "positional.ply")
    geometry.write_ply(plain, v, t, normals=None, colors=None)
    geometry.write_ply(positional, v, t)
    assert open(plain, "rb").read() == open(positional, "rb").read()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty double x\nproperty double y\nproperty double z\n"
            "element face 80\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    body = open(plain, "rb").read()
    assert body.startswith(head) and body[len(head):len(head) + 1200] == v.astype("<f8").tobytes() and len(body) == len(head) + 1200 + 80 * 13
    out = geometry.read_ply(plain)
    assert len(out) == 2 and np.array_equal(out[0], v) and np.array_equal(out[1], t)
    for kw, extra in (({"normals": nrm, "colors": col}, 2), ({"normals": nrm}, 1), ({"colors": col}, 1)):
        path = str(tmp_path / "attr.ply")
        geometry.write_ply(path, v, t, **kw)
        out = geometry.read_ply(path)
        assert len(out) == 2 + extra and np.array_equal(out[0], v) and np.array_equal(out[1], t)
        rest = list(out[2:])
        if "normals" in kw:
            got = rest.pop(0)
            assert got.dtype == np.float32 and np.array_equal(got, nrm.astype(np.float32))
        if "colors" in kw:
            got = rest.pop(0)
            assert got.dtype == np.uint8 and np.array_equal(got, col)
        text = open(path, "rb").read().split(b"end_header\n")[0].decode()
        assert ("property float nx" in text) == ("normals" in kw) and ("property uchar red" in text) == ("colors" in kw)
    with pytest.raises(ValueError):
        geometry.write_ply(str(tmp_path / "bad.ply"), v, t, normals=nrm[:10])
    with pytest.raises(TypeError):
        geometry.write_ply(str(tmp_path / "bad.ply"), v, t, colors=col.astype(np.float32))


def test_new_entry_points_refuse_cpu_tensors():
    import torch
    from humanliff_amd.NeRF import geometry
    vol = torch.zeros((4, 4, 4), dtype=torch.float64)
    for call in (lambda: geometry.label_components(vol, 0.0), lambda: geometry.keep_components(vol, 0.0, "largest"),
                 lambda: geometry.vertex_normals(vol, 0.0, torch.zeros((0, 3), dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            call()
