"""Host side of the device ray batches (humanliff_amd/recon_NeRF/lib/if_nerf_data_utils.py): the numpy restatement the GPU tests are
measured against is pinned to what the reference itself wrote (tests/golden/ray_batch.npz), and the two pure host functions."""
import os

import numpy as np
import pytest
import torch

from tests import ray_batch_restatement as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_batch.npz")
CASES = ["a", "b", "c", "d", "e"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def within_one_ulp(got, want):
    """The bound of tests/test_render_gpu.py:283-288: at most one float32 ulp, fewer than 1 % of the values differing."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (got != want).mean() < 0.01


def restate(g, name, **kw):
    p = name + "_"
    img = g[p + "img_u8"].astype(np.float32) / 255.
    return rs.sample_ray_batch(img, g[p + "body"], g[p + "K"], g[p + "R"], g[p + "T"], g[p + "bounds"], int(g[p + "n"]), g[p + "picks"], **kw)


def test_golden_cases_serve_their_purpose(golden):
    """a: the rejection loop runs (a second round), b: three rounds, c: one round and nothing rejected, d: a row spans two words and
    the hull's edge is inside the image, e: the hull is clipped by the image border."""
    g = golden
    assert [str(n) for n in g["names"]] == CASES
    assert len(g["a_calls"]) == 4 and len(g["b_calls"]) == 6 and len(g["c_calls"]) == 2
    assert g["c_calls"][:, 1].tolist() == [204, 52]                        # int(256 * 0.8) and the rest
    assert g["a_calls"][:2, 1].tolist() == [204, 52] and 0 < g["a_calls"][2:, 1].sum() < 256     # round 2 redraws what round 1 rejected
    H, W = g["d_HW"]
    assert W > 64 and g["d_bound_mask"][:, 64:].any() and g["d_bound_mask"][:, :64].any()
    assert not g["d_bound_mask"][:, 0].any() and not g["d_bound_mask"][:, -1].any() and not g["d_bound_mask"].all()
    assert int(g["d_n"]) > 256                                             # more than one pass of the workgroup
    bm = g["e_bound_mask"]
    assert (bm[:, 0].any() or bm[:, -1].any()) and not bm.all()
    assert (g["e_corners"].min() < 0) or (g["e_corners"][:, 0].max() >= bm.shape[1])


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference_golden(golden, name):
    g, p = golden, name + "_"
    r = restate(g, name)
    assert np.array_equal(r["corners"], g[p + "corners"])
    assert np.array_equal(r["bound_mask"], g[p + "bound_mask"])
    n = int(g[p + "n"])
    assert r["n_valid"] == n == len(g[p + "near"]) and r["rounds"] == len(g[p + "calls"]) // 2
    c0, c1 = rs.classes(r["bound_mask"], g[p + "body"])
    assert [int(c0.sum()), int(c1.sum())] == g[p + "calls"][:2, 0].tolist()                 # len(np.argwhere(...)) of the two classes
    assert np.array_equal(r["coord"], g[p + "coord"])
    assert np.array_equal(r["bkgd_msk"], g[p + "bkgd_msk"][:, 0])
    assert np.array_equal(r["mask_at_box"], g[p + "mask_at_box"])
    assert np.array_equal(r["rgb"], g[p + "rgb"])
    for k in ("ray_o", "ray_d", "near", "far"):
        within_one_ulp(r[k], g[p + k])


def test_restatement_round_cap(golden):
    """max_rounds below what the reference needed: the rows it did fill, then zeros with near 0 / far 1."""
    g = golden
    r = restate(g, "a", max_rounds=1)
    k = r["n_valid"]
    assert 0 < k < 256 and r["rounds"] == 1
    assert np.array_equal(r["coord"][:k], g["a_coord"][:k]) and not r["coord"][k:].any()
    assert not r["near"][k:].any() and (r["far"][k:] == 1).all() and not r["mask_at_box"][k:].any()


def test_fill_closed_rule():
    """Interior, edges and vertices of a quad are set, the outside is not; a degenerate (collinear) polygon sets its segment."""
    m = np.zeros((8, 9), dtype=np.uint8)
    rs.fill_closed(m, [[1, 1], [6, 1], [6, 5], [1, 5], [1, 1]])
    want = np.zeros_like(m)
    want[1:6, 1:7] = 1
    assert np.array_equal(m, want)
    m = np.zeros((8, 9), dtype=np.uint8)
    rs.fill_closed(m, [[0, 0], [3, 3], [6, 6], [3, 3]])
    assert np.array_equal(np.argwhere(m), [[i, i] for i in range(7)])
    m = np.zeros((7, 7), dtype=np.uint8)
    rs.fill_closed(m, [[3, 0], [6, 3], [3, 6], [0, 3]])                     # a diamond: lattice points with |x - 3| + |y - 3| <= 3
    yy, xx = np.mgrid[0:7, 0:7]
    assert np.array_equal(m.astype(bool), np.abs(xx - 3) + np.abs(yy - 3) <= 3)


@pytest.mark.parametrize("name", CASES)
def test_bound_corners_2d(golden, name):
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import bound_corners_2d
    g, p = golden, name + "_"
    got = bound_corners_2d(g[p + "bounds"], g[p + "K"], g[p + "R"], g[p + "T"])
    assert got.shape == (8, 2) and got.dtype == np.int64 and np.array_equal(got, g[p + "corners"])


def test_bound_corners_2d_refuses_a_corner_on_the_camera_plane():
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import bound_corners_2d
    with pytest.raises(ValueError):
        bound_corners_2d([[-1, -1, -1], [1, 1, 1]], np.eye(3), np.eye(3), [0.0, 0.0, 1.0])      # the z = -1 corners have depth 0


def test_epoch_order():
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import epoch_order
    a = epoch_order(37, 3, 0)
    assert a.dtype == torch.int64 and sorted(a.tolist()) == list(range(37))
    assert torch.equal(a, epoch_order(37, 3, 0))
    b = epoch_order(37, 3, 1)
    assert sorted(b.tolist()) == list(range(37)) and not torch.equal(a, b)
    assert not torch.equal(a, epoch_order(37, 4, 0))
