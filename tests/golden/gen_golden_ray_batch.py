"""Generate golden vectors for the training ray batches FROM THE REFERENCE.

Runs only in the build container (needs /root/reference).

    python tests/golden/gen_golden_ray_batch.py

Reference entry point exercised (unmodified, imported from /root/reference/recon_NeRF/lib/if_nerf_data_utils.py):
    sample_ray_batch(..., split='train')   :87-170, and through it get_rays, get_bound_2d_mask, project, get_near_far
Two things are supplied from outside:
  * cv2 is not installed, so a stub module provides fillPoly: the closed integer fill of tests/ray_batch_restatement.py (DESIGN.md 4g;
    cv2's own outline pixels could not be compared);
  * np.random.randint is wrapped so that every call's (high, size) and values are recorded - they become the injected `picks`.
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference/recon_NeRF/lib")

from tests import ray_batch_restatement as rs  # noqa: E402

cv2 = types.ModuleType("cv2")


def _fill_poly(mask, polys, value):
    for p in polys:
        rs.fill_closed(mask, p, value)
    return mask


cv2.fillPoly = _fill_poly
sys.modules["cv2"] = cv2

import if_nerf_data_utils as D  # noqa: E402

from humanliff_amd import synthetic as syn  # noqa: E402

CALLS = []
_randint = np.random.randint


def _recording_randint(low, high=None, size=None, *a, **k):
    v = _randint(low, high, size, *a, **k)
    CALLS.append((int(high), int(size), np.asarray(v).copy()))
    return v


np.random.randint = _recording_randint

NARROW = [[-0.6, -0.9, -0.6], [0.6, 0.9, 0.6]]


def cases():
    """name, H, W, view, n_views, bounds, camera shift along its right axis, n rays, numpy seed."""
    return [("a", 64, 64, 1, 8, syn.WORLD_BOUNDS, 0.0, 256, 5),      # azimuth 45 deg: the principal column is rejected -> the loop repeats
            ("b", 48, 48, 1, 8, syn.WORLD_BOUNDS, 0.0, 256, 0),      # the same view, coarser; with this seed three rounds
            ("c", 64, 64, 0, 8, syn.WORLD_BOUNDS, 0.0, 256, 5),      # one round, nothing rejected
            ("d", 48, 80, 3, 36, NARROW, 0.0, 300, 7),               # hull edge inside the image; a row spans two 64-bit words; two chunks
            ("e", 64, 64, 2, 8, syn.WORLD_BOUNDS, 1.1, 128, 9)]      # the hull is clipped by the image border


def make_case(H, W, view, n_views, bounds, shift, seed):
    K, c2w, cam = syn.orbit_camera(view, n_views, H, W)
    cam = cam + shift * c2w[:, 0]
    R = c2w.T.copy()
    T = (-R @ cam).reshape(3, 1)
    rng = np.random.RandomState(100 + seed)
    img_u8 = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    body = ((((xx - W / 2.0) / (0.22 * W)) ** 2 + ((yy - H / 2.0) / (0.36 * H)) ** 2) <= 1.0).astype(np.uint8)
    return K, R, T, np.asarray(bounds, dtype=np.float64), img_u8, body


def main():
    data, names = {}, []
    for name, H, W, view, n_views, bounds, shift, n, seed in cases():
        K, R, T, b, img_u8, body = make_case(H, W, view, n_views, bounds, shift, seed)
        img = img_u8.astype(np.float32) / 255.                      # what imageio.imread(...).astype(np.float32) / 255. gives
        del CALLS[:]
        np.random.seed(seed)
        rgb, ray_o, ray_d, near, far, coord, mask_at_box, bkgd_msk = D.sample_ray_batch(img.copy(), body.copy(), K.copy(), R.copy(), T.copy(),
                                                                                      b.copy(), n, 'train')
        assert len(CALLS) % 2 == 0
        rounds = len(CALLS) // 2
        picks = np.zeros((rounds, 2, n), dtype=np.int32)
        for i, (high, size, v) in enumerate(CALLS):
            picks[i // 2, i % 2, :size] = v
        pose = np.concatenate([R, T], axis=1)
        corners = np.round(D.project(D.get_bound_corners(b), K, pose)).astype(int)
        bmask = D.get_bound_2d_mask(b, K, pose, H, W)
        names.append(name)
        p = name + "_"
        data[p + "HW"], data[p + "K"], data[p + "R"], data[p + "T"], data[p + "bounds"] = np.array([H, W]), K, R, T, b
        data[p + "img_u8"], data[p + "body"], data[p + "n"] = img_u8, body, np.array(n)
        data[p + "corners"], data[p + "bound_mask"] = corners.astype(np.int64), bmask
        data[p + "calls"] = np.array([[h, s] for h, s, _ in CALLS], dtype=np.int64)
        data[p + "picks"] = picks
        data[p + "rgb"], data[p + "ray_o"], data[p + "ray_d"], data[p + "near"], data[p + "far"] = rgb, ray_o, ray_d, near, far
        data[p + "coord"], data[p + "mask_at_box"], data[p + "bkgd_msk"] = coord, mask_at_box, bkgd_msk
        print(name, f"{H}x{W}", "rounds", rounds, "calls", [(h, s) for h, s, _ in CALLS], "bound", int(bmask.sum()),
              "body&bound", int((bmask * body).sum()), "rows", len(near))
    data["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "ray_batch.npz"), **data)


if __name__ == "__main__":
    main()
