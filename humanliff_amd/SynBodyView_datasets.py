"""Per-view ray generation on the GPU - the ray part of the reference's dataset module
(/root/reference/human_diffusion/SynBodyView_datasets.py), SURVEY.md 8(f) rank 2.

The reference builds every view's rays with numpy on the host (get_rays :316-329, get_near_far :370-403, called from
sample_ray_batch :405-436) and uploads 6.3 MB per 512x512 view; here one kernel writes the same float32 arrays directly
in HBM.  The image / mask half of sample_ray_batch (bound mask, body / background pixel classes, the rejection loop, rgb) runs on the
device as well: recon_NeRF/lib/if_nerf_data_utils.py (ViewStore, sample_ray_batch), which shares this file's per-pixel ray function.
Image files are read and resized by recon_NeRF/lib/SynBody_dataset.py (load_view_store).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _f64(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return a, a.ctypes.data_as(C.c_void_p)


def camera_rays(H, W, K, R, T, bounds, device=None, return_mask=True, split='test'):
    """Rays of one pinhole view, as sample_ray_batch returns them (:422-433):
    rays_o, rays_d (H*W,3) float32, near, far (H*W) float32, mask_at_box (H*W) bool - device tensors.

    K (3,3) intrinsics, R (3,3) / T (3,1) world->camera extrinsics, bounds (2,3) world_bounds; any array-likes.
    Like the reference, exact zeros of rays_d come back as 1e-8 (get_near_far writes them in place, :373) and rays
    that do not cross the 0.01-padded box exactly twice get near=0, far=1.

    split='train' (hl_camera_rays_train) is the arithmetic of the training split of recon_NeRF/lib/if_nerf_data_utils.py (:146-149,
    163-167): get_near_far on the float64 rays, rounded to float32 afterwards - what sample_ray_batch there returns per sampled
    pixel.  The default rounds the rays first, as this file's reference and that module's test split do; near / far of the two
    differ by a few float32 ulp, rays_o / rays_d are the same bits.
    """
    if split not in ('test', 'train'):
        raise ValueError(f"camera_rays: split must be 'test' or 'train', got {split!r}")
    assert int(H) > 0 and int(W) > 0
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    Ki, pKi = _f64(np.linalg.inv(np.asarray(K, dtype=np.float64)), (3, 3))   # :324
    Rm, pR = _f64(R, (3, 3))
    Tm, pT = _f64(T, (3,))
    Bm, pB = _f64(bounds, (2, 3))
    n = int(H) * int(W)
    rays_o = torch.empty((n, 3), device=device, dtype=torch.float32)
    rays_d = torch.empty((n, 3), device=device, dtype=torch.float32)
    near = torch.empty((n,), device=device, dtype=torch.float32)
    far = torch.empty((n,), device=device, dtype=torch.float32)
    mask = torch.empty((n,), device=device, dtype=torch.uint8) if return_mask else None
    with torch.cuda.device(device):
        fn = _lib.lib().hl_camera_rays_train if split == 'train' else _lib.lib().hl_camera_rays
        _lib.check(fn(pKi, pR, pT, pB, int(H), int(W), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(near),
                      _lib.ptr(far), _lib.ptr(mask, torch.uint8) if return_mask else None, _lib.stream_ptr()))
    return rays_o, rays_d, near, far, (mask.bool() if return_mask else None)


def get_rays(H, W, K, R, T, device=None):
    """get_rays (:316-329) -> rays_o, rays_d (H,W,3).  Device float32 (the reference returns host float64 and casts to
    float32 before use, :422-423); bounds are irrelevant here, so a unit box is passed."""
    ro, rd, _, _, _ = camera_rays(H, W, K, R, T, [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], device, return_mask=False)
    return ro.view(H, W, 3), rd.view(H, W, 3)


BIG_GLOBAL_ORIENT = (-3.1416, 0.0, 0.0)          # this twin's big pose for smpl_type 'smplx' (:199)


def prepare_input(body_model, params):
    """prepare_input (:141-182) for smpl_type='smpl' on the device: `params` holds 'poses' (1,72) or (F,72) and 'shapes' (device
    tensors), 'R' (3,3) and 'Th' (1,3) (host arrays, as prepare_smpl_params makes them) -> (world_bounds (2,3), vertices (V,3), params,
    joints (J,3)) as device float32 tensors, with a leading frame axis when poses has more than one row.  The PosedBody behind them
    (tables for the renderer included) is body_model.pose(...) of the same arguments (humanliff_amd/body.py).
    A SmplxModel takes the SMPL-X params of prepare_smpl_params (:128-138: the smplx.npz keys, 'R', 'Th'); as the reference does (:158,
    165-166) the model is run with a zero transl - this twin carries the translation in 'Th' - and 'poses' (the full pose) and 'shapes'
    (betas || expression) are added to `params`."""
    from .body import SmplxModel
    if isinstance(body_model, SmplxModel):
        posed = body_model.pose_dict(dict(params, transl=None), big_global_orient=BIG_GLOBAL_ORIENT)
        params['poses'], params['shapes'] = posed.poses, posed.shapes
    else:
        posed = body_model.pose(params['poses'], params['shapes'], params.get('R'), params.get('Th'))
    if posed.F == 1:
        return posed.world_bounds[0], posed.vertices[0], params, posed.joints[0]
    return posed.world_bounds, posed.vertices, params, posed.joints
