"""Held-out view scores on the device: masked MSE / PSNR, the mask's bounding rectangle and SSIM on the crop, as the reference's test
mode computes them on the host (recon_NeRF/lib/all_test.py:19-42 psnr_metric / ssim_metric, :175-188) - hl_image_metrics
(csrc/hl_metrics.hip; contract: DESIGN.md "Evaluation").  There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib

WIN_SIZE = 7                # skimage's default window: a crop narrower or lower than this has no SSIM

# The reference calls skimage's structural_similarity on float64 images WITHOUT data_range (all_test.py:37).  The skimage of its pinned
# environment then takes the dtype range of a float image, (-1, 1): R = 2 - although the images live in [0, 1].  That is the number
# its papers' tables hold, so it is the default here; pass data_range=1.0 for the SSIM of [0, 1] images.
REFERENCE_DATA_RANGE = 2.0


def _views(pred, gt, mask):
    for name, t in (("pred", pred), ("gt", gt), ("mask", mask)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"image_metrics: {name} must be a HIP tensor; humanliff_amd has no CPU path")
    if pred.dim() == 3:
        pred, gt, mask = pred[None], gt[None], mask[None]
    if pred.dim() != 4 or pred.shape[-1] != 3 or gt.shape != pred.shape or tuple(mask.shape) != tuple(pred.shape[:3]):
        raise RuntimeError(f"image_metrics: pred and gt must be (V, H, W, 3) or (H, W, 3) and mask (V, H, W) or (H, W); got "
                           f"{tuple(pred.shape)}, {tuple(gt.shape)}, {tuple(mask.shape)}")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"image_metrics: pred and gt must be float32 and mask bool or uint8; got {pred.dtype}, {gt.dtype}, {mask.dtype}")
    if gt.device != pred.device or mask.device != pred.device:
        raise RuntimeError("image_metrics: pred, gt and mask must be on one device")
    mask = mask.contiguous()
    return pred.contiguous(), gt.contiguous(), (mask.view(torch.uint8) if mask.dtype == torch.bool else mask)


def image_records(pred, gt, mask, data_range=REFERENCE_DATA_RANGE, return_uint8=False):
    """The raw records of hl_image_metrics: a (V, 6) float64 device tensor whose rows are hl_metrics_record (mse, psnr, ssim, then
    count, x, y, w, h as int32), and the two uint8 images or None.  Enqueue-only."""
    pred, gt, mask = _views(pred, gt, mask)
    V, H, W, _ = pred.shape
    dev = pred.device
    L = _lib.lib()
    rec = torch.empty((V, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(max(L.hl_image_metrics_workspace_bytes(V, H, W), 8) // 8, dtype=torch.float64, device=dev)
    pred_u8 = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
    gt_u8 = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
    with _lib.on(dev):
        _lib.check(L.hl_image_metrics(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(mask, torch.uint8), V, H, W, float(data_range), 0,
                                      _lib.ptr(pred_u8, torch.uint8), _lib.ptr(gt_u8, torch.uint8), C.c_void_p(rec.data_ptr()),
                                      C.c_void_p(ws.data_ptr()), ws.numel() * 8, _lib.stream_ptr(dev)), "hl_image_metrics")
    return rec, pred_u8, gt_u8


def split_records(rec):
    """{mse, psnr, ssim, count, bbox} as views of a (V, 6) float64 record tensor (device or host); bbox is (V, 4) int32: x, y, w, h."""
    ints = rec.view(torch.int32)
    return {"mse": rec[:, 0], "psnr": rec[:, 1], "ssim": rec[:, 2], "count": ints[:, 6], "bbox": ints[:, 7:11]}


def image_metrics(pred, gt, mask, data_range=REFERENCE_DATA_RANGE, return_uint8=False):
    """Scores of V views: pred, gt (V, H, W, 3) or (H, W, 3) float32, mask (V, H, W) or (H, W) bool / uint8 (mask_at_box), all on the
    device.  Returns device tensors of leading size V: mse, psnr, ssim (float64), count (int32), bbox (int32 x, y, w, h), and with
    return_uint8 also pred_u8 (to8b of the masked prediction) and gt_u8 (to8b of the unmasked ground truth).  Nothing is read back:
    ssim is NaN for a view whose crop is smaller than the 7 x 7 window (image_metrics_host raises for it)."""
    rec, pred_u8, gt_u8 = image_records(pred, gt, mask, data_range, return_uint8)
    out = split_records(rec)
    if return_uint8:
        out["pred_u8"], out["gt_u8"] = pred_u8, gt_u8
    return out


def records_to_host(rec):
    """One device-to-host copy of a record tensor -> numpy arrays {mse, psnr, ssim, count, bbox}.  Raises ValueError for a view whose
    crop is smaller than the window, as skimage does for such an image."""
    host = split_records(rec.cpu())
    out = {k: v.numpy().copy() for k, v in host.items()}
    for v, (x, y, w, h) in enumerate(out["bbox"]):
        if w < WIN_SIZE or h < WIN_SIZE:
            raise ValueError(f"view {v}: the mask's bounding rectangle is {w} x {h} (w x h), smaller than the {WIN_SIZE} x {WIN_SIZE} "
                             "SSIM window: win_size exceeds image extent")
    return out


def image_metrics_host(pred, gt, mask, data_range=REFERENCE_DATA_RANGE, return_uint8=False):
    """image_metrics, read back once: numpy arrays (the uint8 images too, with return_uint8).  ValueError names the view whose crop is
    smaller than the window."""
    rec, pred_u8, gt_u8 = image_records(pred, gt, mask, data_range, return_uint8)
    out = records_to_host(rec)
    if return_uint8:
        out["pred_u8"], out["gt_u8"] = pred_u8.cpu().numpy(), gt_u8.cpu().numpy()
    return out
