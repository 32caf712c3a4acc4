"""Raw views -> the arrays a ViewStore holds, on the device (csrc/hl_view_ingest.hip; contract: DESIGN.md 4i).

The reference prepares every image in a DataLoader worker (recon_NeRF/lib/SynBody_dataset.py:266-278): imread / 255, img[msk == 0] = 0,
cv2.resize(INTER_AREA) of the image and cv2.resize(INTER_NEAREST) of the mask.  Here the uint8 source goes to the device as it is and one
launch writes the float32 image and the body mask of every view of the batch.

    image, body = ingest_views(img_u8, msk_u8, H, W)      # (V, Hs, Ws, 3), (V, Hs, Ws) uint8 device tensors -> (V, H, W, 3) f32, (V, H, W) u8

The tap tables of the resize rule are built on the host (area_taps, nearest_taps: plain C++, callable without a GPU) and uploaded once per
(Hs, Ws, H, W) and device.  There is no CPU path for the images.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_tables = {}          # (device, Hs, Ws, H, W) -> (xtab, ytab) device int32 tensors


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def check_sizes(Hs, Ws, H, W):
    """ValueError for a target that is empty or enlarges an axis: cv2.resize switches to a bilinear variant there, which is not restated."""
    Hs, Ws, H, W = int(Hs), int(Ws), int(H), int(W)
    if min(Hs, Ws, H, W) <= 0:
        raise ValueError(f"view ingest: bad sizes {Hs} x {Ws} -> {H} x {W}")
    if H > Hs or W > Ws:
        raise ValueError(f"view ingest: {Hs} x {Ws} -> {H} x {W} enlarges an axis; the INTER_AREA rule is restated for reductions only "
                         "(image_scaling <= 1)")
    return Hs, Ws, H, W


def area_taps(src, dst):
    """One axis of the INTER_AREA rule, src -> dst <= src: (idx (dst, T) int32, w (dst, T) float32, count (dst) int32), T = ceil(src / dst) + 1;
    output d is sum_k<count[d] w[d, k] * source[idx[d, k]].  Host."""
    src, dst = int(src), int(dst)
    if not 0 < dst <= src:
        raise ValueError(f"area_taps: {src} -> {dst} is not a reduction")
    L = _lib.lib()
    T = L.hl_area_max_taps(src, dst)
    idx, w, count = np.empty((dst, T), dtype=np.int32), np.empty((dst, T), dtype=np.float32), np.empty((dst,), dtype=np.int32)
    _lib.check(L.hl_area_taps(src, dst, T, _np_ptr(idx), _np_ptr(w), _np_ptr(count)), "hl_area_taps")
    return idx, w, count


def nearest_taps(src, dst):
    """One axis of the INTER_NEAREST rule: (dst,) int32 source indices.  Host."""
    idx = np.empty((int(dst),), dtype=np.int32)
    _lib.check(_lib.lib().hl_nearest_taps(int(src), int(dst), _np_ptr(idx)), "hl_nearest_taps")
    return idx


def packed_table(src, dst):
    """The int32 words hl_view_ingest reads for one axis: count | nearest | idx | weight bits.  Host."""
    L = _lib.lib()
    words = L.hl_view_ingest_table_words(int(src), int(dst))
    if words == 0:
        raise ValueError(f"packed_table: {src} -> {dst} is not a reduction")
    table = np.empty((words,), dtype=np.int32)
    _lib.check(L.hl_view_ingest_table(int(src), int(dst), _np_ptr(table)), "hl_view_ingest_table")
    return table


def device_tables(Hs, Ws, H, W, device):
    """(xtab, ytab) on `device`, uploaded once per size."""
    device = torch.device(device)
    key = (str(device), Hs, Ws, H, W)
    if key not in _tables:
        _tables[key] = (torch.from_numpy(packed_table(Ws, W)).to(device), torch.from_numpy(packed_table(Hs, H)).to(device))
    return _tables[key]


def ingest_views(img_u8, msk_u8, H, W):
    """img_u8 (V, Hs, Ws, 3), msk_u8 (V, Hs, Ws): contiguous uint8 device tensors -> image (V, H, W, 3) float32 in [0, 1] with the pixels
    outside the mask zeroed before the reduction, body (V, H, W) uint8 of 0 / 1.  Enqueue-only on the current stream."""
    if not (torch.is_tensor(img_u8) and torch.is_tensor(msk_u8) and img_u8.is_cuda and msk_u8.is_cuda):
        raise RuntimeError("ingest_views needs device tensors; humanliff_amd has no CPU path")
    if img_u8.dtype != torch.uint8 or msk_u8.dtype != torch.uint8:
        raise TypeError(f"ingest_views: images and masks must be uint8, got {img_u8.dtype}, {msk_u8.dtype}")
    if img_u8.dim() != 4 or img_u8.shape[3] != 3 or tuple(msk_u8.shape) != tuple(img_u8.shape[:3]) or img_u8.shape[0] < 1:
        raise ValueError(f"ingest_views: images must be (V, Hs, Ws, 3) and masks (V, Hs, Ws); got {tuple(img_u8.shape)}, {tuple(msk_u8.shape)}")
    V, Hs, Ws = (int(s) for s in msk_u8.shape)
    Hs, Ws, H, W = check_sizes(Hs, Ws, H, W)
    dev = img_u8.device
    img_u8, msk_u8 = img_u8.contiguous(), msk_u8.contiguous()
    if img_u8.data_ptr() % 16 or msk_u8.data_ptr() % 16:              # (a slice of a larger batch: the kernel's wide loads need the alignment)
        img_u8, msk_u8 = img_u8.clone(), msk_u8.clone()
    image = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    body = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    xtab, ytab = (None, None) if (H, W) == (Hs, Ws) else device_tables(Hs, Ws, H, W, dev)
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_view_ingest(_lib.ptr(img_u8, torch.uint8), _lib.ptr(msk_u8, torch.uint8), V, Hs, Ws, H, W,
                                             _lib.ptr(xtab, torch.int32), _lib.ptr(ytab, torch.int32), _lib.ptr(image),
                                             _lib.ptr(body, torch.uint8), _lib.stream_ptr(dev)), "hl_view_ingest")
    return image, body
