"""Raw views -> the arrays a ViewStore holds, on the device (csrc/hl_view_ingest.hip; contract: DESIGN.md 4i).

The reference prepares every image in a DataLoader worker (recon_NeRF/lib/SynBody_dataset.py:266-278): imread / 255, img[msk == 0] = 0,
cv2.resize(INTER_AREA) of the image and cv2.resize(INTER_NEAREST) of the mask.  Here the uint8 source goes to the device as it is and one
launch writes the float32 image and the body mask of every view of the batch.

    image, body = ingest_views(img_u8, msk_u8, H, W)      # (V, Hs, Ws, 3), (V, Hs, Ws) uint8 device tensors -> (V, H, W, 3) f32, (V, H, W) u8

TightCap has one photograph and five masks per view and no image per cloth layer (recon_NeRF/lib/TightCap_dataset.py:233-298 of the
reference); the same launch composes the layer's image and derives its mask first (contract: DESIGN.md 4j):

    image, body = ingest_layered_views(img_u8, {'full': ..., 'person': ..., 'top': ..., 'bottom': ..., 'shoes': ...}, layers, H, W)

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


PLANES = ("full", "person", "top", "bottom", "shoes")
# the planes a cloth layer's rule names besides the photograph (TightCap_dataset.py:233-298): a plane outside this set is never read
LAYER_PLANES = (("full", "person", "top", "bottom", "shoes"), ("full", "person", "top", "shoes"), ("full", "person", "shoes"), ("full",))


def planes_read(layers):
    """The names of the planes a batch with these cloth layers reads, in PLANES order.  ValueError for a layer outside 0 .. 3."""
    layers = [int(x) for x in layers]
    bad = sorted({x for x in layers if not 0 <= x <= 3})
    if bad:
        raise ValueError(f"view ingest: cloth layers are 0 .. 3, got {bad}")
    return tuple(n for n in PLANES if any(n in LAYER_PLANES[x] for x in layers))


def ingest_layered_views(img_u8, masks, layers, H, W):
    """TightCap's views: img_u8 (V, Hs, Ws, 3), the photographs; masks, a dict or 5-tuple of the (V, Hs, Ws) planes full,
    person, top, bottom, shoes (None for one no view of the batch reads); layers, the V cloth layers as a host sequence.  All tensors
    contiguous uint8 on the device.  -> image (V, H, W, 3) float32, the reduction of each view's composed layer image, and body (V, H, W)
    uint8 of 0 / 1, the nearest pixel of the mask derived from it.  Enqueue-only on the current stream (the layers are uploaded here)."""
    if isinstance(masks, dict):
        unknown = sorted(set(masks) - set(PLANES))
        if unknown:
            raise ValueError(f"ingest_layered_views: unknown planes {unknown}; the planes are {PLANES}")
        masks = tuple(masks.get(n) for n in PLANES)
    masks = tuple(masks)
    if len(masks) != 5:
        raise ValueError(f"ingest_layered_views: masks must hold the five planes {PLANES} (None for one that is not read), got {len(masks)}")
    given = [m for m in masks if m is not None]
    if not (torch.is_tensor(img_u8) and img_u8.is_cuda and all(torch.is_tensor(m) and m.is_cuda for m in given)):
        raise RuntimeError("ingest_layered_views needs device tensors; humanliff_amd has no CPU path")
    if img_u8.dtype != torch.uint8 or any(m.dtype != torch.uint8 for m in given):
        raise TypeError(f"ingest_layered_views: images and masks must be uint8, got {img_u8.dtype}, {[m.dtype for m in given]}")
    if img_u8.dim() != 4 or img_u8.shape[3] != 3 or img_u8.shape[0] < 1 or any(tuple(m.shape) != tuple(img_u8.shape[:3]) for m in given):
        raise ValueError(f"ingest_layered_views: images must be (V, Hs, Ws, 3) and every plane (V, Hs, Ws); got {tuple(img_u8.shape)}, "
                         f"{[tuple(m.shape) for m in given]}")
    V, Hs, Ws = (int(s) for s in img_u8.shape[:3])
    layers = [int(x) for x in layers]
    if len(layers) != V:
        raise ValueError(f"ingest_layered_views: {len(layers)} layers for {V} views")
    missing = [n for n in planes_read(layers) if masks[PLANES.index(n)] is None]
    if missing:
        raise ValueError(f"ingest_layered_views: the layers {sorted(set(layers))} read the planes {missing}, which are None")
    Hs, Ws, H, W = check_sizes(Hs, Ws, H, W)
    dev = img_u8.device
    aligned = lambda t: t if t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) else t.contiguous().clone()  # noqa: E731
    img_u8, masks = aligned(img_u8), [aligned(m) for m in masks]
    d_layers = torch.tensor(layers, dtype=torch.int32).to(dev, non_blocking=True)
    image = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    body = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    xtab, ytab = (None, None) if (H, W) == (Hs, Ws) else device_tables(Hs, Ws, H, W, dev)
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_view_ingest_layers(_lib.ptr(img_u8, torch.uint8), *(_lib.ptr(m, torch.uint8) for m in masks),
                                                    _lib.ptr(d_layers, torch.int32), V, Hs, Ws, H, W, _lib.ptr(xtab, torch.int32),
                                                    _lib.ptr(ytab, torch.int32), _lib.ptr(image), _lib.ptr(body, torch.uint8),
                                                    _lib.stream_ptr(dev)), "hl_view_ingest_layers")
    return image, body
