"""numpy restatement of the layered view ingest (recon_NeRF/lib/TightCap_dataset.py:233-298 of the reference): the composed
float source of a cloth layer and its derived mask written out from the contract's table, and - through tests/view_ingest_restatement.py -
the two reductions and the nearest pick of the mask."""
import numpy as np

from tests import view_ingest_restatement as vr

PLANES = ("full", "person", "top", "bottom", "shoes")
GARMENTS = (("top", "bottom", "shoes"), ("top", "shoes"), ("shoes",))          # G_0, G_1, G_2
SKIN = np.array([0.607186, 0.49289057, 0.43795943]).astype(np.float32)


def compose_view(img_u8, planes, layer):
    """One view: img_u8 (Hs, Ws, 3) uint8, planes {name: (Hs, Ws) uint8} (only the planes the layer names are looked up), layer 0 .. 3
    -> (source (Hs, Ws, 3) float32, mask (Hs, Ws) uint8 of 0 / 1).  The first matching row of the contract's table decides."""
    if not 0 <= layer <= 3:
        raise ValueError(f"cloth layers are 0 .. 3, got {layer}")
    keep = img_u8.astype(np.float32) / np.float32(255)
    full = planes["full"] != 0
    if layer == 3:
        src = np.where(full[..., None], keep, np.float32(0))
        return src.astype(np.float32), full.astype(np.uint8)
    person = (planes["person"] != 0).astype(np.int64)
    s = person + sum((planes[g] != 0).astype(np.int64) for g in GARMENTS[layer])
    src = keep.copy()
    lone = (person == 0) & (s == 1)
    skin = s >= 2
    # written as a priority chain, lowest priority first
    src[lone] = 0
    src[skin] = SKIN
    src[~full] = 0
    mask = (src != 0).any(axis=-1).astype(np.uint8)
    return src, mask


def compose(img_u8, planes, layers):
    """A batch: img_u8 (V, Hs, Ws, 3), planes {name: (V, Hs, Ws) or None} -> (source (V, Hs, Ws, 3) float32, mask (V, Hs, Ws) uint8)."""
    out = [compose_view(img_u8[v], {n: p[v] for n, p in planes.items() if p is not None}, int(layers[v])) for v in range(len(layers))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ingest(img_u8, planes, layers, H, W):
    """dict: 'source', 'mask' (compose), 'f64', 'f32' (V, H, W, 3): the reductions of the source, 'body' (V, H, W) uint8: the nearest pick."""
    src, mask = compose(img_u8, planes, layers)
    if (H, W) == src.shape[1:3]:
        return {"source": src, "mask": mask, "f64": src.astype(np.float64), "f32": src, "body": mask}
    return {"source": src, "mask": mask, "f64": vr.resize_area_f64(src, H, W), "f32": vr.resize_area_f32(src, H, W),
            "body": vr.resize_nearest(mask, H, W)}
