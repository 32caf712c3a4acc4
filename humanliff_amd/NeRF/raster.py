"""Rasterising a mesh on the device: z-buffer and shading (csrc/hl_mesh_raster.hip).

The mesh pipeline - `Renderer.extract_mesh`, `bind_mesh`, `MeshBinding.repose` - ends in vertices, triangles, normals and colours;
this turns them, with the cameras `camera_rays` and `render_view` take (K, R, T), into images in the renderer's own layout and pixel
convention, so that a mesh image and a NeRF image of one view compare pixel by pixel.  Contract and rules: DESIGN.md "Rasterising the
mesh".

    out = raster.rasterize(vertices, triangles, H, W, K, R, T, normals=mesh["normals"], colors=mesh["colors"])
    out["rgb_map"] (F,H,W,3), out["acc_map"] (F,H,W), out["normal_map"] (F,H,W,3), out["depth_map"] (F,H,W)      # the renderer's four
    out["triangle_id"] int32 (F,H,W), out["barycentrics"] (F,H,W,3)

Pixel centres sit at integer coordinates, as in get_rays / camera_rays; depth_map is camera z, which is the ray parameter of
camera_rays' rays (their direction has camera z 1): rays_o + depth_map * rays_d lies on the surface.

There is no CPU path, no near-plane clipping (a triangle with a vertex behind `znear` is dropped), no anti-aliasing and no gradient.
"""
import numpy as np
import torch

from .. import _lib
from . import mesh
from .mesh import device_triangles  # noqa: F401  (callers convert their triangles once with raster.device_triangles)

SHADES = ("colors", "headlight")
CULLS = (None, "back", "front")
MAX_IMAGES = 65535
CAM_ROW_BYTES = 288          # a camera row inside the scratch (36 float64)


def _cameras(K, R, T):
    """Array-likes (3,3), (3,3), (3,) | (3,1) or stacks of C of them -> float64 table (C, HL_RASTER_CAM_ROW): K, inv(K), R, T."""
    K, R, T = (np.asarray(torch.as_tensor(x).detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64) for x in (K, R, T))
    if K.shape[-2:] != (3, 3) or R.shape[-2:] != (3, 3) or K.ndim not in (2, 3) or R.ndim not in (2, 3):
        raise ValueError(f"rasterize: K and R must be (3,3) or (C,3,3), got {K.shape} and {R.shape}")
    if T.shape in ((3,), (3, 1)):
        T = T.reshape(1, 3)
    elif T.ndim in (2, 3) and T.shape[1:] in ((3,), (3, 1)):
        T = T.reshape(-1, 3)
    else:
        raise ValueError(f"rasterize: T must be (3,), (3,1) or a stack of C of them, got {T.shape}")
    K, R = K.reshape(-1, 3, 3), R.reshape(-1, 3, 3)
    C = max(K.shape[0], R.shape[0], T.shape[0])
    if any(x.shape[0] not in (1, C) for x in (K, R, T)):
        raise ValueError(f"rasterize: K, R and T stack {K.shape[0]}, {R.shape[0]} and {T.shape[0]} cameras; each must be one or all {C}")
    if not (np.isfinite(K).all() and np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("rasterize: K, R and T must be finite")
    table = np.empty((C, _lib.HL_RASTER_CAM_ROW), dtype=np.float64)
    for c in range(C):
        Kc = K[c if K.shape[0] > 1 else 0]
        table[c, 0:9] = Kc.reshape(-1)
        table[c, 9:18] = np.linalg.inv(Kc).reshape(-1)           # (raises LinAlgError - a ValueError - for a singular K)
        table[c, 18:27] = R[c if R.shape[0] > 1 else 0].reshape(-1)
        table[c, 27:30] = T[c if T.shape[0] > 1 else 0]
    return table


def rasterize(vertices, triangles, H, W, K, R, T, normals=None, colors=None, shade="colors", white_bkgd=False, cull=None, znear=1e-3,
              check_indices=True):
    """vertices (N,3) | (F,N,3), triangles (T,3) of any integer dtype, normals (N,3) | (1,N,3) | (F,N,3) or None (flat normals, turned
    towards the camera), colors uint8 (N,3) or None (0.7 grey): device tensors or numpy arrays.  K, R, T: one camera or stacks of C.
    The image count is max(F, C), with F == C, F == 1 (a turntable) or C == 1 (a fixed camera on a motion).  shade "colors" writes the
    interpolated colour, "headlight" multiplies it by |n . r| with r the pixel's unit ray direction.  cull "back" / "front" skips the
    triangles whose doubled screen area A is negative / positive; None draws both windings.  check_indices reads one status word back
    and raises for a triangle index outside [0, N) (such a triangle is skipped either way).  int64 triangles - what extract_mesh
    returns - are converted to int32 on the device in every call: for repeated calls pass device_triangles(triangles, device).
    -> dict of device tensors."""
    return _rasterize(vertices, triangles, H, W, K, R, T, normals, colors, shade, white_bkgd, cull, znear, check_indices)[0]


def _rasterize(vertices, triangles, H, W, K, R, T, normals=None, colors=None, shade="colors", white_bkgd=False, cull=None, znear=1e-3,
               check_indices=True, alloc=None):
    """rasterize's body -> (outputs, scratch as int32 words).  `alloc(shape, dtype)`, default torch.empty on the device, provides the
    six outputs and then the scratch, in that order."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError(f"rasterize: bad image size {H} x {W}")
    if shade not in SHADES:
        raise ValueError(f"rasterize: shade must be one of {SHADES}, got {shade!r}")
    if cull not in CULLS:
        raise ValueError(f"rasterize: cull must be one of {CULLS}, got {cull!r}")
    if not (float(znear) > 0 and np.isfinite(float(znear))):
        raise ValueError(f"rasterize: znear must be positive and finite, got {znear}")
    vertices, triangles, normals, colors, N, Tn = mesh.mesh_arrays("rasterize", vertices, triangles, normals, colors, frames=True, any_dtype=True)
    Fv = 1 if len(vertices.shape) == 2 else int(vertices.shape[0])
    table = _cameras(K, R, T)
    C = table.shape[0]
    if not (Fv == C or Fv == 1 or C == 1):
        raise ValueError(f"rasterize: {Fv} frames and {C} cameras; they must be equal, or one of them 1")
    F = max(Fv, C)
    if F > MAX_IMAGES:
        raise ValueError(f"rasterize: {F} images in one call (at most {MAX_IMAGES})")
    mesh.need_device("rasterize")
    dev = mesh.device_of(vertices, triangles, normals, colors)
    verts = mesh.to_device(vertices, torch.float32, dev).view(Fv, N, 3)
    nrm = None if normals is None else mesh.to_device(normals, torch.float32, dev).view(-1, N, 3)
    tri = device_triangles(triangles, dev)
    col = None if colors is None else mesh.to_device(colors, torch.uint8, dev)
    flags = (_lib.HL_RASTER_WHITE_BKGD if white_bkgd else 0) | (_lib.HL_RASTER_HEADLIGHT if shade == "headlight" else 0) | \
        {None: 0, "back": _lib.HL_RASTER_CULL_BACK, "front": _lib.HL_RASTER_CULL_FRONT}[cull]
    if alloc is None:
        alloc = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    new = lambda *shape, dtype=torch.float32: alloc(shape, dtype)  # noqa: E731
    L = _lib.lib()
    need = int(L.hl_mesh_raster_scratch_bytes(N, Tn, F, H, W))
    if need == 0:
        raise ValueError(f"rasterize: sizes the library refuses (N {N}, T {Tn}, F {F}, H {H}, W {W})")
    with _lib.on(dev):
        out = {"rgb_map": new(F, H, W, 3), "acc_map": new(F, H, W), "normal_map": new(F, H, W, 3), "depth_map": new(F, H, W),
               "triangle_id": new(F, H, W, dtype=torch.int32), "barycentrics": new(F, H, W, 3)}
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        scratch = new(need // 4, dtype=torch.int32)
        assert scratch.numel() * 4 == need and scratch.is_contiguous()
        _lib.check(L.hl_mesh_raster(_lib.ptr(verts), int(verts.shape[0]), N, _lib.ptr(tri, torch.int32), Tn, _lib.ptr(nrm),
                                    0 if nrm is None else int(nrm.shape[0]), _lib.ptr(col, torch.uint8), table.ctypes.data,
                                    _lib.HL_RASTER_CAM_ROW if C > 1 else 0, F, H, W, float(znear), flags, _lib.ptr(out["rgb_map"]),
                                    _lib.ptr(out["acc_map"]), _lib.ptr(out["normal_map"]), _lib.ptr(out["depth_map"]),
                                    _lib.ptr(out["triangle_id"], torch.int32), _lib.ptr(out["barycentrics"]), _lib.ptr(status, torch.int32),
                                    _lib.ptr(scratch, torch.int32), need, _lib.stream_ptr(dev)), "hl_mesh_raster")
    if check_indices and int(status.item()) & 1:
        raise ValueError(f"rasterize: `triangles` holds an index outside [0, {N}) (such triangles were skipped)")
    return out, scratch


def scratch_records(scratch, N, F):
    """The vertex records inside a scratch of hl_mesh_raster, for inspection (its fixed layout: F camera rows of 288 bytes, then the
    records): int32 (F,N,4) - X, Y in 1/256 pixel, the bits of float z, flags (bit 0: invalid)."""
    o = F * CAM_ROW_BYTES // 4
    return scratch[o:o + F * N * 4].view(F, N, 4)
