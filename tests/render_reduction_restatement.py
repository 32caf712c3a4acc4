"""Float64 restatements of the three linear reductions of the renderer's backward (include/humanliff_hip.h, "Training of the renderer"):

  weight_grads   hl_render_weight_grads: seven products delta_rows x activation_rows^T and seven row sums over the sample points
  plane_grads    hl_render_plane_grads / hl_render_plane_grads_points: the transposed bilinear tri-plane lookup

Nothing here looks at the kernels: the row ranges are the header's table, the lookup arithmetic is the forward pass's
(oracle/render_oracle.py: _bilinear_zeros, plane_features), which the backward repeats bit for bit - every float32 operation rounded once,
in the order written there.  tests/test_render_reductions_cpu.py pins both against float64 autograd / einsum.
"""
import numpy as np
import torch

ACT_ROWS, DEL_ROWS = 630, 634          # hl_render_train_rows()
DF_ROW0 = 580                          # delta rows [580,607): dL/d tri-plane features; [607,634) belong to hl_render_plane_grads*

# (name, delta rows, activation rows, PyTorch shape of the weight) in the order of hl_render_mlp_grads
WEIGHT_JOBS = (
    ("pts0", (0, 128), (0, 27)),
    ("pts1", (128, 256), (155, 283)),
    ("pts2", (256, 384), (0, 155)),
    ("feat", (384, 512), (283, 411)),
    ("alpha", (576, 577), (283, 411)),
    ("views", (512, 576), (411, 566)),
    ("rgb", (577, 580), (566, 630)),
)
GRAD_NAMES = tuple(f"{n}_{s}" for n, _, _ in WEIGHT_JOBS for s in ("w", "b"))


def grad_shapes():
    """name -> shape of the 14 gradient tensors (PyTorch layouts: weight (out, in), bias (out))."""
    out = {}
    for name, (d0, d1), (a0, a1) in WEIGHT_JOBS:
        out[f"{name}_w"] = (d1 - d0, a1 - a0)
        out[f"{name}_b"] = (d1 - d0,)
    return out


def weight_grads(delta, act, n_cols):
    """delta (>=634, stride), act (>=630, stride) -> the 14 sums over columns [0, n_cols) in float64 (what the call ADDS to `grads`).
    Runs on the device the matrices live on."""
    out = {}
    for name, (d0, d1), (a0, a1) in WEIGHT_JOBS:
        d = delta[d0:d1, :n_cols].double()
        out[f"{name}_w"] = d @ act[a0:a1, :n_cols].double().t()
        out[f"{name}_b"] = d.sum(1)
    return out


def weight_abs_sums(delta, act, n_cols):
    """sum_p |delta[i][p] * act[n][p]| for every weight element and sum_p |delta[i][p]| for every bias element: the condition number's numerator."""
    return weight_grads(delta.abs(), act.abs(), n_cols)


def linspace01(n):
    """torch.linspace(0, 1, n) in float32 as torch defines it (and its device kernel computes it): step = 1 / (n - 1), the first half
    counted up from 0, the second half down from 1 - symmetric, both ends exact; one sample is the start.  (torch's vectorised CPU kernel
    differs from its own definition in the last bit at some n, so it is not called here.)"""
    f = np.float32
    if n == 1:
        return np.zeros(1, f)
    step = f(1) / f(n - 1)
    i = np.arange(n)
    up = (step * i.astype(f)).astype(f)
    down = (f(1) - (step * (n - 1 - i).astype(f)).astype(f)).astype(f)
    return np.where(i < n // 2, up, down)


def linspace_depths(near, far, n):
    """The coarse depths of a NULL z_vals: near * (1 - t) + far * t, t = linspace(0, 1, n), in float32 (header, hl_render_rays)."""
    f = np.float32
    t = linspace01(n)[None]
    near = np.asarray(near, f)[:, None]
    far = np.asarray(far, f)[:, None]
    return ((near * (f(1) - t).astype(f)).astype(f) + (far * t).astype(f)).astype(f)


def ray_points(rays_o, rays_d, z):
    """(R,3), (R,3), (R,S) float32 -> the sample points o + d * z (R,S,3) in float32: one product and one sum, each rounded once."""
    o = np.asarray(rays_o, np.float32)[:, None, :]
    d = np.asarray(rays_d, np.float32)[:, None, :]
    z = np.asarray(z, np.float32)[:, :, None]
    prod = (d * z).astype(np.float32)
    return (o + prod).astype(np.float32)


def texel_coords(pts, bounds, H, W, dtype=np.float32):
    """pts (M,3) -> ix, iy (9,M): the texel coordinates of the 9 (plane, group) images, q = 3 * plane + group, computed in `dtype` in the
    forward pass's order: n = 2 (p - bmin) / (bmax - bmin) - 1; plane 0 looks up (x,y), 1 (x,z), 2 (z,y); group 1 adds 1/H to the first
    coordinate, group 2 to the second; pixel = ((g + 1) size - 1) / 2."""
    f = dtype
    pts = np.asarray(pts, f)
    b = np.asarray(bounds, f).reshape(2, 3)
    ext = (b[1] - b[0]).astype(f)
    n = (f(2) * (pts - b[0][None]).astype(f)).astype(f)
    n = ((n / ext[None]).astype(f) - f(1)).astype(f)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    off = f(1.0 / H)
    ix, iy = [], []
    for u, v in ((x, y), (x, z), (z, y)):
        for g in range(3):
            gu = (u + off).astype(f) if g == 1 else u
            gv = (v + off).astype(f) if g == 2 else v
            ix.append(((((gu + f(1)).astype(f) * f(W)).astype(f) - f(1)).astype(f) / f(2)).astype(f))
            iy.append(((((gv + f(1)).astype(f) * f(H)).astype(f) - f(1)).astype(f) / f(2)).astype(f))
    return np.stack(ix), np.stack(iy)


def plane_grads(pts, delta, bounds, H, W, dtype=np.float32):
    """pts (M,3) float32, delta (M,27) float32 (feature c = 9 * plane + 3 * group + k) -> dict
         want   (27,H,W) float64: sum of the contributions fp32(delta * weight) of the taps inside the image
         taps   (9,H,W) int64: contributions per texel of image q (the same for its three channels)
         abs    (27,H,W) float64: sum of |contributions|
    Coordinates and the four weights are float32 (texel_coords, _bilinear_zeros); the sum alone is float64.  dtype = np.float64 runs the
    same statements in float64 (the CPU test compares that with autograd to rounding: the statements are the lookup's transpose)."""
    f = dtype
    pts = np.asarray(pts, f)
    delta = np.asarray(delta, f)
    M = pts.shape[0]
    assert delta.shape == (M, 27)
    IX, IY = texel_coords(pts, bounds, H, W, f)
    want = np.zeros((27, H * W), np.float64)
    absw = np.zeros((27, H * W), np.float64)
    taps = np.zeros((9, H * W), np.int64)
    for q in range(9):
        ix, iy = IX[q], IY[q]
        x0, y0 = np.floor(ix), np.floor(iy)
        x1, y1 = (x0 + f(1)).astype(f), (y0 + f(1)).astype(f)
        wx1, wx0 = (ix - x0).astype(f), (x1 - ix).astype(f)
        wy1, wy0 = (iy - y0).astype(f), (y1 - iy).astype(f)
        for xi, yi, w in ((x0, y0, wx0 * wy0), (x1, y0, wx1 * wy0), (x0, y1, wx0 * wy1), (x1, y1, wx1 * wy1)):
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)          # NaN coordinates compare false: no tap
            idx = (yi[ok].astype(np.int64) * W + xi[ok].astype(np.int64))
            w = w.astype(f)[ok]
            np.add.at(taps[q], idx, 1)
            for k in range(3):
                c = (delta[ok, 3 * q + k] * w).astype(f).astype(np.float64)
                np.add.at(want[3 * q + k], idx, c)
                np.add.at(absw[3 * q + k], idx, np.abs(c))
    return {"want": want.reshape(27, H, W), "taps": taps.reshape(9, H, W), "abs": absw.reshape(27, H, W)}


def plane_grads_autograd(pts, delta, bounds, H, W):
    """The same gradient by float64 autograd through oracle.render_oracle.plane_features: d/d planes of sum(features * delta), (27,H,W)."""
    from oracle.render_oracle import plane_features
    planes = torch.zeros(3, 9, H, W, dtype=torch.float64, requires_grad=True)
    feats = plane_features(planes, torch.as_tensor(np.asarray(pts, np.float64)), torch.as_tensor(np.asarray(bounds, np.float64)).reshape(2, 3))
    (feats * torch.as_tensor(np.asarray(delta, np.float64))).sum().backward()
    return planes.grad.reshape(27, H, W).numpy()
