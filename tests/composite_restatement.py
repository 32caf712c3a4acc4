"""The compositing stage of the tri-plane renderer restated in plain torch (no GPU): merge the coarse and the new depths of every ray,
alpha-composite the raw (sigma, r, g, b) records in depth order, and differentiate that by autograd.

Every function works in the dtype of the records it is given, so the same code is the float64 reference and the fp32 CPU reference of
tests/composite_cases.py.  The DEPTHS are float32 values in both (a NULL z_vals is formed in float32 the way the kernels form it), so
the merge order of the two references and of the kernels is the same by construction.  Pinned in tests/test_composite_cpu.py: against
oracle/render_oracle.py::composite, and the backward recurrence of the kernels against autograd.

Merge order (the headers of k_composite and k_composite_wave): by depth; at equal depths a coarse sample comes before a new one and equal
depths of one list keep their list order - a stable sort of [coarse, new].
"""
import torch
import torch.nn.functional as F

from tests.render_reduction_restatement import linspace_depths

WHITE_BKGD, NORMALIZE_DEPTH, CLAMP_DEPTH = 1, 2, 8          # HL_RENDER_* of include/humanliff_hip.h
DROW_REC = 576                                              # rows 576..579 of the delta matrix: d/d(sigma, r, g, b) raw


def coarse_depths(near, far, z_vals, n_samples):
    """The coarse depths (R, N) in float32: the given rows, or for NULL near * (1 - t) + far * t with the kernels' float32 linspace."""
    if z_vals is not None:
        return z_vals.float()
    return torch.from_numpy(linspace_depths(near.float().numpy(), far.float().numpy(), n_samples))


def merge(zc, zn):
    """(R,N), (R,Ni) sorted rows -> sorted depths (R,S) and `order` (R,S): sorted sample s is entry order[s] of [coarse, new]."""
    z, order = torch.sort(torch.cat([zc, zn], 1), dim=1, stable=True)
    return z, order


def composite(zc, zn, rec_c, rec_n, noise=None, near=None, far=None, flags=0):
    """zc (R,N), zn (R,Ni) float32 depths; rec_c (R,N,4), rec_n (R,Ni,4) raw records; noise (R,S) by SORTED position or None
    -> rgb (R,3), acc (R), depth (R) in the dtype of rec_c.  renderer.py:185-186, 212-213, 221-229, 252-253, 268-274."""
    dt = rec_c.dtype
    R = zc.shape[0]
    z, order = merge(zc, zn)
    z = z.to(dt)
    rec = torch.cat([rec_c, rec_n], 1).gather(1, order[:, :, None].expand(-1, -1, 4))
    sigma = rec[..., 0]
    if noise is not None:
        sigma = sigma + noise.to(dt)
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, dtype=dt)], dim=1)        # not scaled by |d|
    alpha = 1.0 - torch.exp(-F.softplus(sigma) * dist)
    trans = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dt), 1.0 - alpha + 1e-7], dim=1), dim=1)[:, :-1]
    w = alpha * trans
    acc = w.sum(dim=1)
    rgb = (torch.sigmoid(rec[..., 1:]) * w[:, :, None]).sum(dim=1)
    depth = (w * z).sum(dim=1)
    if flags & WHITE_BKGD:
        rgb = rgb + (1.0 - acc[:, None])
    if flags & NORMALIZE_DEPTH:
        depth = (depth - near.to(dt)) / (far.to(dt) - near.to(dt) + 1e-5)
        if flags & CLAMP_DEPTH:
            depth = depth.clamp(0, 1)
    return rgb, acc, depth


def composite_grads(zc, zn, rec_c, rec_n, noise, g_rgb, g_acc, flags=0):
    """autograd of sum(rgb g_rgb) + sum(acc g_acc) with respect to the (unsorted) coarse and new records -> (R,N,4), (R,Ni,4)."""
    dt = rec_c.dtype
    rc, rn = rec_c.detach().clone().requires_grad_(True), rec_n.detach().clone().requires_grad_(True)
    rgb, acc, _ = composite(zc, zn, rc, rn, noise, flags=flags & WHITE_BKGD)
    loss = (rgb * g_rgb.to(dt)).sum() + (acc * g_acc.to(dt)).sum()
    d_c, d_n = torch.autograd.grad(loss, [rc, rn])
    return d_c, d_n


def composite_grads_recurrence(zc, zn, rec_c, rec_n, noise, g_rgb, g_acc, flags=0):
    """The same gradients by the formula the kernels state (k_composite_bwd): with gw_s = g_rgb . c_s + g_acc (- sum g_rgb under a white
    background), dL/dalpha_s = T_s (gw_s - Q_s) and Q_{s-1} = gw_s alpha_s + (1 - alpha_s + 1e-7) Q_s from Q_{S-1} = 0, then
    dalpha/dsigma = exp(-softplus(x) dist) dist softplus'(x) with softplus' = 1 beyond 20 - no division by the transmittance."""
    dt = rec_c.dtype
    R, N = zc.shape
    z, order = merge(zc, zn)
    z = z.to(dt)
    S = z.shape[1]
    rec = torch.cat([rec_c, rec_n], 1).gather(1, order[:, :, None].expand(-1, -1, 4))
    x = rec[..., 0] if noise is None else rec[..., 0] + noise.to(dt)
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, dtype=dt)], dim=1)
    e = torch.exp(-F.softplus(x) * dist)
    alpha = 1.0 - e
    f = 1.0 - alpha + 1e-7
    T = torch.ones(R, S, dtype=dt)
    for s in range(1, S):
        T[:, s] = T[:, s - 1] * f[:, s - 1]
    c = torch.sigmoid(rec[..., 1:])
    g = g_rgb.to(dt)
    ga = g_acc.to(dt) - (g.sum(1) if flags & WHITE_BKGD else 0.0)
    gw = (c * g[:, None, :]).sum(2) + ga[:, None]
    Q = torch.zeros(R, dtype=dt)
    d = torch.zeros(R, S, 4, dtype=dt)
    dsp = torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))
    for s in range(S - 1, -1, -1):
        d[:, s, 0] = T[:, s] * (gw[:, s] - Q) * (e[:, s] * dist[:, s]) * dsp[:, s]
        Q = gw[:, s] * alpha[:, s] + f[:, s] * Q
    d[..., 1:] = g[:, None, :] * (alpha * T)[:, :, None] * c * (1.0 - c)
    out = torch.zeros_like(d).scatter(1, order[:, :, None].expand(-1, -1, 4), d)
    return out[:, :N], out[:, N:]


# ---- the library's layouts ---------------------------------------------------------------------------------------------------------

def n_tiles(n_rays):
    return (n_rays + 31) // 32


def tile(rows, pad="last"):
    """Caller rows (R, n, K) or (R, n) -> the tile-major array [ceil(R/32)][n][32](K) as a flat tensor.  The rays that pad the last tile hold
    copies of the last ray (pad="last": what the renderer's own tile_rows gives the depth lists, so they are sorted like any ray's) or a
    fill value (records: NaN - nothing a padding ray holds may reach an output)."""
    squeeze = rows.dim() == 2
    if squeeze:
        rows = rows[:, :, None]
    R, n, K = rows.shape
    tiles = n_tiles(R)
    buf = torch.empty((tiles * 32, n, K), dtype=rows.dtype)
    buf[:R] = rows
    buf[R:] = rows[-1] if pad == "last" else pad
    return buf.view(tiles, 32, n, K).permute(0, 2, 1, 3).contiguous().view(-1)


def untile(flat, n_rays, n, K=1):
    """The inverse: flat [ceil(R/32)][n][32](K) -> rows of ALL ceil(R/32)*32 rays (tiles*32, n, K); [:R] are the caller's rays."""
    tiles = n_tiles(n_rays)
    return flat.view(tiles, n, 32, K).permute(0, 2, 1, 3).reshape(tiles * 32, n, K)
