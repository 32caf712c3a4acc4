"""The importance-sampling stage of the tri-plane renderer restated in plain torch (no GPU): up_sample / sample_pdf of the reference's
renderer (renderer.py:158-170, 533-563) as oracle/render_oracle.py::importance_z states them - the weights of the coarse densities, their
pdf with the 1e-5 floor, the cdf, and the inverse cdf at the uniforms `u`.

Every function works in the dtype of the densities it is given, so the same code is the float64 reference and the fp32 CPU reference of
tests/importance_cases.py.  The depths, directions and uniforms are float32 VALUES in both (a NULL z_vals comes from
composite_restatement.coarse_depths, the kernels' own float32 linspace).  Pinned in tests/test_importance_cpu.py: in float32 the sorted
union is oracle.render_oracle.importance_z bit for bit.

Where the inverse cdf is DISCONTINUOUS.  A sample in bin (lo, hi) is b0 + (u - c0) / den (b1 - b0) with den = c1 - c0 replaced by 1 when it
is below 1e-5.  Across an edge between two bins with den >= 1e-5 the value is continuous (t = 1 of one bin is t = 0 of the next); at the
LOWER edge of a flat bin (den -> 1, t ~ 0) it is b0, the end of the bin below: continuous as well.  It jumps in three places only -
  (a) den itself within rounding of 1e-5: t is (u - c0) / den or (u - c0), a whole bin apart at the upper end;
  (b) u within rounding of the UPPER edge of a flat bin: this side b0 (+ 1e-5 of a bin), the other side b1;
  (c) u within rounding of its own lower edge with a flat bin BELOW: the other side is the lower midpoint of that bin.
An empty bin of an opaque or single-spike ray has den = 1e-5 / (1 + M 1e-5), a few 1e-9 under the threshold: fp32 rounding of the running
cdf decides the branch there, for any fp32 implementation.  `ambiguous` marks those samples in the float64 result and lists what either
side of each jump gives; the tests hold such a sample to the hull of these candidates and every other sample to float64 itself.
"""
import collections

import torch
import torch.nn.functional as F

DEN_MIN = 1e-5             # sample_pdf: den < 1e-5 -> 1
PDF_FLOOR = 1e-5           # sample_pdf: weights + 1e-5

Samples = collections.namedtuple("Samples", "z_new lo hi c0 c1 den b0 b1 cdf bins")


def sample_pdf(sigma_raw, z, rays_d, u):
    """sigma_raw, z (R,N); rays_d (R,3); u (R,Ni) -> Samples in the dtype of sigma_raw: z_new (R,Ni) by position of u (NOT sorted), the bin
    (lo, hi) of every sample, its cdf values c0, c1, the raw den = c1 - c0 (before the threshold), the bin midpoints b0, b1; the ray's
    cdf (R,N-1) and midpoints `bins` (R,N-1).  The operations and their order are oracle/render_oracle.py::importance_z's."""
    dt = sigma_raw.dtype
    z, rays_d, u = z.to(dt), rays_d.to(dt), u.to(dt).contiguous()
    R, N = z.shape
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, dtype=dt)], dim=1)
    dist = dist * rays_d.norm(dim=1, keepdim=True)
    alpha = 1.0 - torch.exp(-F.softplus(sigma_raw) * dist)
    trans = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dt), 1.0 - alpha + 1e-10], dim=1), dim=1)[:, :-1]
    w = (alpha * trans)[:, 1:-1] + PDF_FLOOR
    pdf = w / w.sum(dim=1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1, dtype=dt), torch.cumsum(pdf, dim=1)], dim=1)        # (R, N-1)
    bins = 0.5 * (z[:, 1:] + z[:, :-1])                                                    # (R, N-1)
    idx = torch.searchsorted(cdf, u, right=True)
    lo = (idx - 1).clamp(min=0)
    hi = idx.clamp(max=cdf.shape[1] - 1)
    c0, c1 = cdf.gather(1, lo), cdf.gather(1, hi)
    b0, b1 = bins.gather(1, lo), bins.gather(1, hi)
    den = c1 - c0
    den_used = torch.where(den < DEN_MIN, torch.ones_like(den), den)
    z_new = b0 + (u - c0) / den_used * (b1 - b0)
    return Samples(z_new, lo, hi, c0, c1, den, b0, b1, cdf, bins)


def up_sample(sigma_raw, z, rays_d, u):
    """The reference's up_sample: the sorted union (R, N + Ni) of the coarse and the new depths."""
    return torch.sort(torch.cat([z.to(sigma_raw.dtype), sample_pdf(sigma_raw, z, rays_d, u).z_new], dim=1), dim=1)[0]


def ambiguous(s, u, e_cdf):
    """s: the float64 Samples of a case, u (R,Ni), e_cdf: the largest |cdf32 - cdf64| of the case ->
    mask (R,Ni) of the samples at one of the three jumps of the module docstring, within m = 4 e_cdf + 2^-22, and candidates (R,Ni,5):
    the float64 value, the value with den forced to 1, with den kept as computed, b1, and the lower midpoint of the bin below."""
    m = 4.0 * e_cdf + 2.0 ** -22
    u = u.double()
    flat = s.den < DEN_MIN + m
    at_threshold = (s.den - DEN_MIN).abs() <= m
    upper_of_flat = flat & (s.c1 - u <= m)
    below = (s.lo - 1).clamp(min=0)
    den_below = s.c0 - s.cdf.gather(1, below)
    lower_above_flat = (s.lo >= 1) & (den_below < DEN_MIN + m) & (u - s.c0 <= m)
    mask = at_threshold | upper_of_flat | lower_above_flat
    forced = s.b0 + (u - s.c0) * (s.b1 - s.b0)
    kept = torch.where(s.den > 0, s.b0 + (u - s.c0) / s.den.clamp(min=1e-300) * (s.b1 - s.b0), s.b0)
    cands = torch.stack([s.z_new, forced, kept, s.b1, s.bins.gather(1, below)], dim=2)
    return mask, cands


def hull_distance(got, cands):
    """How far `got` (R,Ni) lies outside [min, max] of its candidates (R,Ni,K); 0 inside."""
    got = got.double()
    lo, hi = cands.min(dim=2).values, cands.max(dim=2).values
    return torch.clamp(lo - got, min=0.0) + torch.clamp(got - hi, min=0.0)
