"""Seeded inputs of tests/test_importance_{cpu,gpu}.py: raw coarse densities, coarse depths, ray directions and uniforms for the two
importance-sampling entries (hl_render_importance_new, hl_render_importance), with their float64 and fp32-CPU references
(tests/importance_restatement.py).  Plain functions, seeded generators, no GPU; every builder returns the same bits on every call, cached
results are shared and must not be written to.

One metric: E = the largest |new depth - float64| / (far - near) over the samples that are not `ambiguous` (importance_restatement: the
three places where the inverse cdf jumps), E_ref the same for the fp32 restatement, held to norm_cases.bar(E_ref) = 4 E_ref + 2e-6; an
ambiguous sample is held, with the same bar, to the hull of the values either side of its jump can give.

norm_cases.E_REF_MAX does NOT apply here: the reference's own fp32 arithmetic divides differences of a running fp32 cdf (rounding ~1e-7)
by bin masses near the 1e-5 floor, so E_ref reaches 1e-3 of the span on faint rays whatever the implementation.  The fairness condition
of this stage is instead that the bar stays below a quarter of a coarse bin, bar(E_ref) <= 0.25 / (N - 1): an indexing error moves a
sample by a bin or more (tests/test_importance_cpu.py asserts it for every case).

Geometries (R, N, Ni, z_given): every R leaves padding rays in its last 32-ray tile; every geometry but the lone ray has at least 2048 new
depths.  rpw: the rays a wave of k_importance walks (hl_render_importance_plan).

Flavours of the raw density, x = 2 randn:
  plain        x
  opaque       x + 30
  transparent  x - 24: the pdf is the 1e-5 floor
  faint        x - 8: weights comparable to the floor, 1 - expf(-x) has lost most of its bits
  wall         -30 with 5 % of the samples at +60
  spike        -30 with one interior sample at +60
  ties         (z_given only) plain densities, z[:, 2] = z[:, 1] and z[:, N-1] = z[:, N-2] where N >= 4: zero-width bins, zero distances
"""
import collections
import functools
import zlib

import torch

from tests import composite_restatement as cr
from tests import importance_restatement as ir
from tests.norm_cases import bar          # noqa: F401  (the one bar of the suite's float64 tests)

Geometry = collections.namedtuple("Geometry", "R N Ni z_given rpw")

GEOMETRIES = {
    "1ray-3+64":  Geometry(1, 3, 64, True, 1),          # one bin, one ray in the tile
    "8+8":        Geometry(264, 8, 8, False, 1),        # smallest sort
    "16+16":      Geometry(136, 16, 16, True, 1),
    "64+64":      Geometry(40, 64, 64, False, 1),       # exactly one wave chunk
    "65+130":     Geometry(40, 65, 130, True, 1),       # the carry and the running cdf cross a chunk; Ni > 128
    "128+128":    Geometry(40, 128, 128, False, 1),     # production counts, the last N with the up-front density fetch
    "129+64":     Geometry(40, 129, 64, False, 1),      # the first N without it
    "300+512":    Geometry(33, 300, 512, True, 1),      # N + Ni = 812, padded to 1024
    "512+512":    Geometry(33, 512, 512, False, 1),     # IMP_MAX_N: the LDS arrays full
    "512+1-many": Geometry(2050, 512, 1, False, 1),     # Ni = 1: no sort pass
    "rpw2":       Geometry(8200, 16, 16, False, 2),
    "rpw4":       Geometry(16390, 16, 16, True, 4),
    "rpw8":       Geometry(32769, 70, 9, False, 8),     # both fetched chunks in use
}
FLAVOURS = ("plain", "opaque", "transparent", "faint", "wall", "spike", "ties")
RPW_FLAVOURS = ("plain", "faint", "spike")


def _flavours_of(geom):
    if geom.startswith("rpw"):
        return RPW_FLAVOURS
    return tuple(f for f in FLAVOURS if f != "ties" or GEOMETRIES[geom].z_given)


CASES = tuple((g, f) for g in GEOMETRIES for f in _flavours_of(g))
PERMUTATION_CASES = tuple((g, f) for g in GEOMETRIES for f in ("plain", "wall"))       # (two outputs compared with each other: no reference needed)
UNION_CASES = tuple((g, f) for g in GEOMETRIES for f in ("plain", "spike", "ties") if f != "ties" or GEOMETRIES[g].z_given)

# Cases that missed a condition of tests/test_importance_cpu.py as first drawn, and what was done about each (none is dropped):
#   REDRAWN   another seed key.  faint at 512+512: bar(E_ref) was 0.256 of a coarse bin (the limit is a quarter); key 1 gives 0.248, too near
#             the limit to hold on another CPU's fp32 arithmetic, key 3 gives 0.213.
#             plain at 128+128: fair, but ill-conditioned as first drawn.  2 of its 5 120 samples fell in bins of mass below 1e-4, one in a bin of
#             2.1e-5, where a cdf rounding of 2e-7 moves the depth by 8e-5 of the span (binwidth / den): E and E_ref were both that ONE sample,
#             and whether its cdf entries round well is chance - the same fp32 restatement gives E_ref 2.3e-5 on one CPU and 2.6e-6 on another
#             (other vector widths in exp / cumsum), the kernel 4.5e-5, against bars of 9.3e-5 and 1.2e-5.  Key 9: the most sensitive clear
#             sample moves by 1.6e-5 of the span under the largest cdf error of the case, a third of the bar, so no single sample decides.
#             plain at 512+512: the same; as first drawn the kernel stood at 0.95 of its bar (E 4.3e-5, E_ref 1.1e-5) through two samples in bins
#             of mass 1.3e-5.  Key 3: the most sensitive clear sample moves by 3.3e-5 under the largest cdf error of the case, bar 9.0e-5.
#   SOFTENED  wall at 512+1-many: with one uniform per ray, every fourth ray has only u = 0, which falls in bin 0; on a wall ray that bin is
#             empty, its den = 1e-5 / (1 + 510e-5) within rounding of the threshold, and 22 % of the case's samples were ambiguous (the cap
#             is 10 %) although t = 0 gives b0 on either side.  Here sample 1 of those rays is a wall sample, so that their bin 0 holds mass.
REDRAWN = {("512+512", "faint"): (3,), ("128+128", "plain"): (9,), ("512+512", "plain"): (3,)}
SOFTENED = {("512+1-many", "wall")}

U_TOP = 1.0 - 2.0 ** -24         # the largest float32 below 1: above the last fp32 cdf entry of most rays

Case = collections.namedtuple("Case", "geom flavour R N Ni near far z_vals zc rays_d sigma u")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _density(flavour, R, N, g):
    x = 2.0 * torch.randn((R, N), generator=g)
    if flavour == "opaque":
        return x + 30.0
    if flavour == "transparent":
        return x - 24.0
    if flavour == "faint":
        return x - 8.0
    if flavour == "wall":
        return torch.where(torch.rand((R, N), generator=g) < 0.05, torch.full((R, N), 60.0), torch.full((R, N), -30.0))
    if flavour == "spike":
        x = torch.full((R, N), -30.0)
        at = torch.randint(1, N - 1, (R, 1), generator=g)              # interior: 1 .. N-2
        return x.scatter(1, at, 60.0)
    return x


@functools.lru_cache(maxsize=None)
def case(geom, flavour):
    """The tensors of one case, all float32 on the CPU: near, far (R); z_vals (R,N) or None; zc (R,N) the coarse depths the kernels see;
    rays_d (R,3) with norms in [0.5, 1.5]; sigma (R,N) raw; u (R,Ni) ascending per ray, on every fourth ray u[0] = 0 and (Ni >= 2)
    u[-1] = 1 - 2^-24."""
    gm = GEOMETRIES[geom]
    R, N, Ni = gm.R, gm.N, gm.Ni
    g = _gen("importance", geom, flavour, *REDRAWN.get((geom, flavour), ()))
    near = 0.25 + 0.5 * torch.rand(R, generator=g)
    far = near + 2.0 + torch.rand(R, generator=g)
    span = (far - near)[:, None]
    z_vals = None
    if gm.z_given:                                               # stratified: one depth per N-th of the interval, ascending
        z_vals = near[:, None] + span * (torch.arange(N)[None] + torch.rand((R, N), generator=g)) / N
        if flavour == "ties" and N >= 4:
            z_vals[:, 2] = z_vals[:, 1]
            z_vals[:, N - 1] = z_vals[:, N - 2]
    zc = cr.coarse_depths(near, far, z_vals, N)
    assert bool((zc[:, 1:] >= zc[:, :-1]).all())
    d = torch.randn((R, 3), generator=g)
    rays_d = d / d.norm(dim=1, keepdim=True) * (0.5 + torch.rand((R, 1), generator=g))
    sigma = _density(flavour, R, N, g)
    u = torch.rand((R, Ni), generator=g).sort(dim=1).values
    u[::4, 0] = 0.0
    if Ni >= 2:
        u[::4, -1] = U_TOP
    if (geom, flavour) in SOFTENED:
        sigma[::4, 1] = 60.0
    return Case(geom, flavour, R, N, Ni, near, far, z_vals, zc, rays_d, sigma, u)


Reference = collections.namedtuple("Reference", "want s64 ref32 e_cdf amb cands e_ref amb_share")


@functools.lru_cache(maxsize=None)
def reference(geom, flavour):
    """want (R,Ni) float64 new depths by position of u (u ascends and the inverse cdf is monotone: also the sorted order), s64 the float64
    Samples, ref32 the fp32 restatement's new depths, e_cdf = max |cdf32 - cdf64|, the ambiguous mask with its candidates, E_ref over the
    other samples in units of the ray span, and the share of ambiguous samples."""
    c = case(geom, flavour)
    s64 = ir.sample_pdf(c.sigma.double(), c.zc, c.rays_d, c.u)
    s32 = ir.sample_pdf(c.sigma, c.zc, c.rays_d, c.u)
    e_cdf = float((s32.cdf.double() - s64.cdf).abs().max())
    amb, cands = ir.ambiguous(s64, c.u, e_cdf)
    e_ref, _ = measure(c, s32.z_new, s64.z_new, amb, cands)
    return Reference(s64.z_new, s64, s32.z_new, e_cdf, amb, cands, e_ref, float(amb.double().mean()))


def measure(c, got, want, amb, cands):
    """-> (E, E_amb) in units of the ray span: the largest |got - want| over the samples that are not ambiguous, and the largest distance
    of an ambiguous sample from the hull of its candidates.  The rule of the GPU test: both at most bar(E_ref)."""
    span = (c.far - c.near).double()[:, None]
    d = (got.double() - want).abs() / span
    h = ir.hull_distance(got, cands) / span
    clear = ~amb
    e = float(d[clear].max()) if bool(clear.any()) else 0.0
    e_amb = float(h[amb].max()) if bool(amb.any()) else 0.0
    return e, e_amb
