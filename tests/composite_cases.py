"""Seeded inputs of tests/test_composite_{cpu,gpu}.py: depth lists, raw records, density noise and cotangents for the compositing entries
(hl_render_composite, hl_render_composite_noise, hl_render_composite_backward), with their float64 and fp32-CPU references
(tests/composite_restatement.py).  Plain functions, seeded generators, no GPU; every builder returns the same bits on every call, cached
results are shared and must not be written to.  tests/test_composite_cpu.py proves every case FAIR (the fp32 restatement within E_REF_MAX
of float64) and pinned to the kernel its geometry is named for; the GPU test holds the kernels to norm_cases.bar(E_ref) on the same tensors.

Flavours (what the raw records hold; outside `ties` equal depths occur only by accident: one or two pairs in the 256+256 cases):
  plain          records 2 randn, noise randn
  ties           plain records; every new depth is a copy of a coarse depth of its ray, with repeats (equal depths across the lists and inside
                 the new list, distances of 0), and where z_vals is given some neighbouring coarse depths are equal too
  opaque         raw density + 30: the transmittance falls to the decay of the 1e-7 floor within a few samples
  transparent    raw density - 24: empty but for the last sample, where softplus(x) 1e10 is O(0.1 .. 10)
  wall           raw density -30 except about 5 % of the samples at +60
  threshold      raw density 20 + 0.5 randn, zero noise; three samples of every list exactly 20.0 with neighbours nextafter(20, +-inf)
  saturated_rgb  raw colours x 30
"""
import collections
import functools
import zlib

import torch

from tests import composite_restatement as cr
from tests.norm_cases import E_REF_MAX, bar, err, rel_err          # noqa: F401  (the one metric and bar of the suite's float64 tests)

FLAVOURS = ("plain", "ties", "opaque", "transparent", "wall", "threshold", "saturated_rgb")

Geometry = collections.namedtuple("Geometry", "R N Ni z_given fwd bwd backward")       # fwd / bwd: the kernels hl_render_composite_noise /
#                                                                                        _backward must reach; backward: False = forward only
# plan numbers of include/humanliff_hip.h
SERIAL_RAW, WAVE_FWD, SERIAL_EXACT, WAVE_BWD, SERIAL_BWD = 1, 2, 3, 4, 5
KERNELS = {SERIAL_RAW: "k_composite (raw forms)", WAVE_FWD: "k_composite_wave<false>", SERIAL_EXACT: "k_composite (exact forms)",
           WAVE_BWD: "k_composite_wave<true>", SERIAL_BWD: "k_composite_bwd"}

# every R leaves padding rays in its last 32-ray tile
GEOMETRIES = {
    "wave-16+16":       Geometry(40, 16, 16, False, WAVE_FWD, WAVE_BWD, True),
    "wave-1+1":         Geometry(33, 1, 1, True, WAVE_FWD, WAVE_BWD, True),
    "wave-3+64-1ray":   Geometry(1, 3, 64, True, WAVE_FWD, WAVE_BWD, True),
    "wave-32+33":       Geometry(40, 32, 33, False, WAVE_FWD, WAVE_BWD, True),        # S = 65: one sample past the first chunk
    "wave-64+64":       Geometry(40, 64, 64, True, WAVE_FWD, WAVE_BWD, True),
    "wave-256+256":     Geometry(40, 256, 256, False, WAVE_FWD, WAVE_BWD, True),      # S = 512: the carry crosses eight chunks
    "serial-257+3":     Geometry(40, 257, 3, True, SERIAL_EXACT, SERIAL_BWD, True),
    "serial-2+257":     Geometry(33, 2, 257, False, SERIAL_EXACT, SERIAL_BWD, True),
    "serial-65537rays": Geometry(65537, 2, 2, False, SERIAL_EXACT, WAVE_BWD, False),  # forward only: the noise branch by ray count
}
CASES = tuple((g, f) for g in GEOMETRIES for f in FLAVOURS)
BACKWARD_CASES = tuple((g, f) for g, f in CASES if GEOMETRIES[g].backward)
WAVE_BACKWARD_CASES = tuple((g, f) for g, f in BACKWARD_CASES if GEOMETRIES[g].bwd == WAVE_BWD)

FLAG_SETS = {"flags0": 0, "white_bkgd": cr.WHITE_BKGD, "depth01": cr.NORMALIZE_DEPTH | cr.CLAMP_DEPTH}
BACKWARD_FLAG_SETS = {"flags0": 0, "white_bkgd": cr.WHITE_BKGD}

Case = collections.namedtuple("Case", "geom flavour R N Ni near far z_vals zc zn rec_c rec_n noise g_rgb g_acc zero_ray")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _density(flavour, shape, g):
    x = 2.0 * torch.randn(shape, generator=g)
    if flavour == "opaque":
        return x + 30.0
    if flavour == "transparent":
        return x - 24.0
    if flavour == "wall":
        return torch.where(torch.rand(shape, generator=g) < 0.05, torch.full(shape, 60.0), torch.full(shape, -30.0))
    if flavour == "threshold":
        x = 20.0 + 0.25 * x
        n = shape[1]
        t20 = torch.tensor(20.0)
        below, above = torch.nextafter(t20, torch.tensor(-float("inf"))), torch.nextafter(t20, torch.tensor(float("inf")))
        for k in range(3):                                       # exactly 20.0 at three places of every ray, its float32 neighbours beside it
            i = (k * n) // 3
            x[:, i] = t20
            if i + 1 < n:
                x[:, i + 1] = above
            if i + 2 < n:
                x[:, i + 2] = below
        return x
    return x


@functools.lru_cache(maxsize=None)
def case(geom, flavour):
    """The tensors of one case, all float32 on the CPU: near, far (R); z_vals (R,N) or None; zc (R,N) the coarse depths the kernels see
    (z_vals, or the float32 linspace of a NULL z_vals); zn (R,Ni) sorted; rec_c (R,N,4), rec_n (R,Ni,4); noise (R,S) by sorted position;
    cotangents g_rgb (R,3), g_acc (R) with ray `zero_ray` all zero (None for a lone ray: the GPU test makes a second call with zeros)."""
    gm = GEOMETRIES[geom]
    R, N, Ni = gm.R, gm.N, gm.Ni
    g = _gen("composite", geom, flavour)
    near = 0.25 + 0.5 * torch.rand(R, generator=g)               # depths below 3.75: the fp32 rounding of the 1e-7 floor over 511 samples is 1e-5 of the depth
    far = near + 2.0 + torch.rand(R, generator=g)
    span = (far - near)[:, None]
    z_vals = None
    if gm.z_given:                                               # stratified: one depth per N-th of the interval, ascending
        z_vals = near[:, None] + span * (torch.arange(N)[None] + torch.rand((R, N), generator=g)) / N
        if flavour == "ties" and N >= 4:                         # equal neighbours inside the coarse list
            z_vals[:, 2] = z_vals[:, 1]
            z_vals[:, N - 1] = z_vals[:, N - 2]
    zc = cr.coarse_depths(near, far, z_vals, N)
    assert bool((zc[:, 1:] >= zc[:, :-1]).all())
    if flavour == "ties":
        zn = zc.gather(1, torch.randint(0, N, (R, Ni), generator=g)).sort(dim=1).values
    else:
        # even rays: up to 5 % past the far end, so that the last sample (distance 1e10) is a new one on some rays and a coarse one on others
        reach = torch.where(torch.arange(R) % 2 == 0, 1.05, 0.95)[:, None]
        zn = (near[:, None] + reach * span * torch.rand((R, Ni), generator=g)).sort(dim=1).values
    rec_c = 2.0 * torch.randn((R, N, 4), generator=g)
    rec_n = 2.0 * torch.randn((R, Ni, 4), generator=g)
    rec_c[..., 0] = _density(flavour, (R, N), g)
    rec_n[..., 0] = _density(flavour, (R, Ni), g)
    if flavour == "saturated_rgb":
        rec_c[..., 1:] *= 30.0
        rec_n[..., 1:] *= 30.0
    noise = torch.zeros((R, N + Ni)) if flavour == "threshold" else torch.randn((R, N + Ni), generator=g)
    g_rgb, g_acc = torch.randn((R, 3), generator=g), torch.randn(R, generator=g)
    zero_ray = None
    if R > 1:
        zero_ray = R // 2
        g_rgb[zero_ray] = 0.0
        g_acc[zero_ray] = 0.0
    return Case(geom, flavour, R, N, Ni, near, far, z_vals, zc, zn, rec_c, rec_n, noise, g_rgb, g_acc, zero_ray)


Forward = collections.namedtuple("Forward", "want ref32 e_ref")        # dicts over ("rgb", "acc", "depth")
Backward = collections.namedtuple("Backward", "want ref32 e_ref")      # dicts over ("d_rec_coarse", "d_rec_new"); e_ref in the relative form

FWD_NAMES = ("rgb", "acc", "depth")
BWD_NAMES = ("d_rec_coarse", "d_rec_new")


@functools.lru_cache(maxsize=None)
def forward_reference(geom, flavour, with_noise, flags):
    """float64 `want`, fp32 `ref32` and E_ref = max-abs between them, per output, on the case's tensors."""
    c = case(geom, flavour)
    noise = c.noise if with_noise else None
    want = dict(zip(FWD_NAMES, cr.composite(c.zc, c.zn, c.rec_c.double(), c.rec_n.double(), noise, c.near, c.far, flags)))
    ref32 = dict(zip(FWD_NAMES, cr.composite(c.zc, c.zn, c.rec_c, c.rec_n, noise, c.near, c.far, flags)))
    return Forward(want, ref32, {k: err(ref32[k], want[k]) for k in FWD_NAMES})


@functools.lru_cache(maxsize=None)
def backward_reference(geom, flavour, flags, zero_cotangents=False):
    """float64 autograd `want`, fp32 autograd `ref32` and E_ref = rel_err between them, per record array (noise always given)."""
    c = case(geom, flavour)
    g_rgb, g_acc = (torch.zeros_like(c.g_rgb), torch.zeros_like(c.g_acc)) if zero_cotangents else (c.g_rgb, c.g_acc)
    want = dict(zip(BWD_NAMES, cr.composite_grads(c.zc, c.zn, c.rec_c.double(), c.rec_n.double(), c.noise, g_rgb, g_acc, flags)))
    ref32 = dict(zip(BWD_NAMES, cr.composite_grads(c.zc, c.zn, c.rec_c, c.rec_n, c.noise, g_rgb, g_acc, flags)))
    return Backward(want, ref32, {k: rel_err(ref32[k], want[k]) for k in BWD_NAMES})


@functools.lru_cache(maxsize=None)
def recurrence_reference(geom, flavour, flags):
    """The serial kernels' backward formula in float64 (cr.composite_grads_recurrence) on the case."""
    c = case(geom, flavour)
    return dict(zip(BWD_NAMES, cr.composite_grads_recurrence(c.zc, c.zn, c.rec_c.double(), c.rec_n.double(), c.noise, c.g_rgb, c.g_acc, flags)))
