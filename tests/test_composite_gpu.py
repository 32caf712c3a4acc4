"""The renderer's compositing stage alone against float64, forward and backward, each entry called through the C ABI:

  hl_render_composite            k_composite, the raw exp2 / log2 / rcp forms (the last sample: the exact ones)
  hl_render_composite_noise      k_composite_wave<false>, or k_composite with the exact forms beyond 256 samples a list / 65536 rays
  hl_render_composite_backward   k_composite_wave<true>, or k_composite_bwd beyond 256 samples a list

Inputs and both references: tests/composite_cases.py (each geometry pinned to its kernel and each case proven fair in
tests/test_composite_cpu.py); the right answer: tests/composite_restatement.py.  One metric: E = max-abs against float64 for the outputs
and max-abs over the largest |element| for the gradients, held to norm_cases.bar(E_ref) = 4 E_ref + 2e-6 with E_ref the same measure of the
fp32 CPU restatement on the identical tensors.  Every output lives inside a larger buffer of SENTINELs; the records of the rays that pad
the last 32-ray tile are NaN.
"""
import pytest
import torch

from tests import composite_cases as cc
from tests import composite_restatement as cr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 256                      # floats in front of and behind every output
DEL_ROWS = 634
_IDS = dict(ids=lambda v: v)


def _L():
    from humanliff_amd import _lib
    return _lib


def _dev(t):
    return None if t is None else t.contiguous().cuda()


class _Out:
    """n floats of SENTINEL between two guards of SENTINEL."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _inputs(c):
    nan = float("nan")
    return dict(near=_dev(c.near), far=_dev(c.far), z_vals=_dev(c.z_vals), zn=_dev(cr.tile(c.zn)), rec_c=_dev(cr.tile(c.rec_c, pad=nan)),
                rec_n=_dev(cr.tile(c.rec_n, pad=nan)), noise=_dev(c.noise))


def _forward(c, d, entry, flags, expect_rc=0, null=None, Ni=None):
    """hl_render_composite (entry "raw") or hl_render_composite_noise ("noise") -> rgb (R,3), acc (R), depth (R) on the CPU and the bits of
    all three; asserts that the guards and the rows past R keep their fill.  expect_rc != 0: asserts the refusal and that nothing was written."""
    _lib = _L()
    L = _lib.lib()
    Rp = cr.n_tiles(c.R) * 32
    outs = dict(rgb=_Out(Rp * 3), acc=_Out(Rp), depth=_Out(Rp))
    a = dict(d, **{k: o.t for k, o in outs.items()})
    if null:
        a[null] = None
    p = _lib.ptr
    head = [p(a["near"]), p(a["far"]), p(a["z_vals"]), p(a["zn"]), p(a["rec_c"]), p(a["rec_n"])]
    tail = [c.R, c.N, c.Ni if Ni is None else Ni, flags, p(a["rgb"]), p(a["acc"]), p(a["depth"]), _lib.stream_ptr()]
    if entry == "raw":
        rcode = L.hl_render_composite(*head, *tail)
    else:
        rcode = L.hl_render_composite_noise(*head, p(a["noise"]), *tail)
    torch.cuda.synchronize()
    if expect_rc:
        assert rcode == expect_rc, (rcode, L.hl_last_error())
        assert all(o.untouched() for o in outs.values()), "a refused call wrote to its outputs"
        return None
    assert rcode == 0, L.hl_last_error()
    for k, o in outs.items():
        per = 3 if k == "rgb" else 1
        assert o.guards_intact(), f"wrote outside {k}"
        assert bool((o.t[c.R * per:] == SENTINEL).all()), f"wrote {k} past the last ray"
    got = dict(rgb=outs["rgb"].t[:c.R * 3].view(c.R, 3).cpu(), acc=outs["acc"].t[:c.R].cpu(), depth=outs["depth"].t[:c.R].cpu())
    return got


def _backward(c, d, flags, g_rgb, g_acc, extra_stride=64, expect_rc=0, null=None, Ni=None, stride=None):
    """hl_render_composite_backward -> d_rec_coarse (tiles*32, N, 4), d_rec_new (tiles*32, Ni, 4) as rows of ALL rays of the tiles, and
    `del` (634, stride), on the CPU.  Asserts the guards, the delta rows other than DROW_REC..+3 and the columns past tiles*32*(N+Ni)."""
    _lib = _L()
    L = _lib.lib()
    tiles = cr.n_tiles(c.R)
    cols = tiles * 32 * (c.N + c.Ni)
    full = cols + extra_stride
    outs = dict(d_c=_Out(tiles * 32 * c.N * 4), d_n=_Out(tiles * 32 * c.Ni * 4), dl=_Out(DEL_ROWS * full))
    scratch = torch.empty(L.hl_render_composite_backward_scratch_bytes(c.R, c.N, c.Ni) // 4 + 1, dtype=torch.float32, device="cuda")
    a = dict(d, g_rgb=_dev(g_rgb), g_acc=_dev(g_acc), scratch=scratch, **{k: o.t for k, o in outs.items()})
    if null:
        a[null] = None
    p = _lib.ptr
    rcode = L.hl_render_composite_backward(p(a["near"]), p(a["far"]), p(a["z_vals"]), p(a["zn"]), p(a["rec_c"]), p(a["rec_n"]), p(a["noise"]),
                                           p(a["g_rgb"]), p(a["g_acc"]), c.R, c.N, c.Ni if Ni is None else Ni, flags, p(a["d_c"]), p(a["d_n"]),
                                           p(a["dl"]), full if stride is None else stride, p(a["scratch"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_rc:
        assert rcode == expect_rc, (rcode, L.hl_last_error())
        assert all(o.untouched() for o in outs.values()), "a refused call wrote to its outputs"
        return None
    assert rcode == 0, L.hl_last_error()
    assert all(o.guards_intact() for o in outs.values()), "wrote outside an output"
    dl = outs["dl"].t.view(DEL_ROWS, full)
    assert bool((dl[:cr.DROW_REC] == SENTINEL).all()) and bool((dl[cr.DROW_REC + 4:] == SENTINEL).all()), "wrote delta rows other than 576..579"
    assert bool((dl[:, cols:] == SENTINEL).all()), "wrote delta columns past tiles * 32 * (N + Ni)"
    return (cr.untile(outs["d_c"].t.cpu(), c.R, c.N, 4), cr.untile(outs["d_n"].t.cpu(), c.R, c.Ni, 4), dl[cr.DROW_REC:cr.DROW_REC + 4, :cols].cpu())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# --------------------------------------------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("entry", ["raw", "noise"])
@pytest.mark.parametrize("geom, flavour", cc.CASES, **_IDS)
def test_forward_against_float64(geom, flavour, entry):
    """rgb, acc and depth of both forward entries with flags 0, a white background, and the normalised + clamped depth."""
    c = cc.case(geom, flavour)
    gm = cc.GEOMETRIES[geom]
    d = _inputs(c)
    kernel = cc.KERNELS[cc.SERIAL_RAW if entry == "raw" else gm.fwd]
    for fname, flags in cc.FLAG_SETS.items():
        ref = cc.forward_reference(geom, flavour, entry == "noise", flags)
        got = _forward(c, d, entry, flags)
        again = _forward(c, d, entry, flags)
        failures = []
        for k in cc.FWD_NAMES:
            assert bool(torch.isfinite(got[k]).all()), (k, fname)
            assert _same_bits(got[k], again[k]), f"{k} ({fname}): two calls differ"
            e, bar = cc.err(got[k], ref.want[k]), cc.bar(ref.e_ref[k])
            print(f"\ncomposite-fwd | {kernel} | {geom} | {flavour} | {fname} | {k} | E {e:.3e} | E_ref {ref.e_ref[k]:.3e} | bar {bar:.3e}", end="")
            if e > bar:
                failures.append((k, fname, e, ref.e_ref[k], bar))
        assert not failures, failures


@pytest.mark.parametrize("entry", ["raw", "noise"])
def test_forward_refuses_bad_arguments(entry):
    """Host checks: a null argument, n_importance = 0.  Nothing is launched: the outputs keep their fill."""
    c = cc.case("wave-16+16", "plain")
    d = _inputs(c)
    for null in ("near", "far", "zn", "rec_c", "rec_n", "rgb", "acc", "depth"):
        _forward(c, d, entry, 0, expect_rc=-1, null=null)
    _forward(c, d, entry, 0, expect_rc=-1, Ni=0)


# -------------------------------------------------------------------------------------------------------------------------- backward

def _check_backward(c, got, extra=""):
    """Properties every backward call must have: finite, padding rays exactly zero, rows DROW_REC..+3 of `del` = the two record arrays bit
    for bit (coarse columns first, then the new ones)."""
    d_c, d_n, dl = got
    assert bool(torch.isfinite(d_c).all()) and bool(torch.isfinite(d_n).all()), "non-finite gradient" + extra
    assert bool((d_c[c.R:] == 0).all()) and bool((d_n[c.R:] == 0).all()), "padding rays are not zero" + extra
    tiles = cr.n_tiles(c.R)
    flat_c, flat_n = cr.tile(d_c[:tiles * 32], pad=0.0).view(-1, 4), cr.tile(d_n[:tiles * 32], pad=0.0).view(-1, 4)
    n_c = tiles * 32 * c.N
    for k in range(4):
        assert _same_bits(dl[k, :n_c], flat_c[:, k]) and _same_bits(dl[k, n_c:], flat_n[:, k]), f"delta row {cr.DROW_REC + k} differs from the records" + extra


@pytest.mark.parametrize("geom, flavour", cc.BACKWARD_CASES, **_IDS)
def test_backward_against_float64_autograd(geom, flavour):
    """d_rec_coarse and d_rec_new against float64 autograd of the restatement, with and without a white background (which moves g_acc);
    on the wave kernel's geometries also against the serial kernels' recurrence evaluated in float64."""
    c = cc.case(geom, flavour)
    gm = cc.GEOMETRIES[geom]
    d = _inputs(c)
    kernel = cc.KERNELS[gm.bwd]
    for fname, flags in cc.BACKWARD_FLAG_SETS.items():
        ref = cc.backward_reference(geom, flavour, flags)
        got = _backward(c, d, flags, c.g_rgb, c.g_acc)
        again = _backward(c, d, flags, c.g_rgb, c.g_acc, extra_stride=0)
        _check_backward(c, got, f" ({fname})")
        assert _same_bits(got[0], again[0]) and _same_bits(got[1], again[1]) and _same_bits(got[2], again[2]), f"two calls differ ({fname})"
        if c.zero_ray is not None:
            assert bool((got[0][c.zero_ray] == 0).all()) and bool((got[1][c.zero_ray] == 0).all()), "a ray with zero cotangents has deltas"
        failures = []
        for k, g in zip(cc.BWD_NAMES, got[:2]):
            e, bar = cc.rel_err(g[:c.R], ref.want[k]), cc.bar(ref.e_ref[k])
            print(f"\ncomposite-bwd | {kernel} | {geom} | {flavour} | {fname} | {k} | E {e:.3e} | E_ref {ref.e_ref[k]:.3e} | bar {bar:.3e}", end="")
            if e > bar:
                failures.append((k, fname, e, ref.e_ref[k], bar))
            if gm.bwd == cc.WAVE_BWD:
                e2 = cc.rel_err(g[:c.R], cc.recurrence_reference(geom, flavour, flags)[k])
                print(f" | against the float64 recurrence {e2:.3e}", end="")
                if e2 > bar:
                    failures.append((k, fname, "recurrence", e2, bar))
        assert not failures, failures
    if c.zero_ray is None:                                   # a lone ray: the zero cotangents in a call of their own
        got = _backward(c, d, 0, torch.zeros_like(c.g_rgb), torch.zeros_like(c.g_acc))
        _check_backward(c, got, " (zero cotangents)")
        assert bool((got[0] == 0).all()) and bool((got[1] == 0).all()), "zero cotangents give deltas"


def test_backward_refuses_bad_arguments():
    """Host checks: a null argument, a delta stride below tiles * 32 * (N + Ni), n_importance = 0.  Nothing is launched."""
    c = cc.case("wave-16+16", "plain")
    d = _inputs(c)
    for null in ("near", "far", "zn", "rec_c", "rec_n", "g_rgb", "g_acc", "d_c", "d_n", "dl", "scratch"):
        _backward(c, d, 0, c.g_rgb, c.g_acc, expect_rc=-1, null=null)
    cols = cr.n_tiles(c.R) * 32 * (c.N + c.Ni)
    _backward(c, d, 0, c.g_rgb, c.g_acc, expect_rc=-1, stride=cols - 1)
    _backward(c, d, 0, c.g_rgb, c.g_acc, expect_rc=-1, stride=c.R * (c.N + c.Ni))
    _backward(c, d, 0, c.g_rgb, c.g_acc, expect_rc=-1, Ni=0)
