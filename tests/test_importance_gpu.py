"""The renderer's importance sampling alone against float64, both entries called through the C ABI:

  hl_render_importance_new   k_importance, new_only = 1, sig_stride = 4: the densities are .x of the float4 coarse records, the n_importance
                             new depths come back sorted - the entry of the evaluate-once renders and of the fitting loop
  hl_render_importance       k_importance, sig_stride = 1: the sorted union of the coarse and the new depths (the re-evaluating schedule)

and importance_tile (phase B of the one-pass fine launch), a second copy of the arithmetic with a rank sort, against hl_render_importance_new
on the records and uniforms of a real render.

Inputs and both references: tests/importance_cases.py (every case proven fair and every geometry pinned to its rays per wave in
tests/test_importance_cpu.py); the right answer and the samples excused as `ambiguous`: tests/importance_restatement.py.  One metric: the
largest |new depth - float64| / (far - near) over the clear samples, held to norm_cases.bar(E_ref) = 4 E_ref + 2e-6 with E_ref the same
measure of the fp32 CPU restatement on the identical tensors; an ambiguous sample must lie within the same bar of the hull of the values
either side of its jump gives.  Every output lives between two guards of SENTINELs; the records of the rays that pad the last 32-ray tile
are NaN, and so are .y/.z/.w of every record.
"""
import pytest
import torch

from tests import composite_restatement as cr
from tests import importance_cases as ic
from tests.test_composite_gpu import SENTINEL, _Out, _dev, _same_bits

pytestmark = pytest.mark.gpu

_IDS = dict(ids=lambda v: v)
NAN = float("nan")


def _L():
    from humanliff_amd import _lib
    return _lib


def _inputs(c, u=None):
    rec = torch.full((c.R, c.N, 4), NAN)
    rec[..., 0] = c.sigma
    return dict(records=_dev(cr.tile(rec, pad=NAN)), sigma=_dev(cr.tile(c.sigma, pad=NAN)), rays_d=_dev(c.rays_d), near=_dev(c.near), far=_dev(c.far),
                z_vals=_dev(c.z_vals), u=_dev(c.u if u is None else u))


def _call(entry, c, d, expect_rc=0, null=None, R=None, N=None, Ni=None):
    """entry "new": hl_render_importance_new -> (tiles * 32, Ni) sorted new depths; "union": hl_render_importance -> (tiles * 32, N + Ni);
    rows of ALL rays of the tiles, on the CPU.  Asserts the guards.  expect_rc != 0: asserts the refusal and that nothing was written."""
    _lib = _L()
    L = _lib.lib()
    tiles = cr.n_tiles(c.R)
    n = c.Ni if entry == "new" else c.N + c.Ni
    out = _Out(tiles * 32 * n)
    a = dict(d, out=out.t)
    if null:
        a[null] = None
    p = _lib.ptr
    fn, dens = (L.hl_render_importance_new, a["records"]) if entry == "new" else (L.hl_render_importance, a["sigma"])
    rcode = fn(p(dens), p(a["rays_d"]), p(a["near"]), p(a["far"]), p(a["z_vals"]), p(a["u"]), c.R if R is None else R, c.N if N is None else N,
               c.Ni if Ni is None else Ni, p(a["out"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_rc:
        assert rcode in expect_rc, (rcode, L.hl_last_error())
        assert out.untouched(), "a refused call wrote to its output"
        return None
    assert rcode == 0, L.hl_last_error()
    assert out.guards_intact(), "wrote outside the output"
    return cr.untile(out.t.cpu(), c.R, n)[..., 0]


def _rpw(c):
    return _L().lib().hl_render_importance_plan(c.R)


# ------------------------------------------------------------------------------------------- hl_render_importance_new against float64

@pytest.mark.parametrize("geom, flavour", ic.CASES, **_IDS)
def test_new_depths_against_float64(geom, flavour):
    """Finite, ascending, the same bits on a second call; sorted position q is sample q (u ascends and the inverse cdf is monotone): every
    clear sample within bar(E_ref) of float64, every ambiguous one within bar(E_ref) of the hull of its candidates."""
    c, r = ic.case(geom, flavour), ic.reference(geom, flavour)
    d = _inputs(c)
    got, again = _call("new", c, d), _call("new", c, d)
    assert _same_bits(got, again), "two calls differ"
    got = got[:c.R]
    assert bool(torch.isfinite(got).all()), "non-finite depth"
    assert bool((got[:, 1:] >= got[:, :-1]).all()), "not ascending"
    e, e_amb = ic.measure(c, got, r.want, r.amb, r.cands)
    b = ic.bar(r.e_ref)
    print(f"\nimportance | new | {geom} | rays_per_wave {_rpw(c)} | {flavour} | E {e:.3e} | E_ref {r.e_ref:.3e} | bar {b:.3e} | "
          f"ambiguous {100 * r.amb_share:.2f} % | outside their hull {e_amb:.3e}", end="")
    assert _rpw(c) == ic.GEOMETRIES[geom].rpw
    assert e <= b and e_amb <= b, (e, e_amb, r.e_ref, b)


@pytest.mark.parametrize("geom, flavour", ic.PERMUTATION_CASES, **_IDS)
def test_order_of_u_does_not_matter(geom, flavour):
    """Each depth is drawn from its own u and the depths are sorted afterwards: a random permutation of every ray's u gives the same bits."""
    c = ic.case(geom, flavour)
    g = ic._gen("importance-permutation", geom, flavour)
    perm = torch.rand((c.R, c.Ni), generator=g).argsort(dim=1)
    shuffled = c.u.gather(1, perm)
    assert c.Ni == 1 or not torch.equal(shuffled, c.u)
    want = _call("new", c, _inputs(c))
    got = _call("new", c, _inputs(c, shuffled))
    assert bool(torch.isfinite(got[:c.R]).all())
    assert _same_bits(got[:c.R], want[:c.R])


# ------------------------------------------------------------------------------------------------ hl_render_importance (the union entry)

@pytest.mark.parametrize("geom, flavour", ic.UNION_CASES, **_IDS)
def test_union_is_the_sort_of_the_coarse_and_the_new_depths(geom, flavour):
    """(R, N + Ni) of hl_render_importance = sort([coarse depths, what hl_render_importance_new returned]) bit for bit: the sig_stride = 1
    and union-sort paths are held to the float64-checked entry without a tolerance of their own."""
    c = ic.case(geom, flavour)
    d = _inputs(c)
    new = _call("new", c, d)[:c.R]
    union = _call("union", c, d)[:c.R]
    assert bool(torch.isfinite(union).all())
    want = torch.sort(torch.cat([c.zc, new], dim=1), dim=1).values
    assert _same_bits(union, want), float((union - want).abs().max())


# -------------------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize("entry", ["new", "union"])
def test_refuses_bad_arguments(entry):
    """Host checks: n_samples = 2, n_importance = 0, either count at 513, no rays, each required pointer null (z_vals may be).  Nothing is launched."""
    c = ic.case("16+16", "plain")
    d = _inputs(c)
    bad = (-1,)
    _call(entry, c, d, expect_rc=bad, N=2)
    _call(entry, c, d, expect_rc=bad, Ni=0)
    _call(entry, c, d, expect_rc=(-2,), N=513)                        # (beyond IMP_MAX_N: HL_ERR_UNSUPPORTED)
    _call(entry, c, d, expect_rc=(-2,), Ni=513)
    _call(entry, c, d, expect_rc=bad, R=0)
    for null in ("records" if entry == "new" else "sigma", "rays_d", "near", "far", "u", "out"):
        _call(entry, c, d, expect_rc=bad, null=null)


# ---------------------------------------------------------------------------------------------- phase B of the one-pass fine launch

@pytest.mark.parametrize("R, N", [(33, 3), (777, 64), (300, 65), (1000, 128)])
def test_one_pass_launch_draws_the_depths_of_importance_new(R, N):
    """importance_tile inside k_march_plw<2, false, true> against k_importance: render once on the default schedule (fp16x2 products, NULL
    z_vals, N <= 128: two launches), read the coarse records at offset 0 of the workspace and the new depths at
    hl_render_workspace_new_depths_offset, and call hl_render_importance_new on those very records with the same u.  Rows < R: equal
    bits (both sort the same multiset; equal depths are interchangeable)."""
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    _lib = _L()
    L = _lib.lib()
    dev = torch.device("cuda:0")
    planes = syn.triplane(seed=11, H=64, W=64)
    ro_, rd_, nr_, fr_ = syn.orbit_rays(3, 36, 48, 48)
    sl = slice(48 * 9 + 5, 48 * 9 + 5 + R)
    ro_, rd_, nr_, fr_ = ro_[sl], rd_[sl], nr_[sl], fr_[sl]
    assert ro_.shape[0] == R
    u = syn.importance_u(R, N, seed=5)
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(syn.render_mlp_state(3, gain=2.0), strict=False)
    r = r.to(dev)
    assert r.mlp_products == "fp16x2" and not getattr(r, "four_launch", False)
    bounds = torch.tensor(syn.WORLD_BOUNDS)
    out = r.render({"world_bounds": bounds[None].to(dev)}, None, None, ro_[None].to(dev), rd_[None].to(dev), nr_[None].to(dev), fr_[None].to(dev),
                   planes.to(dev), N, False, n_samples=N, u=u.to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["rgb_map"]).all())
    tiles = (R + 31) // 32
    off = L.hl_render_workspace_new_depths_offset(R, N, N)
    assert off % 4 == 0 and off + tiles * 32 * N * 4 <= r._ws.numel() * 4
    fused = cr.untile(r._ws[off // 4:off // 4 + tiles * 32 * N].cpu(), R, N)[:R, :, 0]
    zn = _Out(tiles * 32 * N)
    p = _lib.ptr
    d = lambda t: t.contiguous().to(dev)  # noqa: E731
    rd_d, nr_d, fr_d, u_d = d(rd_), d(nr_), d(fr_), d(u)
    _lib.check(L.hl_render_importance_new(p(r._ws), p(rd_d), p(nr_d), p(fr_d), None, p(u_d), R, N, N, p(zn.t), _lib.stream_ptr()), "hl_render_importance_new")
    torch.cuda.synchronize()
    assert zn.guards_intact()
    alone = cr.untile(zn.t.cpu(), R, N)[:R, :, 0]
    assert bool(torch.isfinite(alone).all()) and bool((alone[:, 1:] >= alone[:, :-1]).all())
    assert float((alone.max(dim=1).values - alone.min(dim=1).values).min()) > 0 or N == 3        # real depths, not a buffer of one value
    assert _same_bits(fused, alone), float((fused - alone).abs().max())
    assert SENTINEL not in (float(alone.min()), float(alone.max()))
