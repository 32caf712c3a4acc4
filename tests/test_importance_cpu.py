"""tests/importance_cases.py and tests/importance_restatement.py on the CPU (no GPU): in float32 the restatement IS the oracle's
importance_z; every case is FAIR for this stage - bar(E_ref) at most a quarter of a coarse bin (norm_cases.E_REF_MAX does not apply: the
reference's own fp32 arithmetic divides cdf differences by values near 1e-5, see importance_cases) - has at most 10 % ambiguous samples,
and the fp32 restatement itself passes the rule the GPU test holds the kernels to; every geometry is pinned to the rays a wave walks
(hl_render_importance_plan, host arithmetic); hl_render_workspace_new_depths_offset is where the render workspace keeps the new depths."""
import pytest
import torch

from tests import importance_cases as ic
from tests import importance_restatement as ir

_IDS = dict(ids=lambda v: v)
QUARTER_BIN = 0.25
AMBIGUOUS_CAP = 0.10


def _L():
    from humanliff_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("geom", list(ic.GEOMETRIES))
def test_restatement_in_float32_is_the_oracle_bit_for_bit(geom):
    from oracle import render_oracle as ro
    c = ic.case(geom, "plain")
    want = ro.importance_z(c.sigma, c.zc, c.rays_d, c.u)
    got = ir.up_sample(c.sigma, c.zc, c.rays_d, c.u)
    assert got.dtype == want.dtype == torch.float32 and got.shape == (c.R, c.N + c.Ni)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert ir.up_sample(c.sigma.double(), c.zc, c.rays_d, c.u).dtype == torch.float64


def _row(geom, flavour):
    gm = ic.GEOMETRIES[geom]
    c, r = ic.case(geom, flavour), ic.reference(geom, flavour)
    e32, a32 = ic.measure(c, r.ref32, r.want, r.amb, r.cands)
    b = ic.bar(r.e_ref)
    return c, r, e32, a32, b, b * (gm.N - 1)


@pytest.mark.parametrize("geom, flavour", ic.CASES, **_IDS)
def test_case_is_fair(geom, flavour):
    """bar(E_ref) <= 0.25 / (N - 1) of the span; at most 10 % of the samples ambiguous; the fp32 restatement passes the GPU test's rule
    (clear samples within the bar of float64, ambiguous ones within the bar of the hull of their candidates); float64 finite and ascending
    with the ascending u, which is what lets the GPU test compare sorted position q with sample q."""
    c, r, e32, a32, b, bins = _row(geom, flavour)
    print(f"importance-fair | {geom} | {flavour} | E_ref {r.e_ref:.3e} | bar {b:.3e} | {bins:.3f} of a bin | E_cdf {r.e_cdf:.1e} | "
          f"ambiguous {100 * r.amb_share:.2f} % | fp32 outside the hull {a32:.1e}")
    assert r.want.dtype == torch.float64 and r.ref32.dtype == torch.float32 and r.want.shape == (c.R, c.Ni)
    assert bool(torch.isfinite(r.want).all()) and bool(torch.isfinite(r.ref32).all())
    span = (c.far - c.near).double()[:, None]
    assert float(((r.want[:, :-1] - r.want[:, 1:]) / span).clamp(min=0).max()) <= 1e-12 if c.Ni > 1 else True
    assert bins <= QUARTER_BIN, (bins, r.e_ref)
    assert r.amb_share <= AMBIGUOUS_CAP, r.amb_share
    assert e32 == r.e_ref and e32 <= b and a32 <= b, (e32, a32, b)
    assert c.R % 32 != 0 and (c.R == 1 or c.R * c.Ni >= 2048)


def test_fairness_table_and_largest_ambiguous_share():
    """The table DESIGN.md quotes: per flavour the geometry with the largest bar in bins, and the largest ambiguous share of any case."""
    worst, share = {}, (-1.0, ("", ""))
    for geom, flavour in ic.CASES:
        _, r, _, _, b, bins = _row(geom, flavour)
        if bins >= worst.get(flavour, (-1.0,))[0]:
            worst[flavour] = (bins, geom, r.e_ref, b)
        share = max(share, (r.amb_share, (geom, flavour)))
    print()
    for flavour in ic.FLAVOURS:
        bins, geom, e_ref, b = worst[flavour]
        print(f"importance-fair worst | {flavour:11s} | {geom:10s} | E_ref {e_ref:.3e} | bar {b:.3e} | {bins:.3f} of a bin")
    print(f"importance-fair largest ambiguous share: {100 * share[0]:.2f} % ({share[1][0]}, {share[1][1]})")
    assert max(v[0] for v in worst.values()) <= QUARTER_BIN and share[0] <= AMBIGUOUS_CAP
    for flavour in ("plain", "transparent"):              # hardly a flat bin, hardly a den near the threshold: next to nothing may be excused there
        shares = {g: ic.reference(g, f).amb_share for g, f in ic.CASES if f == flavour}
        print(f"importance-fair ambiguous on {flavour}: at most {100 * max(shares.values()):.4f} %")
        assert max(shares.values()) <= 1e-3, (flavour, shares)
    assert all(ic.reference("1ray-3+64", f).amb_share == 0.0 for f in ic.FLAVOURS)
    assert ic.reference("8+8", "spike").amb_share > 0.0 and ic.reference("16+16", "wall").amb_share > 0.0


def test_inputs_are_what_the_cases_say():
    for geom, flavour in ic.CASES:
        c = ic.case(geom, flavour)
        assert bool((c.u[:, 1:] >= c.u[:, :-1]).all()) and float(c.u.min()) == 0.0 and float(c.u.max()) < 1.0
        assert bool((c.u[::4, 0] == 0).all()) and (c.Ni < 2 or bool((c.u[::4, -1] == ic.U_TOP).all()))
        n = c.rays_d.double().norm(dim=1)
        assert 0.5 - 1e-6 <= float(n.min()) and float(n.max()) <= 1.5 + 1e-6
        assert (c.z_vals is not None) == ic.GEOMETRIES[geom].z_given
        if flavour == "ties" and c.N >= 4:
            assert bool((c.zc[:, 1] == c.zc[:, 2]).all()) and bool((c.zc[:, -1] == c.zc[:, -2]).all())
        if flavour == "spike":
            assert bool(((c.sigma == 60.0).sum(1) == 1).all()) and bool((c.sigma[:, 0] == -30.0).all()) and bool((c.sigma[:, -1] == -30.0).all())
        if flavour == "wall" and c.R * c.N > 1000:
            assert 0.02 < float((c.sigma == 60.0).float().mean()) < 0.1
    assert float(ic.U_TOP) == float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))


def test_ambiguous_marks_the_three_jumps_and_nothing_else():
    """One ray, cdf (0, 0.5, 0.5 + 9e-6, 1): bin 1 is flat.  u well inside bin 0: clear.  u just under the flat bin's upper edge: (b);
    u just over it, in bin 2 with the flat bin below: (c); u inside the flat bin away from its edges: clear (den 9e-6 is not within
    m of 1e-5 for m = 2^-22); with den 1e-5 - 1e-9 it is (a)."""
    def samples(den1, us):
        cdf = torch.tensor([[0.0, 0.5, 0.5 + den1, 1.0]], dtype=torch.float64)
        bins = torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=torch.float64)
        u = torch.tensor([us], dtype=torch.float64)
        idx = torch.searchsorted(cdf, u, right=True)
        lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=3)
        c0, c1, b0, b1 = cdf.gather(1, lo), cdf.gather(1, hi), bins.gather(1, lo), bins.gather(1, hi)
        den = c1 - c0
        z = b0 + (u - c0) / torch.where(den < 1e-5, torch.ones_like(den), den) * (b1 - b0)
        return ir.Samples(z, lo, hi, c0, c1, den, b0, b1, cdf, bins), u
    s, u = samples(9e-6, [0.25, 0.5 + 8.9e-6, 0.5 + 9.1e-6, 0.5 + 4e-6, 0.75])
    mask, cands = ir.ambiguous(s, u, 0.0)
    assert s.lo.tolist() == [[0, 1, 2, 1, 2]]
    assert mask.tolist() == [[False, True, True, False, False]]
    assert cands.shape == (1, 5, 5) and torch.equal(cands[..., 0], s.z_new)
    assert float(cands[0, 1].max()) == 3.0 and float(cands[0, 2].min()) == 2.0       # (b) reaches b1, (c) reaches the midpoint below
    s, u = samples(1e-5 - 1e-9, [0.5 + 4e-6])
    mask, cands = ir.ambiguous(s, u, 0.0)
    assert mask.tolist() == [[True]]
    assert float(cands[0, 0].min()) < 2.0 + 1e-5 and float(cands[0, 0].max()) == 3.0  # den forced to 1 ... b1
    assert ir.hull_distance(torch.tensor([[2.5]]), cands).item() == 0.0 and abs(ir.hull_distance(torch.tensor([[3.5]]), cands).item() - 0.5) < 1e-12


# ---- host queries ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", list(ic.GEOMETRIES))
def test_geometry_is_pinned_to_its_rays_per_wave(geom):
    gm = ic.GEOMETRIES[geom]
    assert _L().hl_render_importance_plan(gm.R) == gm.rpw


def test_geometries_cover_every_rays_per_wave():
    assert {gm.rpw for gm in ic.GEOMETRIES.values()} == {1, 2, 4, 8}


def test_importance_plan_boundaries():
    """1 below 256 tiles of 32 rays, 2 from 256, 4 from 512, 8 from 1024; no rays: refused."""
    L = _L()
    for tiles, (below, at) in ((256, (1, 2)), (512, (2, 4)), (1024, (4, 8))):
        assert L.hl_render_importance_plan((tiles - 1) * 32) == below          # tiles - 1 full tiles
        assert L.hl_render_importance_plan((tiles - 1) * 32 + 1) == at         # one ray into tile number `tiles`
        assert L.hl_render_importance_plan(tiles * 32) == at
    assert L.hl_render_importance_plan(1) == 1 and L.hl_render_importance_plan(1 << 33) == 8
    for bad in (0, -5):
        assert L.hl_render_importance_plan(bad) == -1
        assert b"hl_render_importance_plan" in L.hl_last_error()


def test_workspace_new_depths_offset():
    """Behind the float4 records of the N coarse and the Ni new points of ceil(R/32) * 32 rays; inside hl_render_workspace_bytes with room
    for the depths; 0 where there is no workspace."""
    L = _L()
    assert L.hl_render_workspace_new_depths_offset(0, 32, 32) == 0 and L.hl_render_workspace_new_depths_offset(64, 32, 0) == 0
    for R, N, Ni in ((33, 3, 3), (777, 64, 64), (65536, 128, 128)):
        tiles = (R + 31) // 32
        off = L.hl_render_workspace_new_depths_offset(R, N, Ni)
        assert off == 32 * tiles * (N + Ni) * 16
        assert off + 32 * tiles * Ni * 4 <= L.hl_render_workspace_bytes(R, N, Ni)
    assert L.hl_render_workspace_new_depths_offset(40, 16, 8) + 64 * 8 * 4 <= L.hl_render_workspace_bytes(40, 16, 8)
