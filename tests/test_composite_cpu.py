"""tests/composite_cases.py and tests/composite_restatement.py on the CPU (no GPU): every geometry reaches the kernel it is named for
(hl_render_composite_plan / hl_render_composite_backward_plan are host arithmetic) and together they reach all five; every case is FAIR
(the fp32 restatement within E_REF_MAX of the float64 one, float64 finite); the restatement equals oracle/render_oracle.py::composite; the
kernels' backward recurrence equals autograd; the merge is the order the kernels' headers state; the layout helpers invert each other."""
import pytest
import torch

from tests import composite_cases as cc
from tests import composite_restatement as cr


def _plans(gm):
    from humanliff_amd import _lib
    L = _lib.lib()
    return (L.hl_render_composite_plan(gm.R, gm.N, gm.Ni, 0), L.hl_render_composite_plan(gm.R, gm.N, gm.Ni, 1),
            L.hl_render_composite_backward_plan(gm.N, gm.Ni))


@pytest.mark.parametrize("geom", sorted(cc.GEOMETRIES))
def test_geometry_reaches_the_kernels_it_is_named_for(geom):
    gm = cc.GEOMETRIES[geom]
    raw, fwd, bwd = _plans(gm)
    assert (cc.KERNELS[raw], cc.KERNELS[fwd], cc.KERNELS[bwd]) == (cc.KERNELS[cc.SERIAL_RAW], cc.KERNELS[gm.fwd], cc.KERNELS[gm.bwd])
    assert gm.R % 32 != 0                                      # padding rays in the last tile


def test_geometries_cover_all_five_kernels():
    from humanliff_amd import _lib
    reached = set()
    for gm in cc.GEOMETRIES.values():
        raw, fwd, bwd = _plans(gm)
        reached |= {raw, fwd} | ({bwd} if gm.backward else set())
    assert reached == set(cc.KERNELS) == {_lib.HL_COMPOSITE_SERIAL_RAW, _lib.HL_COMPOSITE_WAVE_FWD, _lib.HL_COMPOSITE_SERIAL_EXACT,
                                          _lib.HL_COMPOSITE_WAVE_BWD, _lib.HL_COMPOSITE_SERIAL_BWD}


def test_plan_thresholds_and_refusals():
    """The limits the header states, one step either side, and the sizes the entries refuse."""
    from humanliff_amd import _lib
    L = _lib.lib()
    assert L.hl_render_composite_plan(65536, 256, 256, 1) == cc.WAVE_FWD
    assert L.hl_render_composite_plan(65537, 256, 256, 1) == cc.SERIAL_EXACT
    assert L.hl_render_composite_plan(1, 257, 1, 1) == cc.SERIAL_EXACT and L.hl_render_composite_plan(1, 1, 257, 1) == cc.SERIAL_EXACT
    assert L.hl_render_composite_plan(1 << 33, 1, 1, 0) == cc.SERIAL_RAW and L.hl_render_composite_plan(1, 1, 1, 0) == cc.SERIAL_RAW
    assert L.hl_render_composite_backward_plan(256, 256) == cc.WAVE_BWD
    assert L.hl_render_composite_backward_plan(257, 1) == cc.SERIAL_BWD and L.hl_render_composite_backward_plan(1, 257) == cc.SERIAL_BWD
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 0), (-1, 4, 4, 0)):
        assert L.hl_render_composite_plan(*bad) == -1, bad
        assert b"hl_render_composite_plan" in L.hl_last_error()
    for bad in ((0, 4), (4, 0), (4, -2)):
        assert L.hl_render_composite_backward_plan(*bad) == -1, bad
        assert b"hl_render_composite_backward_plan" in L.hl_last_error()


@pytest.mark.parametrize("geom, flavour", cc.CASES, ids=lambda v: v)
def test_case_is_fair(geom, flavour):
    """fp32 restatement within E_REF_MAX of float64 for every checked quantity (outputs: max-abs; gradients: relative to the largest
    element), float64 free of NaN and inf."""
    c = cc.case(geom, flavour)
    worst = 0.0
    for with_noise in (False, True):
        for fname, flags in cc.FLAG_SETS.items():
            r = cc.forward_reference(geom, flavour, with_noise, flags)
            for k in cc.FWD_NAMES:
                assert r.want[k].dtype == torch.float64 and r.ref32[k].dtype == torch.float32
                assert bool(torch.isfinite(r.want[k]).all()), (k, fname, with_noise)
                assert r.e_ref[k] <= cc.E_REF_MAX, (k, fname, with_noise, r.e_ref[k])
                worst = max(worst, r.e_ref[k])
    worst_b = 0.0
    if cc.GEOMETRIES[geom].backward:
        for fname, flags in cc.BACKWARD_FLAG_SETS.items():
            r = cc.backward_reference(geom, flavour, flags)
            for k in cc.BWD_NAMES:
                assert bool(torch.isfinite(r.want[k]).all()), (k, fname)
                assert r.e_ref[k] <= cc.E_REF_MAX, (k, fname, r.e_ref[k])
                worst_b = max(worst_b, r.e_ref[k])
                if c.zero_ray is not None:
                    assert bool((r.want[k][c.zero_ray] == 0).all())
    print(f"{geom} {flavour}: forward E_ref {worst:.2e}, backward E_ref (relative) {worst_b:.2e}")


@pytest.mark.parametrize("flavour", cc.FLAVOURS)
def test_flavour_is_what_its_name_says(flavour):
    """The conditions the GPU test's findings rest on, in float64 on the 16+16 and 64+64 cases."""
    for geom in ("wave-16+16", "wave-64+64"):
        c = cc.case(geom, flavour)
        z, order = cr.merge(c.zc, c.zn)
        gaps = z[:, 1:] - z[:, :-1]
        assert bool((gaps >= 0).all())
        sig = torch.cat([c.rec_c[..., 0], c.rec_n[..., 0]], 1).gather(1, order).double() + c.noise.double()
        dist = torch.cat([gaps.double(), torch.full((c.R, 1), 1e10, dtype=torch.float64)], 1)
        alpha = 1.0 - torch.exp(-torch.nn.functional.softplus(sig) * dist)
        T = torch.cumprod(1.0 - alpha + 1e-7, 1)
        if flavour == "ties":
            assert bool(((gaps == 0).sum(1) >= c.Ni).all())                     # every new depth sits on a coarse one
            assert bool((c.zn[:, 1:] == c.zn[:, :-1]).any())                    # repeats inside the new list
            if c.z_vals is not None:
                assert bool((c.zc[:, 1] == c.zc[:, 2]).all())
        else:
            assert bool((gaps > 0).all())
        if flavour == "opaque":
            assert geom != "wave-16+16" or float(T[:, 5].max()) < 1e-2          # 99 % opaque after six samples
            assert float(T[:, -2].max()) < 1e-20                                # and by the end far below anything the sums can hold
        if flavour == "transparent":
            assert float(alpha[:, :-1].max()) < 1e-6                            # empty but for the last sample
            last = torch.nn.functional.softplus(sig[:, -1]) * 1e10
            assert 1e-4 < float(last.min()) and float(last.max()) < 1e4 and 0.1 < float(last.median()) < 10
        if flavour == "wall":
            raw = torch.cat([c.rec_c[..., 0], c.rec_n[..., 0]], 1)
            assert set(raw.unique().tolist()) == {-30.0, 60.0} and 0.02 < float((raw == 60.0).float().mean()) < 0.1
        if flavour == "threshold":
            assert not bool(c.noise.any())
            for rec in (c.rec_c, c.rec_n):
                x = rec[..., 0]
                assert bool((x == 20.0).any(1).all())
                assert float(x[x > 20.0].min()) == float(torch.nextafter(torch.tensor(20.0), torch.tensor(float("inf"))))
                assert float(x[x < 20.0].max()) == float(torch.nextafter(torch.tensor(20.0), torch.tensor(-float("inf"))))
        if flavour == "saturated_rgb":
            s = torch.sigmoid(torch.cat([c.rec_c[..., 1:], c.rec_n[..., 1:]], 1))
            assert bool((s == 0).any()) and bool((s == 1).any())


@pytest.mark.parametrize("geom", sorted(cc.GEOMETRIES))
def test_restatement_equals_the_oracle_composite_on_plain_cases(geom):
    """oracle/render_oracle.py::composite on the merged float64 samples gives the same float64 numbers, with and without noise and under
    a white background (the oracle normalises the depth in render_rays: compared without)."""
    from oracle import render_oracle as ro
    c = cc.case(geom, "plain")
    z, order = cr.merge(c.zc, c.zn)
    rec = torch.cat([c.rec_c, c.rec_n], 1).double().gather(1, order[:, :, None].expand(-1, -1, 4))
    for noise in (None, c.noise):
        for white in (False, True):
            want = ro.composite(rec[..., 1:], rec[..., 0], z.double(), white, None if noise is None else noise.double())
            got = cr.composite(c.zc, c.zn, c.rec_c.double(), c.rec_n.double(), noise, c.near, c.far, cr.WHITE_BKGD if white else 0)
            for k, a, b in zip(cc.FWD_NAMES, got, want):
                assert a.dtype == b.dtype == torch.float64
                assert torch.equal(a, b), (k, white, noise is None, float((a - b).abs().max()))


def test_merge_puts_the_coarse_sample_first_and_keeps_list_order():
    zc = torch.tensor([[1.0, 2.0, 2.0, 3.0]])
    zn = torch.tensor([[0.5, 2.0, 2.0, 3.0, 4.0]])
    z, order = cr.merge(zc, zn)
    assert z.tolist() == [[0.5, 1.0, 2.0, 2.0, 2.0, 2.0, 3.0, 3.0, 4.0]]
    assert order.tolist() == [[4, 0, 1, 2, 5, 6, 3, 7, 8]]
    # the serial kernels' walk (za <= zb takes the coarse one) on a ties case
    c = cc.case("wave-64+64", "ties")
    _, order = cr.merge(c.zc, c.zn)
    for r in (0, c.R - 1):
        ia = ib = 0
        walk = []
        while ia < c.N or ib < c.Ni:
            za = float(c.zc[r, ia]) if ia < c.N else float("inf")
            zb = float(c.zn[r, ib]) if ib < c.Ni else float("inf")
            if za <= zb:
                walk.append(ia)
                ia += 1
            else:
                walk.append(c.N + ib)
                ib += 1
        assert order[r].tolist() == walk


@pytest.mark.parametrize("flavour", cc.FLAVOURS)
@pytest.mark.parametrize("geom", ["wave-32+33", "wave-3+64-1ray", "serial-257+3"])
def test_backward_recurrence_equals_autograd_in_float64(geom, flavour):
    """The formula the kernels state (no division by the transmittance) against autograd of the restatement: 1e-11 of the largest element."""
    for flags in cc.BACKWARD_FLAG_SETS.values():
        want = cc.backward_reference(geom, flavour, flags).want
        got = cc.recurrence_reference(geom, flavour, flags)
        for k in cc.BWD_NAMES:
            assert bool(torch.isfinite(got[k]).all())
            assert cc.rel_err(got[k], want[k]) <= 1e-11, (k, flags)


def test_null_z_vals_are_the_float32_linspace_of_the_kernels():
    """near (1 - t) + far t, every operation rounded to float32, t = s / (N - 1) from the front half and 1 - (N - 1 - s) / (N - 1) from the back."""
    import numpy as np
    c = cc.case("wave-16+16", "plain")
    assert c.z_vals is None and c.zc.dtype == torch.float32
    f = np.float32
    near, far = c.near.numpy(), c.far.numpy()
    step = f(1) / f(15)
    for s in (0, 1, 7, 8, 15):
        t = f(step * f(s)) if s < 8 else f(f(1) - f(step * f(15 - s)))
        want = (near * f(f(1) - t)).astype(f) + (far * t).astype(f)
        assert np.array_equal(c.zc[:, s].numpy(), want.astype(f)), s
    assert torch.equal(c.zc[:, 0], c.near) and torch.equal(c.zc[:, -1], c.far)
    assert torch.equal(cc.case("wave-1+1", "plain").zc, cc.case("wave-1+1", "plain").z_vals)


def test_layout_helpers_invert_each_other():
    rows = torch.arange(40 * 5 * 4, dtype=torch.float32).view(40, 5, 4)
    flat = cr.tile(rows, pad=float("nan"))
    assert flat.numel() == 2 * 5 * 32 * 4
    # record (ray r, sample i) sits at float4 index tile * 32 * n + 32 * i + lane
    assert torch.equal(flat.view(-1, 4)[1 * 32 * 5 + 32 * 3 + 7], rows[39, 3])
    back = cr.untile(flat, 40, 5, 4)
    assert torch.equal(back[:40], rows) and bool(torch.isnan(back[40:]).all())
    z = torch.rand(33, 6).sort(dim=1).values
    back = cr.untile(cr.tile(z), 33, 6)[..., 0]
    assert torch.equal(back[:33], z) and torch.equal(back[33:], z[-1:].expand(31, 6))
    from humanliff_amd.NeRF.renderer import tile_rows
    assert torch.equal(cr.tile(z), tile_rows(z))
