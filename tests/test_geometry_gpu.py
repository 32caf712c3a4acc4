"""Mesh extraction on the MI355X (NeRF/geometry.py, hl_geometry.hip) against the numpy restatement of its contract
(tests/geometry_restatement.py, DESIGN.md "Mesh extraction")."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_restatement as gr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def surface_mlp(planes, dev, occupied=0.3):
    """The synthetic MLP has sigma < 0 everywhere on the synthetic planes (no surface); shift its density bias so that a fraction
    `occupied` of a coarse lattice has sigma >= 0 (u = -sigma <= 0)."""
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    mlp = syn.render_mlp_state(3, gain=2.0)
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(mlp, strict=False)
    r = r.to(dev)
    u = r.density_grid(_tp(dev), planes.to(dev), resolution=32)
    mlp["alpha_linear.bias"] = mlp["alpha_linear.bias"] + float(torch.quantile(u.flatten().double().cpu(), occupied))
    return mlp


def _tp(dev):
    from humanliff_amd import synthetic as syn
    return {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}


def _renderer(mlp, dev):
    from humanliff_amd.NeRF import Renderer
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(mlp, strict=False)
    return r.to(dev)


@pytest.fixture(scope="module")
def field_setup(dev):
    from humanliff_amd import synthetic as syn
    planes = syn.triplane(seed=11, H=64, W=64)
    return planes, surface_mlp(planes, dev)


def _sphere_bin(n=40):
    p = np.indices((n, n, n)).astype(np.float64)
    c = np.array([19.3, 20.1, 18.6])[:, None, None, None]
    return np.where(np.sqrt(((p - c) ** 2).sum(0)) < 12.4, 1.0, -1.0)


def _bridge():
    p = np.indices((33, 41, 29)).astype(np.float64)
    d1 = np.sqrt((p[0] - 9) ** 2 + (p[1] - 10) ** 2 + (p[2] - 14) ** 2)
    d2 = np.sqrt((p[0] - 23) ** 2 + (p[1] - 30) ** 2 + (p[2] - 14) ** 2)
    v = np.where((d1 < 7.5) | (d2 < 8.2), 1.0, -1.0)
    for t in np.linspace(0, 1, 200):                       # one-voxel-thin bridge between the two centres
        x, y = int(round(9 + 14 * t)), int(round(10 + 20 * t))
        v[x, y, 14] = 1.0
    return v


def _density(setup, dev, n):
    planes, mlp = setup
    return _renderer(mlp, dev).density_grid(_tp(dev), planes.to(dev), resolution=n)


CASES = ["sphere40", "bridge", "density48", "density96"]


def _case(name, setup, dev):
    if name == "sphere40":
        return torch.from_numpy(_sphere_bin()).to(dev)
    if name == "bridge":
        return torch.from_numpy(_bridge()).float().to(dev)
    return _density(setup, dev, int(name[len("density"):]))


@pytest.fixture(scope="module")
def smoothed(field_setup, dev):
    from humanliff_amd.NeRF import geometry
    out = {}
    for name in CASES:
        v = _case(name, field_setup, dev)
        got, info = geometry.smooth_constrained(v, return_info=True)
        want, it, nb = gr.smooth_constrained(v.cpu().numpy())
        out[name] = (got, info, want, it, nb)
    return out


@pytest.mark.parametrize("name", CASES)
def test_smooth_constrained_matches_restatement(smoothed, name):
    got, (it_got, nb_got), want, it, nb = smoothed[name]
    assert got.dtype == torch.float64 and got.is_cuda
    assert (nb_got, it_got) == (nb, it)
    assert 0 < it <= 250 and nb > 0
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-9


def _mc_equal(vol, iso):
    from humanliff_amd.NeRF import geometry
    v, t = geometry.marching_cubes(vol, iso)
    wv, wt = gr.marching_cubes(vol.cpu().numpy(), iso)
    assert v.dtype == torch.float64 and t.dtype == torch.int64 and v.is_cuda and t.is_cuda
    assert torch.equal(t.cpu(), torch.from_numpy(wt))
    assert v.shape == wv.shape and (len(wv) == 0 or np.abs(v.cpu().numpy() - wv).max() <= 1e-12)
    return v, t


@pytest.mark.parametrize("name", CASES)
def test_marching_cubes_matches_restatement_on_smoothed_fields(smoothed, name):
    got = smoothed[name][0]
    assert (got == 0).sum() > 0                             # the bounds clamp to exact zeros: the corner rule matters
    v, t = _mc_equal(got, 0.0)
    assert len(t) > 0


def test_marching_cubes_exact_zeros_at_isovalue(dev):
    rng = np.random.default_rng(2)
    vol = rng.integers(-1, 2, (17, 19, 23)).astype(np.float64)
    assert (vol == 0).mean() > 0.3
    _mc_equal(torch.from_numpy(vol).to(dev), 0.0)
    _mc_equal(torch.from_numpy(vol).to(dev), 1.0)          # every corner <= 1: nothing above, empty mesh
    v, t = _mc_equal(torch.from_numpy(vol).to(dev), -1.0)
    assert len(t) > 0


def test_marching_cubes_surface_cut_by_boundary(dev):
    p = np.indices((30, 26, 34)).astype(np.float64)
    vol = np.sqrt((p[0] - 2.3) ** 2 + (p[1] - 3.1) ** 2 + (p[2] - 30.2) ** 2) - 14.7
    v, t = _mc_equal(torch.from_numpy(vol).to(dev), 0.0)
    assert len(t) > 100


def test_marching_cubes_closed_sphere(dev):
    from humanliff_amd.NeRF import geometry
    n, r = 48, 15.3
    p = np.indices((n, n, n)).astype(np.float64)
    c = np.array([23.7, 24.2, 23.9])
    vol = np.sqrt(((p - c[:, None, None, None]) ** 2).sum(0)) - r     # above = outside the ball
    v, t = geometry.marching_cubes(torch.from_numpy(vol).to(dev), 0.0)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    directed = {}
    for tri in t:
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            directed[(a, b)] = directed.get((a, b), 0) + 1
    for (a, b), k in directed.items():
        assert k == 1 and directed.get((b, a)) == 1
    n_edges = len(directed) // 2
    assert len(np.unique(t)) - n_edges + len(t) == 2
    vol6 = np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0
    want = 4.0 / 3.0 * np.pi * r ** 3
    assert vol6 > 0 and abs(vol6 - want) / want < 0.02


def _restated_extract(u, bounds, res):
    sm, _, _ = gr.smooth_constrained(u)
    v, t = gr.marching_cubes(sm, 0.0)
    b = bounds.numpy()
    return v / (res - 1.0) * (b[1] - b[0])[None, :] + b[0][None, :], t


def test_extract_geometry_hip_matches_restatement_both_twins(field_setup, dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.recon_NeRF import Renderer as ReconRenderer
    planes, mlp = field_setup
    bounds = torch.tensor(syn.WORLD_BOUNDS)
    r = _renderer(mlp, dev)
    u = r.density_grid(_tp(dev), planes.to(dev), resolution=64).cpu().numpy()
    wv, wt = _restated_extract(u, bounds, 64)
    assert len(wt) > 0
    v, t = r.extract_geometry(_tp(dev), planes.to(dev), resolution=64, threshold=0.0, mesher="hip")
    assert isinstance(v, np.ndarray) and v.dtype == np.float64 and t.dtype == np.int64
    assert np.array_equal(t, wt) and np.abs(v - wv).max() <= 1e-12
    rr = ReconRenderer(use_canonical_space=False, num_instances=1, triplane_dim=64, triplane_ch=27, test=True)
    rr.load_state_dict(mlp, strict=False)
    with torch.no_grad():
        rr.tri_planes[0, 2].copy_(planes[0])
    rr = rr.to(dev)
    tp = dict(_tp(dev), instance_idx=torch.tensor([0], device=dev), cloth_layer_index=torch.tensor([2], device=dev))
    v2, t2 = rr.extract_geometry(tp, 64, 0.0, mesher="hip")
    assert np.array_equal(t2, wt) and np.abs(v2 - wv).max() <= 1e-12
    with pytest.raises(ValueError):
        r.extract_geometry(_tp(dev), planes.to(dev), resolution=16, mesher="cpu")


def test_extract_geometry_hip_at_512_is_reproducible(field_setup, dev, tmp_path):
    from humanliff_amd.NeRF import geometry
    planes, mlp = field_setup
    r = _renderer(mlp, dev)
    v1, t1 = r.extract_geometry(_tp(dev), planes.to(dev), resolution=512, mesher="hip")
    v2, t2 = r.extract_geometry(_tp(dev), planes.to(dev), resolution=512, mesher="hip")
    assert len(t1) > 1000
    assert np.array_equal(v1, v2) and np.array_equal(t1, t2)
    assert np.isfinite(v1).all() and t1.min() >= 0 and t1.max() < len(v1)
    path = str(tmp_path / "mesh512.ply")
    geometry.write_ply(path, v1, t1)
    rv, rt = geometry.read_ply(path)
    assert np.array_equal(rv, v1) and np.array_equal(rt, t1)


def test_uniform_field(dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import geometry
    with pytest.raises(ValueError):
        geometry.smooth(torch.ones((16, 16, 16), device=dev))
    with pytest.raises(ValueError):
        geometry.smooth_constrained(-torch.ones((9, 10, 11), dtype=torch.float64, device=dev))
    r = _renderer(syn.render_mlp_state(3, gain=2.0), dev)
    v, t = r.extract_geometry(_tp(dev), torch.zeros((1, 3, 9, 64, 64), device=dev), resolution=24, mesher="hip")
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == np.float64 and t.dtype == np.int64
