"""Finishing an extracted mesh on the MI355X (hl_geometry.hip: components, filter, normals; colours through hl_render_eval_points)
against the numpy restatement (tests/mesh_finish_restatement.py) and the oracle MLP.  DESIGN.md "Finishing the mesh"."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_restatement as gr  # noqa: E402
import mesh_finish_restatement as mf  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


# ---- volumes ----------------------------------------------------------------------------------------------------------------
def _solid_volume(solid):
    """Solid voxels at -1, the rest at +1 (iso 0)."""
    return np.where(solid, -1.0, 1.0)


def _corner_cubes():
    s = np.zeros((8, 9, 10), dtype=bool)
    s[1:4, 1:4, 1:4] = True
    s[4:7, 4:7, 4:7] = True          # touches the first cube at one corner only: (3,3,3) - (4,4,4)
    return s


def _serpentine(n=24):
    """A one-voxel-thick path through the whole volume: full rows along x in every second row of every second layer, joined at
    alternating row ends and, layer to layer, above the last row.  Rows and layers are two apart, so the path never touches itself
    except where it turns: the longest chain a volume of this size holds."""
    s = np.zeros((n, n, n), dtype=bool)
    for z in range(0, n, 2):
        rows = list(range(0, n, 2))
        if (z // 2) % 2:
            rows = rows[::-1]
        for k, y in enumerate(rows):
            s[:, y, z] = True
            if k + 1 < len(rows):
                s[0 if k % 2 else n - 1, (y + rows[k + 1]) // 2, z] = True
        if z + 2 < n:
            s[0, rows[-1], z + 1] = True             # (an even number of rows: the layer ends at the x it began at)
    return s


def _lattice(n=17):
    s = np.zeros((n, n, n), dtype=bool)
    s[::2, ::2, ::2] = True
    return s


def _border():
    """One voxel on every corner, edge and face of a (9,10,11) volume."""
    s = np.zeros((9, 10, 11), dtype=bool)
    pos = [(0, 4, 8), (0, 5, 9), (0, 5, 10)]
    for x in pos[0]:
        for y in pos[1]:
            for z in pos[2]:
                if (x, y, z) != (4, 5, 5):
                    s[x, y, z] = True
    return s


def _equal_pair():
    s = np.zeros((7, 12, 9), dtype=bool)
    s[1:3, 1:3, 1:3] = True
    s[4:6, 8:10, 5:7] = True
    return s


def _nan_and_iso():
    rng = np.random.default_rng(5)
    r = rng.random((15, 18, 13))
    v = np.full(r.shape, 1.5)
    v[r < 0.05] = 0.5                # exactly iso: solid
    v[(r >= 0.05) & (r < 0.10)] = np.nan
    v[(r >= 0.10) & (r < 0.13)] = -1.0
    return v


LABEL_CASES = {
    "bernoulli0": lambda: (_solid_volume(mf.bernoulli(*mf.BERNOULLI[0])), 0.0),
    "bernoulli1": lambda: (_solid_volume(mf.bernoulli(*mf.BERNOULLI[1])), 0.0),
    "bernoulli2": lambda: (_solid_volume(mf.bernoulli(*mf.BERNOULLI[2])), 0.0),
    "corner_cubes": lambda: (_solid_volume(_corner_cubes()), 0.0),
    "serpentine": lambda: (_solid_volume(_serpentine()), 0.0),
    "lattice": lambda: (_solid_volume(_lattice()), 0.0),
    "border": lambda: (_solid_volume(_border()), 0.0),
    "all_solid": lambda: (np.full((9, 10, 11), -2.0), 0.0),
    "no_solid": lambda: (np.full((6, 5, 7), 3.0), 0.0),
    "equal_pair": lambda: (_solid_volume(_equal_pair()), 0.0),
    "nan_and_iso": lambda: (_nan_and_iso(), 0.5),
}
EXPECTED_COMPONENTS = {"corner_cubes": 1, "serpentine": 1, "lattice": 729, "border": 26, "all_solid": 1, "no_solid": 0, "equal_pair": 2}


@pytest.fixture(scope="module")
def restated_labels():
    """The restatement's (volume, iso, labels, sizes) per case, computed once."""
    out = {}
    for name, make in LABEL_CASES.items():
        vol, iso = make()
        out[name] = (vol, iso) + mf.label_volume(vol, iso)
    return out


@pytest.mark.parametrize("name", list(LABEL_CASES))
def test_labels_and_sizes_equal_restatement(name, restated_labels, dev):
    from humanliff_amd.NeRF import geometry
    vol, iso, want, want_sizes = restated_labels[name]
    if name in EXPECTED_COMPONENTS:
        assert len(want_sizes) == EXPECTED_COMPONENTS[name]          # the case is what it is meant to be
    else:
        assert len(want_sizes) >= 2
    if name == "serpentine":
        assert want_sizes[0] > 3000 and (np.asarray(vol) < 0).sum() == want_sizes[0]
    if name == "nan_and_iso":
        assert np.isnan(vol).sum() > 50 and (vol == iso).sum() > 50
    labels, sizes = geometry.label_components(torch.from_numpy(vol).to(dev), iso)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int64 and labels.is_cuda and sizes.is_cuda
    assert tuple(labels.shape) == vol.shape and tuple(sizes.shape) == (len(want_sizes),)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(sizes.cpu().numpy(), want_sizes)


@pytest.mark.parametrize("name", ["serpentine", "lattice"])
def test_labelling_is_reproducible(name, dev):
    from humanliff_amd.NeRF import geometry
    vol, iso = LABEL_CASES[name]()
    v = torch.from_numpy(vol).to(dev)
    a, b = geometry.label_components(v, iso), geometry.label_components(v, iso)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- keep_components ----------------------------------------------------------------------------------------------------------
def _bridge_field():
    """The two balls and the one-voxel bridge of the smoothing tests, as solid (-) in empty (+), with two loose blobs beside them."""
    p = np.indices((33, 41, 29)).astype(np.float64)
    d1 = np.sqrt((p[0] - 9) ** 2 + (p[1] - 10) ** 2 + (p[2] - 14) ** 2) - 7.5
    d2 = np.sqrt((p[0] - 23) ** 2 + (p[1] - 30) ** 2 + (p[2] - 14) ** 2) - 8.2
    d3 = np.sqrt((p[0] - 27) ** 2 + (p[1] - 6) ** 2 + (p[2] - 5) ** 2) - 2.6
    d4 = np.sqrt((p[0] - 4) ** 2 + (p[1] - 35) ** 2 + (p[2] - 24) ** 2) - 3.4
    v = np.minimum.reduce([d1, d2, d3, d4])
    for t in np.linspace(0, 1, 200):
        x, y = int(round(9 + 14 * t)), int(round(10 + 20 * t))
        v[x, y, 14] = min(v[x, y, 14], -0.25)
    return v


def _sphere_with_floaters():
    p = np.indices((30, 31, 33)).astype(np.float64)
    d = lambda c, r: np.sqrt(sum((p[k] - c[k]) ** 2 for k in range(3))) - r  # noqa: E731
    return np.minimum.reduce([d((14.3, 15.1, 16.2), 8.4), d((3.2, 4.1, 3.3), 2.1), d((26.4, 27.2, 28.9), 2.6), d((25.7, 3.9, 31.6), 1.7)])


FILTER_FIELDS = {"bridge": _bridge_field, "floaters": _sphere_with_floaters}


@functools.lru_cache(maxsize=None)
def _filter_reference(name):
    """(volume, labels, sizes, cell of every triangle) of the restatement, once per field."""
    vol = FILTER_FIELDS[name]()
    labels, sizes = mf.label_volume(vol, 0.0)
    return vol, labels, sizes, mf.triangle_cells(vol, 0.0)


KEEPS = ["largest", 2, 99, ("min_voxels", 60)]


@pytest.mark.parametrize("keep", KEEPS, ids=str)
@pytest.mark.parametrize("name", list(FILTER_FIELDS))
def test_keep_components_equals_restatement_and_keeps_the_kept_mesh(name, keep, dev):
    from humanliff_amd.NeRF import geometry
    vol, labels, sizes, cells = _filter_reference(name)
    assert len(sizes) == (3 if name == "bridge" else 4)
    kept_want = mf.select(sizes, keep)
    want = mf.filter_volume(vol, 0.0, labels, kept_want)
    v = torch.from_numpy(vol).to(dev)
    got, kept = geometry.keep_components(v, 0.0, keep)
    assert got.dtype == torch.float64 and got.is_cuda and kept.dtype == torch.int64
    assert np.array_equal(kept.cpu().numpy(), kept_want)
    assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))          # bit for bit
    # the triangle-subset property on the device's own marching cubes
    full = tuple(a.cpu().numpy() for a in geometry.marching_cubes(v, 0.0))
    filtered = tuple(a.cpu().numpy() for a in geometry.marching_cubes(got, 0.0))
    expect = mf.expected_subset(vol, 0.0, labels, kept_want, cells)
    assert 0 < expect.sum() and (len(kept_want) == len(sizes)) == bool(expect.all())
    mf.check_subset(full, filtered, expect)


def test_keep_components_ties_exact_values_and_bad_arguments(dev):
    from humanliff_amd.NeRF import geometry
    vol, iso = LABEL_CASES["equal_pair"]()
    got, kept = geometry.keep_components(torch.from_numpy(vol).to(dev), iso, "largest")
    assert kept.tolist() == [1]                                     # equal sizes: the lower label
    assert np.array_equal(got.cpu().numpy(), mf.keep_components(vol, iso, "largest")[0])
    vol, iso = LABEL_CASES["nan_and_iso"]()
    for keep in ("largest", 3, ("min_voxels", 2)):
        got, kept = geometry.keep_components(torch.from_numpy(vol).to(dev), iso, keep)
        want, kept_want = mf.keep_components(vol, iso, keep)
        assert np.array_equal(kept.cpu().numpy(), kept_want)
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))      # NaN and iso voxels included
    dropped = np.isnan(vol) & ~np.isnan(want)
    assert dropped.sum() > 0 and (want[dropped] == np.nextafter(iso, np.inf)).all()
    empty, kept = geometry.keep_components(torch.full((4, 5, 6), 2.0, dtype=torch.float64, device=dev), 0.0, "largest")
    assert kept.numel() == 0 and bool((empty == 2.0).all())
    with pytest.raises(ValueError):
        geometry.keep_components(torch.from_numpy(vol).to(dev), iso, "smallest")
    with pytest.raises(TypeError):
        geometry.label_components(torch.from_numpy(vol).float().to(dev), iso)


# ---- vertex normals -------------------------------------------------------------------------------------------------------------
def _sphere_sdf(n=40):
    p = np.indices((n, n, n)).astype(np.float64)
    c = np.array([19.3, 20.1, 18.6])
    return np.sqrt(((p - c[:, None, None, None]) ** 2).sum(0)) - 12.4, c


def _cut_field():
    p = np.indices((30, 26, 34)).astype(np.float64)
    return np.sqrt((p[0] - 2.3) ** 2 + (p[1] - 3.1) ** 2 + (p[2] - 30.2) ** 2) - 14.7


def _zeros_field():
    return np.random.default_rng(2).integers(-1, 2, (17, 19, 23)).astype(np.float64)


NORMAL_FIELDS = {"sphere": lambda: (_sphere_sdf()[0], None), "cut_by_boundary": lambda: (_cut_field(), (2.0, 2.2, 1.5)),
                 "exact_zeros": lambda: (_zeros_field(), (1.0, 0.5, 3.0))}


@pytest.mark.parametrize("name", list(NORMAL_FIELDS))
def test_vertex_normals_equal_restatement(name, dev):
    """Both sides are fp64 and the formula is a few dozen operations on values of order 1, so the components of a unit vector agree
    to a few hundred ulp: 1e-12 absolute, the bound of the marching-cubes vertex test."""
    from humanliff_amd.NeRF import geometry
    vol, ext = NORMAL_FIELDS[name]()
    v = torch.from_numpy(vol).to(dev)
    verts, tris = geometry.marching_cubes(v, 0.0)
    got = geometry.vertex_normals(v, 0.0, verts, None if ext is None else torch.tensor(ext, dtype=torch.float64))
    want = mf.vertex_normals(vol, 0.0, ext)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == tuple(verts.shape) == want.shape and len(want) > 500
    g = got.cpu().numpy()
    print(f"{name}: max |normal - restatement| = {np.abs(g - want).max():.3e}")
    assert np.isfinite(g).all()
    assert np.abs(g - want).max() <= 1e-12
    length = np.linalg.norm(g, axis=1)
    assert (np.abs(length - 1.0) < 1e-12)[length > 0].all()
    if name == "exact_zeros":
        assert (length == 0).sum() == (np.linalg.norm(want, axis=1) == 0).sum()
    if name == "cut_by_boundary":
        on_face = (verts.cpu().numpy() == 0).any(axis=1)
        assert on_face.sum() > 20                                  # vertices whose gradient is one-sided
    # outward: along the winding the case table gives the triangles
    vw = verts.cpu().numpy()
    t = tris.cpu().numpy()
    if name != "exact_zeros":
        e = 1.0 if ext is None else np.asarray(ext)
        face = np.cross((vw[t[:, 1]] - vw[t[:, 0]]) * e, (vw[t[:, 2]] - vw[t[:, 0]]) * e)
        assert (np.einsum("ij,ij->i", face, g[t[:, 0]]) > 0).mean() > 0.999
    with pytest.raises(ValueError):
        geometry.vertex_normals(v, 0.0, verts[:-1])


def test_sphere_normals_are_radial(dev):
    """The angle between a normal and the radius of the sphere: bounded by what the restatement, on the CPU, gives for the same
    definition plus 10 % (DESIGN.md records the figure).  The error is the finite difference's, not the kernel's."""
    from humanliff_amd.NeRF import geometry
    vol, c = _sphere_sdf()
    wv, _ = gr.marching_cubes(vol, 0.0)

    def angles(n, verts):
        r = verts - c[None]
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        return np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", n, r), -1.0, 1.0)))

    bound = angles(mf.vertex_normals(vol, 0.0), wv).max() * 1.1
    v = torch.from_numpy(vol).to(dev)
    verts, _ = geometry.marching_cubes(v, 0.0)
    got = angles(geometry.vertex_normals(v, 0.0, verts).cpu().numpy(), verts.cpu().numpy())
    print(f"sphere 40^3, r = 12.4: max angle to the radius {got.max():.4f} deg (bound {bound:.4f})")
    assert 0 < bound < 1.0 and got.max() <= bound


# ---- vertex colours -------------------------------------------------------------------------------------------------------------
# The bound is the one tests/test_render_gpu.py::test_canonical_density_grid_matches_oracle holds hl_render_eval_points' records to
# against the oracle: 5e-5 on 99.9 % of the points (a near-tie between two body vertices may resolve differently in float32).  The
# sigmoid that follows has slope <= 1/4, so the colours inherit it; without the deformation there are no ties and every vertex holds it.
COLOR_TOL = 5e-5


def _oracle_colors(mlp, planes, pts, dirs, bounds):
    from oracle import render_oracle as orc
    m64 = {k: v.double() for k, v in mlp.items()}
    with torch.no_grad():
        rgb_raw, _ = orc.mlp(m64, orc.plane_features(planes[0].double(), pts.double(), bounds.double()), dirs.double())
    return torch.sigmoid(rgb_raw)


def _renderer(mlp, dev):
    from humanliff_amd.NeRF import Renderer
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, smpl_type='smpl', test=True)
    r.load_state_dict(mlp, strict=False)
    return r.to(dev)


def _unit(d):
    return d / d.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("V", [1000, 33])
def test_vertex_colors_identity_branch_match_oracle(V, dev):
    from humanliff_amd import synthetic as syn
    planes = syn.triplane(seed=11, H=64, W=64)
    mlp = syn.render_mlp_state(3, gain=2.0)
    r = _renderer(mlp, dev)
    bounds = torch.tensor(syn.WORLD_BOUNDS)
    g = torch.Generator().manual_seed(V)
    pts = (bounds[0] + (bounds[1] - bounds[0]) * torch.rand((V, 3), generator=g)).double()       # fp64 in, as the mesh path hands them over
    dirs = _unit(torch.randn((V, 3), generator=g)).double()
    got = r.vertex_colors({"world_bounds": bounds[None].to(dev)}, planes.to(dev), pts.to(dev), dirs.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (V, 3) and got.is_cuda
    want = _oracle_colors(mlp, planes, pts.float(), dirs.float(), bounds)
    err = (got.cpu().double() - want).abs()
    print(f"identity V={V}: max colour error {float(err.max()):.3e}, colour range {float(want.min()):.3f}..{float(want.max()):.3f}")
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float(want.max() - want.min()) > 0.05                     # the colours are not one constant
    assert float(err.max()) < COLOR_TOL
    with pytest.raises(RuntimeError):
        r.vertex_colors({"world_bounds": bounds[None].to(dev)}, planes.to(dev), pts, dirs)


@pytest.mark.parametrize("V", [1000, 33])
def test_vertex_colors_canonical_branch_match_oracle(V, dev):
    from oracle import deform_oracle as do
    from humanliff_amd import synthetic as syn
    NV = 1200
    cpu_model = syn.smpl_like_model(NV, 7)
    pose = syn.smpl_like_pose(NV, cpu_model, 17, n_points=V)
    mlp = syn.render_mlp_state(3)
    r = _renderer(mlp, dev)
    r.use_canonical_space = True
    r.SMPL_NEUTRAL = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cpu_model.items()}
    planes = syn.triplane(seed=11, H=64, W=64)
    pts, dirs = pose["pts"][0].float(), _unit(pose["viewdirs"][0].float())
    got = r.vertex_colors(dict(pose), planes.to(dev), pts.to(dev), dirs.to(dev)).cpu()
    with torch.no_grad():
        can, cd, _ = do.deform_target2c(cpu_model, pose, pts, dirs)
    want = _oracle_colors(mlp, planes, can, cd, pose["t_world_bounds"][0])
    err = (got.double() - want).abs().max(dim=1).values
    print(f"canonical V={V}: max colour error {float(err.max()):.3e}, median {float(err.median()):.3e}, "
          f"within {COLOR_TOL:g}: {float((err < COLOR_TOL).float().mean()):.4f}")
    assert tuple(got.shape) == (V, 3)
    assert float((err < COLOR_TOL).float().mean()) > 0.999


# ---- extract_mesh ---------------------------------------------------------------------------------------------------------------
BALLS = [((0.0, 0.0, 0.0), 0.5), ((0.68, 0.74, 0.66), 0.16)]        # the body and the planted floater, in normalised coordinates


def _planted_scene():
    """Tri-planes whose density has a second bump well inside the bounds.  Each plane blends two 9-channel feature chunks, `solid` inside
    the discs the balls project to and `empty` outside; the balls are apart along every axis, so only inside a ball do all three planes
    read `solid`.  The chunks are fitted (a few hundred Adam steps on the oracle MLP, on the CPU) so that this combination has a higher
    density than the seven mixed ones, and the density bias is put between the two."""
    from oracle import render_oracle as orc
    from humanliff_amd import synthetic as syn
    mlp = syn.render_mlp_state(3, gain=2.0)

    def combos(S, E):
        return torch.stack([torch.cat([(S if (k >> p) & 1 else E)[p] for p in range(3)]) for k in range(8)])

    g = torch.Generator().manual_seed(0)
    S = ((torch.rand((3, 9), generator=g) * 2 - 1) * 0.5).requires_grad_()
    E = ((torch.rand((3, 9), generator=g) * 2 - 1) * 0.5).requires_grad_()
    opt = torch.optim.Adam([S, E], lr=0.05)
    for _ in range(300):
        sig = orc.mlp(mlp, combos(S, E))
        loss = -(sig[7] - sig[:7].max())
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            S.clamp_(-1, 1)
            E.clamp_(-1, 1)
    S, E = S.detach(), E.detach()
    with torch.no_grad():
        sig = orc.mlp(mlp, combos(S, E))
    assert float(sig[7] - sig[:7].max()) > 0.5
    mlp["alpha_linear.bias"] = mlp["alpha_linear.bias"] - float(0.5 * (sig[7] + sig[:7].max()))
    H, soft = 64, 0.08
    c = (torch.arange(H) + 0.5) / H * 2 - 1
    vv, uu = torch.meshgrid(c, c, indexing="ij")          # rows: the plane's second coordinate
    planes = torch.empty((1, 3, 9, H, H))
    for p, (a, b) in enumerate([(0, 1), (0, 2), (2, 1)]):
        m = torch.zeros((H, H))
        for ctr, rad in BALLS:
            m = torch.maximum(m, ((rad - torch.sqrt((uu - ctr[a]) ** 2 + (vv - ctr[b]) ** 2)) / soft + 0.5).clamp(0, 1))
        planes[0, p] = E[p][:, None, None] + (S[p] - E[p])[:, None, None] * m[None]
    return planes, mlp


def _twins(planes, mlp, dev):
    """(name, extract_mesh, extract_geometry_hip, vertex_colors, density_grid) of both renderer twins on the same planes and MLP."""
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.recon_NeRF import Renderer as ReconRenderer
    tp = {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(mlp, strict=False)
    r = r.to(dev)
    pl = planes.to(dev)
    yield ("NeRF", lambda **kw: r.extract_mesh(tp, pl, resolution=48, **kw), lambda: r.extract_geometry(tp, pl, resolution=48, mesher="hip"),
           lambda v, d: r.vertex_colors(tp, pl, v, d), lambda: r.density_grid(tp, pl, resolution=48))
    rr = ReconRenderer(use_canonical_space=False, num_instances=1, triplane_dim=64, triplane_ch=27, test=True)
    rr.load_state_dict(mlp, strict=False)
    with torch.no_grad():
        rr.tri_planes[0, 2].copy_(planes[0])
    rr = rr.to(dev)
    tp2 = dict(tp, instance_idx=torch.tensor([0], device=dev), cloth_layer_index=torch.tensor([2], device=dev))
    yield ("recon_NeRF", lambda **kw: rr.extract_mesh(tp2, 48, **kw), lambda: rr.extract_geometry(tp2, 48, 0.0, mesher="hip"),
           lambda v, d: rr.vertex_colors(tp2, v, d), lambda: rr.density_grid(tp2, 48))


@pytest.fixture(scope="module")
def planted():
    return _planted_scene()


def _same(a, b):
    return all((a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])) for k in a) and set(a) == set(b)


def test_extract_mesh_both_twins(planted, dev):
    from humanliff_amd.NeRF import geometry
    planes, mlp = planted
    for name, extract_mesh, extract_geometry, vertex_colors, density_grid in _twins(planes, mlp, dev):
        mesh = extract_mesh()
        assert set(mesh) == {"vertices", "triangles", "normals", "colors", "component_sizes"}, name
        v, t = extract_geometry()
        assert len(t) > 1000
        assert mesh["vertices"].dtype == np.float64 and mesh["triangles"].dtype == np.int64
        assert np.array_equal(mesh["vertices"], v) and np.array_equal(mesh["triangles"], t), name      # the bits of extract_geometry
        # the planted floater survives smoothing at this resolution: shown on the restatement
        u = density_grid()
        restated_sizes = mf.label_volume(gr.smooth_constrained(u.cpu().numpy())[0], 0.0)[1]
        assert len(restated_sizes) == 2 and restated_sizes.min() > 50, restated_sizes
        field = geometry.smooth(u)
        field_cpu = field.cpu().numpy()
        labels, sizes = mf.label_volume(field_cpu, 0.0)
        assert np.array_equal(sizes, restated_sizes)
        assert mesh["component_sizes"].dtype == np.int64 and np.array_equal(mesh["component_sizes"], sizes), name
        # normals: unit or zero; colours: vertex_colors of the returned vertices, seen head-on
        n = mesh["normals"]
        assert n.dtype == np.float64 and n.shape == v.shape
        length = np.linalg.norm(n, axis=1)
        assert (np.abs(length[length > 0] - 1.0) < 1e-12).all() and (length > 0).mean() > 0.99
        body = np.linalg.norm(v, axis=1) < 0.9                                    # (the floater sits in a corner, the body at the origin)
        assert body.sum() > 1000 and (np.einsum("ij,ij->i", n[body], v[body]) > 0).mean() > 0.95          # outward
        c = mesh["colors"]
        assert c.dtype == np.uint8 and c.shape == v.shape
        vc = vertex_colors(torch.from_numpy(v).to(dev), torch.from_numpy(-n).to(dev)).cpu().numpy()
        assert vc.dtype == np.float32 and np.array_equal(c, np.round(np.clip(vc, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)), name
        # components="largest": one component, exactly the body's triangles
        big = extract_mesh(components="largest")
        assert np.array_equal(big["component_sizes"], sizes)
        kept = mf.select(sizes, "largest")
        expect = mf.expected_subset(field_cpu, 0.0, labels, kept, mf.triangle_cells(field_cpu, 0.0))
        assert 0 < (~expect).sum() < expect.sum()
        mf.check_subset((v, t), (big["vertices"], big["triangles"]), expect)
        filtered, _ = geometry.keep_components(field, 0.0, "largest")
        assert geometry.label_components(filtered, 0.0)[1].numel() == 1
        # reproducible, and the switches
        assert _same(mesh, extract_mesh()) and _same(big, extract_mesh(components="largest")), name
        bare = extract_mesh(normals=False, colors=False)
        assert bare["normals"] is None and bare["colors"] is None and np.array_equal(bare["vertices"], v)


def test_extract_mesh_without_a_surface(dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.NeRF import Renderer
    r = Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True)
    r.load_state_dict(syn.render_mlp_state(3, gain=2.0), strict=False)
    r = r.to(dev)
    tp = {"world_bounds": torch.tensor(syn.WORLD_BOUNDS)[None].to(dev)}
    mesh = r.extract_mesh(tp, torch.zeros((1, 3, 9, 64, 64), device=dev), resolution=24, components="largest")
    assert mesh["vertices"].shape == (0, 3) and mesh["triangles"].shape == (0, 3) and mesh["normals"].shape == (0, 3)
    assert mesh["colors"].shape == (0, 3) and mesh["colors"].dtype == np.uint8 and mesh["component_sizes"].shape == (0,)
