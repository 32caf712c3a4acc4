"""Animating an extracted mesh on the MI355X (csrc/hl_mesh_animate.hip, humanliff_amd/NeRF/animate.py, the forward rows of
humanliff_amd/body.py) against the numpy restatement (tests/mesh_animate_restatement.py).  DESIGN.md "Animating the mesh".

The tolerance rule is the one of tests/test_body_gpu.py: against the float64 restatement the kernel may be off by at most FACTOR = 4 x
what the float32 restatement - the same formulas in the kernel's stated order - is off by ON THE SAME INPUTS.  The inputs of the two
entry points are the posed body's own device outputs (its forward rows, verts4, R | Th, transl) and the mesh, so all three - kernel,
float32 and float64 restatement - read the rows and verts4 the device wrote, the float64 one after an exact widening.  (What the rows
themselves are worth is the pass-through test's subject: there they are held against tests/body_restatement.pose.)

Mesh points: body vertices of the bind frame picked at random plus N(0, 0.02^2) noise from numpy.random.default_rng(7), 4097 of them;
a case of N points takes the first N.

Near-ties.  A point is left out of the id comparison when its float64 squared-distance gap is below 1e-6 between neighbours K - 1 and
K (the set) or between any two kept neighbours (their order); the bind test asserts that at most 0.5 % are left out - on the full
4097 points, a share of 1 or 255 points resolving no 0.5 %.  The share is a property of the body and the points alone, and it can be
estimated before any kernel runs: body vertices are uniform in a 0.9 x 1.7 x 0.4 box, density rho = V / 0.612, so the k-th neighbour
sits at squared distance s_k = (k / (4.19 rho))^(2/3), neighbours arrive there at the rate 2 pi rho sqrt(s_k) per unit of s, and the
expected share is 1e-6 x the sum of those rates over the K gaps: 0.3 % for (V 1200, K 4), 0.2 % for (V 2300, K 2), but 0.8 % for
(V 1200, K 8) (0.61 % counted in float64 alone on such a body) - that pairing cannot hold the 0.5 % whatever the kernel does.  So K = 8
is bound on the 257-vertex body (0.15 % counted), where the eight-slot insertion runs the same code, and V = 2300 - a size at which the
search stages a second LDS tile of 2048 vertices - is bound with K = 1 and 2."""
import os

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import body_restatement as br
from tests import mesh_animate_restatement as ma
from tests import smplx_restatement as sr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body.npz")
FACTOR = 4.0
GAP = 1e-6
NMAX = 4097
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _chunk():
    from humanliff_amd import _lib
    return int(_lib.lib().hl_body_chunk_frames())


def _frames(F):
    return {"1": 1, "3": 3, "chunk+1": _chunk() + 1}[F]


_MODELS, _SCENES = {}, {}


def models(V, dev, seed=3):
    from humanliff_amd.body import load_body_model
    if (V, seed) not in _MODELS:
        cpu = syn.smpl_like_model(V, seed)
        _MODELS[(V, seed)] = (cpu, br.model64(cpu), load_body_model(cpu, dev))
    return _MODELS[(V, seed)]


def mesh_points(world_vertices):
    """(x, n) float32: 4097 points near the body's vertices and unit normals, one of them zero."""
    rng = np.random.default_rng(7)
    V = world_vertices.shape[0]
    x = (world_vertices[rng.integers(0, V, NMAX)].astype(F64) + rng.normal(0.0, 0.02, (NMAX, 3))).astype(F32)
    n = rng.normal(size=(NMAX, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n[0] = 0.0
    return x, n


class Scene:
    """A posed SMPL-like body of F frames with forward rows, host copies of what the kernels read, mesh points near frame `b`, and the
    restatement's binds of them, each computed once."""

    def __init__(self, V, F, dev):
        self.cpu, self.m64, self.model = models(V, dev)
        g = syn._gen(1000 * V + F)
        self.poses = torch.randn((F, 72), generator=g) * 0.25
        self.shapes = torch.randn((10,), generator=g) * 0.5
        self.per_frame = F == 3                                         # F = 3: R and Th of their own per frame
        n_rt = F if self.per_frame else 1
        self.Rs = torch.stack([syn._rodrigues1(torch.tensor([0.3, -0.2, 0.5]) + torch.randn(3, generator=g) * 0.2) for _ in range(n_rt)]).numpy()
        self.Ths = (torch.tensor([0.1, -0.7, 0.4]) + torch.randn((n_rt, 3), generator=g) * 0.2).numpy()
        self.dev, self.V, self.F, self.b = dev, V, F, min(1, F - 1)
        self.posed = self.pose()
        self.rows, self.verts4 = self.posed.rows.cpu().numpy(), self.posed.verts4.cpu().numpy()
        self.x, self.n = mesh_points(self.posed.vertices[self.b].cpu().numpy())
        self._found, self._binds = {}, {}

    def rt(self, f):
        return (self.Rs[f], self.Ths[f]) if self.per_frame else (self.Rs[0], self.Ths[0])

    def pose(self, f=None, **kw):
        kw.setdefault("forward_rows", True)
        if f is None:
            return self.model.pose(self.poses.to(self.dev), self.shapes.to(self.dev), self.Rs if self.per_frame else self.Rs[0],
                                   self.Ths if self.per_frame else self.Ths[0], **kw)
        return self.model.pose(self.poses[f:f + 1].to(self.dev), self.shapes.to(self.dev), *self.rt(f), **kw)

    def bind(self, K, N, dtype):
        if (K, N, dtype) not in self._binds:
            R, Th = self.rt(self.b)
            if dtype not in self._found:
                self._found[dtype] = ma.search(self.x, self.verts4[self.b], R, Th, dtype)
            found = tuple(a[:N] for a in self._found[dtype])
            self._binds[(K, N, dtype)] = ma.bind(self.x[:N], self.n[:N], self.verts4[self.b], self.rows[self.b], R, Th, K, dtype, found=found)
        return self._binds[(K, N, dtype)]

    def repose(self, t, f, dtype, normals=True):
        return ma.repose(t["ids"], t["weights"], t["rest"], t["rest_normals"] if normals else None, self.rows[f], *self.rt(f), dtype=dtype)


def scene(V, F, dev):
    if (V, F) not in _SCENES:
        _SCENES[(V, F)] = Scene(V, F, dev)
    return _SCENES[(V, F)]


def check(tag, kernel, yard, want):
    ek = float(np.abs(np.asarray(kernel, dtype=F64) - want).max())
    ey = float(np.abs(np.asarray(yard, dtype=F64) - want).max())
    print(f"{tag}: kernel {ek:.3e}, fp32 restatement {ey:.3e}")
    assert ek <= FACTOR * ey, (tag, ek, ey)


def excluded_points(t64):
    return (np.diff(t64["d_sorted"], axis=1) < GAP).any(axis=1)


# ---- 1. bind ------------------------------------------------------------------------------------------------------------------
BIND_CASES = [(257, 1, NMAX), (257, 4, NMAX), (257, 8, NMAX), (257, 3, 255), (257, 4, 1), (1200, 1, NMAX), (1200, 4, NMAX), (1200, 1, 255),
              (2300, 1, NMAX), (2300, 2, NMAX)]


@pytest.mark.parametrize("V,K,N", BIND_CASES)
def test_bind(dev, V, K, N):
    from humanliff_amd.NeRF import animate
    sc = scene(V, 3, dev)
    b = animate.bind_mesh(sc.x[:N], sc.posed, frame=sc.b, neighbours=K, normals=sc.n[:N])
    assert (b.N, b.K, b.model) == (N, K, sc.model) and b.ids.dtype == torch.int32 and tuple(b.ids.shape) == (N, K)
    assert tuple(b.weights.shape) == (N, K) and tuple(b.rest.shape) == tuple(b.rest_normals.shape) == (N, 3)
    t64, t32 = sc.bind(K, N, F64), sc.bind(K, N, F32)
    out = excluded_points(t64)
    keep = ~out
    ids = b.ids.cpu().numpy()
    print(f"V {V} K {K} N {N}: {out.mean() * 100:.3f} % of the points are near-ties in float64; the kernel's ids differ on "
          f"{int((ids != t64['ids']).any(axis=1).sum())} points, the fp32 restatement's on {int((t32['ids'] != t64['ids']).any(axis=1).sum())}")
    if N == NMAX:
        assert out.mean() <= 0.005
    assert np.array_equal(ids[keep], t64["ids"][keep])
    assert np.array_equal(t32["ids"][keep], t64["ids"][keep])               # (the yardstick speaks of the same neighbours)
    w = b.weights.cpu().numpy()
    assert np.abs(w.astype(F64).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -23 and (w > 0).all()
    if keep.any():
        check(f"V {V} K {K} N {N} weights", w[keep], t32["weights"][keep], t64["weights"][keep])
        check(f"V {V} K {K} N {N} rest", b.rest.cpu().numpy()[keep], t32["rest"][keep], t64["rest"][keep])
        check(f"V {V} K {K} N {N} rest normals", b.rest_normals.cpu().numpy()[keep], t32["rest_normals"][keep], t64["rest_normals"][keep])
    assert bool((b.rest_normals[0] == 0).all())                              # point 0 carries the zero normal


# ---- 2. round trip and repose ------------------------------------------------------------------------------------------------------
REPOSE_CASES = [(257, 4, NMAX, "chunk+1"), (257, 1, 255, "3"), (257, 8, 1, "chunk+1"), (1200, 4, 255, "1"), (1200, 8, NMAX, "3"),
                (2300, 2, NMAX, "1")]


@pytest.mark.parametrize("V,K,N,F", REPOSE_CASES)
def test_round_trip_and_repose(dev, V, K, N, F):
    from humanliff_amd.NeRF import animate
    F = _frames(F)
    sc = scene(V, F, dev)
    x, n = sc.x[:N], sc.n[:N]
    b = animate.bind_mesh(torch.from_numpy(x).to(dev), sc.posed, frame=sc.b, neighbours=K, normals=torch.from_numpy(n).double().to(dev))
    out = b.repose(sc.posed)
    assert tuple(out["vertices"].shape) == tuple(out["normals"].shape) == (F, N, 3) and tuple(out["world_bounds"].shape) == (F, 2, 3)
    verts, nrm = out["vertices"].cpu().numpy(), out["normals"].cpu().numpy()
    assert np.isfinite(verts).all() and np.isfinite(nrm).all()
    t64, t32 = sc.bind(K, N, F64), sc.bind(K, N, F32)
    agree = (b.ids.cpu().numpy() == t64["ids"]).all(axis=1) & (t32["ids"] == t64["ids"]).all(axis=1)
    assert agree.mean() >= 0.99 or N == 1
    tag = f"V {V} K {K} N {N} F {F}"
    # the bind frame gives the input back (whichever neighbours a near-tie chose)
    yv, yn = sc.repose(t32, sc.b, F32)
    n64 = n.astype(F64)
    unit = n64 / np.where(np.linalg.norm(n64, axis=1, keepdims=True) > 0, np.linalg.norm(n64, axis=1, keepdims=True), 1.0)
    check(f"{tag} bind frame vertices", verts[sc.b], yv, x.astype(F64))
    check(f"{tag} bind frame normals", nrm[sc.b], yn, unit)
    for f in range(F):
        if f == sc.b or not agree.any():
            continue
        wv, wn = sc.repose(t64, f, F64)
        yv, yn = sc.repose(t32, f, F32)
        check(f"{tag} frame {f} vertices", verts[f][agree], yv[agree], wv[agree])
        check(f"{tag} frame {f} normals", nrm[f][agree], yn[agree], wn[agree])
    length = np.linalg.norm(nrm.astype(F64), axis=2)
    assert (nrm[:, 0] == 0).all() and (np.abs(length[:, 1:] - 1.0) < 1e-6).all()       # point 0 carries the zero normal
    keys = ("vertices", "normals", "world_bounds")
    again = b.repose(sc.posed)
    for k in keys:
        assert torch.equal(out[k], again[k]), f"{k}: two runs differ"
    for f in range(F):                                                         # a batch is its frames reposed one by one, bit for bit
        alone = b.repose(sc.pose(f))
        by_index = b.repose(sc.posed, frames=f)
        for k in keys:
            assert torch.equal(alone[k][0], out[k][f]), f"{k}: frame {f} of the batch differs from the frame alone"
            assert torch.equal(by_index[k], out[k][f:f + 1])
    if F >= 3:
        part = b.repose(sc.posed, frames=slice(1, 3))
        for k in keys:
            assert torch.equal(part[k], out[k][1:3])
    bare = b.repose(sc.posed, normals=False, bounds=False)
    assert bare["normals"] is None and bare["world_bounds"] is None and torch.equal(bare["vertices"], out["vertices"])


# ---- 3. bounds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [NMAX, 255, 1])
@pytest.mark.parametrize("margins", [(0.05, 0.05), (0.02, 0.1)])
def test_bounds_are_the_reference_arithmetic_on_the_kernels_vertices(dev, N, margins):
    from humanliff_amd.NeRF import animate
    sc = scene(257, _chunk() + 1, dev)
    b = animate.bind_mesh(sc.x[:N], sc.posed, frame=sc.b, neighbours=4)
    out = b.repose(sc.posed, margin=margins[0], y_margin=margins[1])
    assert out["normals"] is None
    lo, hi = out["vertices"].amin(dim=1) - margins[0], out["vertices"].amax(dim=1) + margins[0]
    lo[:, 1] -= margins[1]
    hi[:, 1] += margins[1]
    assert torch.equal(out["world_bounds"], torch.stack([lo, hi], dim=1))


# ---- 4. the renderer's rule ----------------------------------------------------------------------------------------------------
def test_one_neighbour_is_the_renderers_deformation(dev):
    """K = 1 against the reference's own deform_target2c outputs (tests/golden/body.npz), with the two numbers
    test_body_gpu.py::test_end_to_end_deform_matches_the_reference holds hl_deform_points to on the same data."""
    from humanliff_amd.NeRF import animate
    g = dict(np.load(GOLDEN))
    _, _, model = models(int(g["V"]), dev, int(g["seed"]))
    posed = model.pose(torch.from_numpy(g["b1_poses"]).to(dev), torch.from_numpy(g["b1_shapes"]).to(dev), g["b1_R"], g["b1_Th"], forward_rows=True)
    b = animate.bind_mesh(g["pts"][0], posed, neighbours=1)
    ids = b.ids[:, 0].cpu().numpy()
    same = ids == g["ids"]
    row = posed.table[0].cpu().numpy().astype(F64)[ids]
    u = b.rest.cpu().numpy().astype(F64)
    can = np.einsum("nrc,nc->nr", row[:, 21:30].reshape(-1, 3, 3), u - row[:, 15:18] + row[:, 18:21]) + row[:, 30:33]
    e = np.abs(can[same] - g["can_pts"][0][same]).max()
    print(f"same nearest vertex {same.mean():.5f}; canonical points from the binding's rest positions {e:.3e}")
    assert same.mean() >= 0.9995 and e < 2e-5
    assert bool((b.weights == 1.0).all())


# ---- 5. SMPL-X -----------------------------------------------------------------------------------------------------------------
def test_smplx_round_trip_and_transl(dev):
    """The guard against mixing the two shape sets and against losing transl: a 400-column SMPL-X-like model (two sets), jaw and finger
    poses, expression and transl all non-zero."""
    from humanliff_amd.body import load_smplx_model
    from humanliff_amd.NeRF import animate
    from tests.test_smplx_gpu import PART_NAMES, torch_path, truth
    V, F, N, K = 300, 3, 1000, 4
    cpu = syn.smplx_like_model(V, 23, 400)
    m64, model = sr.model64(cpu), load_smplx_model(cpu, dev)
    assert model.two_sets == 1
    g = syn._gen(77)
    d = {k: torch.randn((F, 3 * n), generator=g) * 0.25 for k, n in sr.PARTS}
    d["betas"], d["expression"] = torch.randn((1, 10), generator=g) * 0.5, torch.randn((F, 10), generator=g) * 0.5
    d["transl"] = torch.randn((F, 3), generator=g) * 0.3
    for k in PART_NAMES + ["expression"]:
        d[k][2] = d[k][0]                                                       # frame 2: frame 0 with another transl
    assert float(d["jaw_pose"].abs().min()) > 0 and float(d["left_hand_pose"].abs().min()) > 0
    R, Th = syn._rodrigues1(torch.tensor([0.3, -0.2, 0.5])).numpy(), np.array([0.1, -0.7, 0.4], dtype=F32)
    args = [d[k].to(dev) for k in ("global_orient", "body_pose", "betas", "expression", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose",
                                   "right_hand_pose", "transl")]
    plain, posed = model.pose(*args, R, Th), model.pose(*args, R, Th, forward_rows=True)
    assert plain.rows is None and tuple(posed.rows.shape) == (F, V, 16)
    for k in ("vertices", "joints", "world_bounds", "verts4", "table"):
        assert torch.equal(getattr(plain, k), getattr(posed, k)), k
    rows, verts4, tr = posed.rows.cpu().numpy(), posed.verts4.cpu().numpy(), d["transl"].numpy()
    assert np.array_equal(rows[0], rows[2])
    # the rows are shape set 1's: applied to set 1's rest vertices they give the posed body, to set 2's they do not
    cols, mean = sr.columns(400), sr.pose_mean(m64, True)
    coef = np.concatenate([d["betas"][0].numpy(), d["expression"][0].numpy()]).astype(F64)
    poses = sr.full_pose({k: d[k][0].numpy() for k in PART_NAMES}, mean)
    sets = {1: np.concatenate([m64["shapedirs"][..., :10], m64["shapedirs"][..., 300:310]], axis=-1), 2: m64["shapedirs"][..., :20]}
    r64 = rows[0].astype(F64)
    want = truth(m64, cols, mean, d, 0, R, Th)["verts4"]
    errs = {}
    for s, sd in sets.items():
        lbs = sr._lbs(m64, syn.SMPLX_PARENTS, poses, sd, coef)
        v_rest = m64["v_template"] + lbs["shape_off"] + lbs["pose_off"]
        errs[s] = np.abs(np.einsum("vrc,vc->vr", r64[:, :9].reshape(V, 3, 3), v_rest) + r64[:, 9:12] + tr[0].astype(F64) - want).max()
    yard = np.abs(torch_path(cpu, cols, mean, d, 0, R, Th)["verts4"].astype(F64) - want).max()
    print(f"SMPL-X rows on set 1's rest vertices {errs[1]:.3e} (fp32 torch path {yard:.3e}); on set 2's {errs[2]:.3e}")
    assert errs[1] <= FACTOR * yard and errs[2] > 1e-3
    x, n = mesh_points(posed.vertices[0].cpu().numpy())
    x, n = x[:N], n[:N]
    b = animate.bind_mesh(x, posed, frame=0, neighbours=K, normals=n)
    out = b.repose(posed)
    verts = out["vertices"].cpu().numpy()
    t32 = ma.bind(x, n, verts4[0], rows[0], R, Th, K, F32, transl=tr[0])
    t64 = ma.bind(x, n, verts4[0], rows[0], R, Th, K, F64, transl=tr[0])
    agree = (b.ids.cpu().numpy() == t64["ids"]).all(axis=1) & (t32["ids"] == t64["ids"]).all(axis=1)
    assert agree.mean() >= 0.99
    check("SMPL-X rest", b.rest.cpu().numpy()[agree], t32["rest"][agree], t64["rest"][agree])
    rep = lambda t, f, dt: ma.repose(t["ids"], t["weights"], t["rest"], t["rest_normals"], rows[f], R, Th, transl=tr[f], dtype=dt)  # noqa: E731
    check("SMPL-X bind frame vertices", verts[0], rep(t32, 0, F32)[0], x.astype(F64))
    moved = x.astype(F64) + (tr[2].astype(F64) - tr[0].astype(F64)) @ R.astype(F64).T
    check("SMPL-X frame with another transl", verts[2], rep(t32, 2, F32)[0], moved)
    assert np.abs(tr[2] - tr[0]).max() > 0.1
    check("SMPL-X frame 1 vertices", verts[1][agree], rep(t32, 1, F32)[0][agree], rep(t64, 1, F64)[0][agree])
    check("SMPL-X frame 1 normals", out["normals"].cpu().numpy()[1][agree], rep(t32, 1, F32)[1][agree], rep(t64, 1, F64)[1][agree])
    alone = b.repose(model.pose(*[a[2:3] if a.shape[0] == F else a for a in args], R, Th, forward_rows=True))
    assert torch.equal(alone["vertices"][0], out["vertices"][2]) and torch.equal(alone["world_bounds"][0], out["world_bounds"][2])


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------
def test_edges(dev):
    from humanliff_amd import _lib
    from humanliff_amd.NeRF import animate
    sc = scene(257, 3, dev)
    empty = animate.bind_mesh(np.zeros((0, 3)), sc.posed, neighbours=4, normals=np.zeros((0, 3)))
    assert tuple(empty.ids.shape) == tuple(empty.weights.shape) == (0, 4) and tuple(empty.rest.shape) == tuple(empty.rest_normals.shape) == (0, 3)
    out = empty.repose(sc.posed, frames=slice(0, 2))
    assert tuple(out["vertices"].shape) == tuple(out["normals"].shape) == (2, 0, 3) and tuple(out["world_bounds"].shape) == (2, 2, 3)
    assert out["vertices"].is_cuda and out["vertices"].dtype == torch.float32
    for k in (0, 9, 258):
        with pytest.raises(ValueError, match="neighbours"):
            animate.bind_mesh(sc.x[:8], sc.posed, neighbours=k)
    animate.bind_mesh(sc.x[:8], sc.posed, neighbours=8)
    with pytest.raises(ValueError, match="forward_rows=True"):
        animate.bind_mesh(sc.x[:8], sc.pose(forward_rows=False))
    b = animate.bind_mesh(sc.x[:8], sc.posed)
    assert b.K == 4 and b.rest_normals is None and b.repose(sc.posed)["normals"] is None
    with pytest.raises(ValueError, match="forward_rows=True"):
        b.repose(sc.pose(forward_rows=False))
    other = scene(1200, 3, dev)
    with pytest.raises(ValueError, match="another body model"):
        b.repose(other.posed)
    with pytest.raises(RuntimeError, match="no CPU path"):
        animate.bind_mesh(torch.from_numpy(sc.x[:8]), sc.posed)
    with pytest.raises(ValueError):
        animate.bind_mesh(sc.x[:8], sc.posed, normals=sc.n[:7])
    # the library refuses the same sizes before any launch (and N == 0 is none of them)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    p = _lib.ptr
    rows, v4, rt = sc.posed.rows, sc.posed.verts4, sc.posed.rt
    pts = torch.from_numpy(sc.x[:8]).to(dev)
    for V, K in ((257, 0), (257, 9), (3, 4), (0, 1)):
        assert L.hl_mesh_bind(p(pts), None, 8, p(v4[0]), p(rows[0]), V, p(rt[0]), None, K, p(b.ids, torch.int32), p(b.weights), p(b.rest), None, st) != 0
    assert L.hl_mesh_bind(None, None, 0, p(v4[0]), p(rows[0]), 257, p(rt[0]), None, 4, None, None, None, None, st) == 0
    verts = torch.empty((3, 8, 3), device=dev)
    for V, K, F in ((257, 0, 3), (257, 9, 3), (3, 4, 3), (0, 1, 3), (257, 4, 0)):
        assert L.hl_mesh_repose(p(b.ids, torch.int32), p(b.weights), p(b.rest), None, 8, K, p(rows), V, F, p(rt), 12, None, p(verts), None, None,
                                0.05, 0.05, None, 0, st) != 0
    assert L.hl_mesh_repose(None, None, None, None, 0, 4, p(rows), 257, 3, p(rt), 12, None, None, None, None, 0.05, 0.05, None, 0, st) == 0
    assert L.hl_mesh_repose_scratch_bytes(4097, 3) == 3 * 17 * 6 * 4 and L.hl_mesh_repose_scratch_bytes(0, 3) == 0


# ---- 7. pass-through -----------------------------------------------------------------------------------------------------------
def test_forward_rows_change_nothing_else_and_are_the_skinning_transform(dev):
    from tests.test_body_gpu import torch_path
    sc = scene(1200, 3, dev)
    plain = sc.pose(forward_rows=False)
    assert plain.rows is None and tuple(sc.posed.rows.shape) == (3, 1200, 16)
    for k in ("vertices", "joints", "world_bounds", "verts4", "table"):
        assert torch.equal(getattr(plain, k), getattr(sc.posed, k)), k
    for f in range(3):
        R, Th = sc.rt(f)
        t = br.pose(sc.m64, syn.SMPL_PARENTS, sc.poses[f].numpy(), sc.shapes.numpy(), R, Th)
        r64 = sc.rows[f].astype(F64)
        v_rest = sc.m64["v_template"] + t["shape_off"] + t["pose_off"]
        got = np.einsum("vrc,vc->vr", r64[:, :9].reshape(-1, 3, 3), v_rest) + r64[:, 9:12]
        want = (t["vertices"] - Th.astype(F64)) @ R.astype(F64)
        check(f"rows of frame {f} applied to the restatement's rest vertices", got, torch_path(sc.cpu, sc.poses[f], sc.shapes, R, Th)["verts4"], want)
        assert np.abs(r64[:, 12:15] - t["pose_off"]).max() < 1e-6 and (r64[:, 15] == 0).all()


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
def test_extracted_mesh_follows_the_body(dev):
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.recon_NeRF import Renderer as ReconRenderer
    from tests.test_mesh_finish_gpu import _planted_scene, _twins
    planes, mlp = _planted_scene()
    name, extract_mesh = next(iter(_twins(planes, mlp, dev)))[:2]
    mesh = extract_mesh()
    N = len(mesh["vertices"])
    assert N > 1000 and mesh["normals"].shape == (N, 3)
    sc = scene(257, 3, dev)
    posed = sc.model.pose(sc.poses[:2].to(dev), sc.shapes.to(dev), forward_rows=True)      # (R = I, Th = 0: the body sits inside the scene's bounds)
    for r in (Renderer(use_canonical_space=False, triplane_dim=64, triplane_ch=27, test=True),
              ReconRenderer(use_canonical_space=False, num_instances=1, triplane_dim=64, triplane_ch=27, test=True)):
        b = r.bind_mesh(mesh, posed, frame=0)
        assert b.N == N and b.K == 4 and b.triangles is mesh["triangles"] and b.colors is mesh["colors"]
        out = b.repose(posed)
        assert tuple(out["vertices"].shape) == tuple(out["normals"].shape) == (2, N, 3)
        assert all(bool(torch.isfinite(out[k]).all()) for k in out)
        x32 = mesh["vertices"].astype(F32)
        n32 = mesh["normals"].astype(F32)
        rows, verts4 = posed.rows.cpu().numpy(), posed.verts4.cpu().numpy()
        t32 = ma.bind(x32, n32, verts4[0], rows[0], np.eye(3), np.zeros(3), 4, F32)
        yv, _ = ma.repose(t32["ids"], t32["weights"], t32["rest"], None, rows[0], np.eye(3), np.zeros(3), dtype=F32)
        check(f"{type(r).__module__}: extracted vertices back in the bind frame", out["vertices"][0].cpu().numpy(), yv, mesh["vertices"])
        assert float((out["vertices"][1] - out["vertices"][0]).abs().max()) > 1e-3           # and the other frame moved them
