"""Posing the body model on the device (csrc/hl_body.hip, humanliff_amd/body.py) and the renderer's hook for prebuilt tables.

The yardstick of every tolerance is the fp32 torch path the package had before these kernels (NeRF/deform.py: joint_transforms,
_pose_offsets, weights @ A, the 4x4 apply - and deform_tables for the table), measured against the same float64 truth: the kernels may
be off by at most 4 x what that path is off by (another, but fixed, order of summation).  The truth is the reference's own output
(tests/golden/body.npz) or the float64 restatement (tests/body_restatement.py)."""
import os

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import body_restatement as br

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body.npz")
FACTOR = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


_MODELS = {}


def models(V, seed, dev):
    """(cpu dict, float64 numpy dict, BodyModel on the device), made once per (V, seed)."""
    from humanliff_amd.body import load_body_model
    if (V, seed) not in _MODELS:
        cpu = syn.smpl_like_model(V, seed)
        _MODELS[(V, seed)] = (cpu, br.model64(cpu), load_body_model(cpu, dev))
    return _MODELS[(V, seed)]


def torch_path(cpu, poses, shapes, R, Th):
    """Today's fp32 ops on the CPU for one frame: vertices, joints (world), verts4."""
    from humanliff_amd.NeRF import deform
    poses, shapes = torch.as_tensor(poses, dtype=torch.float32).reshape(-1), torch.as_tensor(shapes, dtype=torch.float32).reshape(-1)
    R, Th = torch.as_tensor(R, dtype=torch.float32).reshape(3, 3), torch.as_tensor(Th, dtype=torch.float32).reshape(3)
    V = cpu["v_template"].shape[0]
    A = deform.joint_transforms(cpu, poses, shapes)
    T = (cpu["weights"] @ A.reshape(-1, 16)).reshape(V, 4, 4)
    sd = cpu["shapedirs"][..., :shapes.numel()]
    v_shaped = cpu["v_template"] + sd @ shapes
    v_posed = v_shaped + deform._pose_offsets(cpu, poses)
    vh = torch.cat([v_posed, torch.ones((V, 1))], dim=1)
    v_smpl = torch.matmul(T, vh[:, :, None])[:, :3, 0]
    rest = cpu["J_regressor"] @ v_shaped
    joints = torch.matmul(A[:, :3, :3], rest[:, :, None])[:, :, 0] + A[:, :3, 3]
    world = v_smpl @ R.t() + Th
    return {"vertices": world.numpy(), "joints": (joints @ R.t() + Th).numpy(), "verts4": ((world - Th) @ R).numpy()}


def errors(got, want):
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max()) for k in want}


def check(tag, kernel, yard, want):
    ek, ey = errors(kernel, want), errors(yard, want)
    for k in want:
        print(f"{tag} {k}: kernel {ek[k]:.3e}, fp32 torch path {ey[k]:.3e}")
    for k in want:
        assert ek[k] <= FACTOR * ey[k], (tag, k, ek[k], ey[k])


def frame(posed, f):
    return {"vertices": posed.vertices[f].cpu().numpy(), "joints": posed.joints[f].cpu().numpy(), "verts4": posed.verts4[f, :, :3].cpu().numpy()}


def test_golden_match(dev, golden):
    g = golden
    cpu, _, model = models(int(g["V"]), int(g["seed"]), dev)
    for name in ("b1", "b2"):
        poses, shapes, R, Th = g[f"{name}_poses"], g[f"{name}_shapes"], g[f"{name}_R"], g[f"{name}_Th"]
        posed = model.pose(torch.from_numpy(poses).to(dev), torch.from_numpy(shapes).to(dev), R, Th)
        want = {"vertices": g[f"{name}_vertices"].astype(np.float64), "joints": g[f"{name}_joints"].astype(np.float64)}
        want["verts4"] = (want["vertices"] - Th.astype(np.float64).reshape(3)) @ R.astype(np.float64)
        check(name, frame(posed, 0), torch_path(cpu, poses, shapes, R, Th), want)
        assert torch.all(posed.verts4[..., 3] == 0) and torch.isfinite(posed.table).all()
    big = model.big_pose()
    assert torch.equal(big.t_vertices, posed.vertices[0]) and torch.equal(big.t_world_bounds, posed.world_bounds[0])      # body 2 is the big pose


def test_bounds_are_the_reference_arithmetic_on_the_kernels_vertices(dev):
    _, _, model = models(1200, 3, dev)
    g = syn._gen(8)
    F = 5
    posed = model.pose((torch.randn((F, 72), generator=g) * 0.25).to(dev), (torch.randn((F, 10), generator=g) * 0.5).to(dev),
                       syn._rodrigues1(torch.tensor([0.3, -0.2, 0.5])).numpy(), np.array([0.1, -0.7, 0.4], dtype=np.float32))
    lo, hi = posed.vertices.amin(dim=1) - 0.05, posed.vertices.amax(dim=1) + 0.05
    lo[:, 1] -= 0.05
    hi[:, 1] += 0.05
    assert torch.equal(posed.world_bounds, torch.stack([lo, hi], dim=1))
    assert np.array_equal(posed.bounds_host()[2], br.bounds(posed.vertices[2].cpu().numpy()))
    # the dataset helper is that call: (world_bounds, vertices, params, joints) of one frame without the frame axis
    from humanliff_amd.SynBodyView_datasets import prepare_input
    params = {"poses": posed.poses[2:3], "shapes": posed.shapes[2:3], "R": posed.R[0], "Th": posed.Th[:1]}
    wb, vertices, same, joints = prepare_input(model, params)
    assert same is params and tuple(wb.shape) == (2, 3) and tuple(vertices.shape) == (1200, 3) and tuple(joints.shape) == (24, 3)
    assert torch.equal(wb, posed.world_bounds[2]) and torch.equal(vertices, posed.vertices[2]) and torch.equal(joints, posed.joints[2])


def _chunk():
    from humanliff_amd import _lib
    return int(_lib.lib().hl_body_chunk_frames())


@pytest.mark.parametrize("V", [257, 300, 1200])
@pytest.mark.parametrize("F", ["1", "3", "chunk", "chunk+1"])
def test_shapes_where_indexing_can_go_wrong(dev, V, F):
    F = {"1": 1, "3": 3, "chunk": _chunk(), "chunk+1": _chunk() + 1}[F]
    cpu, m64, model = models(V, 3, dev)
    assert float((cpu["weights"] == 0).float().mean()) > 0.5                  # blend weights with exact zeros
    g = syn._gen(1000 * V + F)
    poses = torch.randn((F, 72), generator=g) * 0.25
    poses[F // 2] = 0.0                                                        # an all-zero pose
    if F > 1:
        poses[0, 6:9] = 0.0                                                    # and a single zero joint vector
    per_frame = F != 3                                                         # F = 3: shapes, R and Th shared across the frames
    shapes = torch.randn((F if per_frame else 1, 10), generator=g) * 0.5
    Rs = torch.stack([syn._rodrigues1(torch.randn(3, generator=g) * 0.4) for _ in range(F if per_frame else 1)]).numpy()
    Ths = (torch.randn((F if per_frame else 1, 3), generator=g) * 0.2).numpy()
    pick = lambda a, f: a[f if per_frame else 0]  # noqa: E731
    args = (poses.to(dev), (shapes if per_frame else shapes[0]).to(dev), Rs if per_frame else Rs[0], Ths if per_frame else Ths[0])
    posed = model.pose(*args)
    assert torch.isfinite(posed.vertices).all() and torch.isfinite(posed.table).all() and torch.isfinite(posed.joints).all()
    for f in range(F):
        sh, Rf, Tf = pick(shapes, f).numpy(), pick(Rs, f), pick(Ths, f)
        t = br.pose(m64, syn.SMPL_PARENTS, poses[f].numpy(), sh, Rf, Tf)
        want = {"vertices": t["vertices"], "joints": t["joints"], "verts4": (t["vertices"] - Tf.astype(np.float64)) @ Rf.astype(np.float64)}
        check(f"V {V} F {F} frame {f}", frame(posed, f), torch_path(cpu, poses[f], sh, Rf, Tf), want)
    fields = ("vertices", "joints", "world_bounds", "verts4", "table")
    again = model.pose(*args)
    for k in fields:
        assert torch.equal(getattr(posed, k), getattr(again, k)), f"{k}: two runs differ"
    for f in range(F):                                                         # a batch is its frames posed one by one, bit for bit
        one = model.pose(poses[f].to(dev), pick(shapes, f).to(dev), pick(Rs, f), pick(Ths, f))
        for k in fields:
            assert torch.equal(getattr(posed, k)[f], getattr(one, k)[0]), f"{k}: frame {f} of the batch differs from the frame alone"


def test_table_against_todays_deform_tables(dev, golden):
    from humanliff_amd.NeRF import deform
    g = golden
    cpu, m64, model = models(int(g["V"]), int(g["seed"]), dev)
    posed = model.pose(torch.from_numpy(g["b1_poses"]).to(dev), torch.from_numpy(g["b1_shapes"]).to(dev), g["b1_R"], g["b1_Th"])   # pose scale 0.25
    tp = posed.tp_input(0)
    deform._TABLE_CACHE.clear()
    verts4_t, table_t, Rh, Th = deform.deform_tables(model.tensors, tp["params"], tp["t_params"], tp["vertices"])
    assert np.array_equal(Rh, g["b1_R"]) and np.array_equal(Th, g["b1_Th"].reshape(3))
    want, At = br.table(m64, syn.SMPL_PARENTS, g["b1_poses"], g["b1_shapes"], g["b2_poses"])
    got, yard = posed.table[0].cpu().numpy().astype(np.float64), table_t.cpu().numpy().astype(np.float64)
    for name, sl in (("t", slice(0, 3)), ("pose_off", slice(12, 15)), ("shape_off", slice(15, 18)), ("pose_off_big", slice(18, 21)),
                     ("Rbig", slice(21, 30)), ("tbig", slice(30, 33)), ("pad", slice(33, 36))):
        ek, ey = np.abs(got[:, sl] - want[:, sl]).max(), np.abs(yard[:, sl] - want[:, sl]).max()
        print(f"table {name}: kernel {ek:.3e}, deform_tables {ey:.3e}")
        assert ek <= FACTOR * ey, (name, ek, ey)
    assert np.linalg.cond(At).max() < 3.0                                      # well conditioned at this pose scale
    eye = np.eye(3)[None]
    rk = np.abs(got[:, 3:12].reshape(-1, 3, 3) @ At - eye).max()
    ry = np.abs(yard[:, 3:12].reshape(-1, 3, 3) @ At - eye).max()
    print(f"table Rinv residual: kernel {rk:.3e}, torch.inverse {ry:.3e}")
    assert rk <= FACTOR * ry
    assert torch.equal(posed.verts4[0, :, 3], verts4_t[:, 3])


def test_end_to_end_deform_matches_the_reference(dev, golden):
    from humanliff_amd.NeRF.deform import deform_target2c
    g = golden
    _, _, model = models(int(g["V"]), int(g["seed"]), dev)
    posed = model.pose(torch.from_numpy(g["b1_poses"]).to(dev), torch.from_numpy(g["b1_shapes"]).to(dev), g["b1_R"], g["b1_Th"])
    tp = posed.tp_input(0)
    assert set(tp) == {"params", "t_params", "vertices", "world_bounds", "t_world_bounds", "deform"}
    can, cd, box, ids = deform_target2c(model.tensors, tp, torch.from_numpy(g["pts"]).to(dev), torch.from_numpy(g["viewdirs"]).to(dev),
                                        return_ids=True)
    same = ids.cpu().numpy() == g["ids"]
    ep = np.abs(can.cpu().numpy()[0][same] - g["can_pts"][0][same]).max()
    ed = np.abs(cd.cpu().numpy()[0][same] - g["can_dirs"][0][same]).max()
    print(f"same nearest vertex {same.mean():.5f}; canonical points {ep:.3e}, directions {ed:.3e}")
    assert same.mean() > 0.9995
    assert ep < 2e-5 and ed < 2e-5
    assert np.abs(box.cpu().numpy() - g["box"]).max() < 2e-5                  # t_world_bounds: the big-pose body's bounds


# ---- the renderer's hook ----------------------------------------------------------------------------------------------------
def _view(dev, V=1500, H=32, W=32, N=16):
    cpu = syn.smpl_like_model(V, 7)
    pose = syn.smpl_like_pose(V, cpu, 17, n_points=8)
    centre = pose["vertices"][0].mean(0)
    lo, hi = pose["vertices"][0].min(0).values - 0.1, pose["vertices"][0].max(0).values + 0.1
    ro, rd, _, _ = syn.orbit_rays(4, 36, H, W)
    ro = ro + centre
    nr, fr = syn.near_far_from_bounds(torch.stack([lo, hi]).double().numpy(), ro.double().numpy(), rd.double().numpy())
    nr, fr = torch.from_numpy(nr).float(), torch.from_numpy(fr).float()
    u = torch.rand((H * W, N), generator=torch.Generator().manual_seed(9))
    tp = {k: v.to(dev) for k, v in pose.items() if k in ("vertices", "t_world_bounds")}
    tp["params"] = {k: v.to(dev) for k, v in pose["params"].items()}
    tp["t_params"] = {k: v.to(dev) for k, v in pose["t_params"].items()}
    tp["world_bounds"] = torch.stack([lo, hi])[None].to(dev)
    rays = (ro[None].to(dev), rd[None].to(dev), nr[None].to(dev), fr[None].to(dev))
    return cpu, tp, rays, u.to(dev), N


def _renderer(dev, cpu=None, test=True, **kw):
    from humanliff_amd.NeRF import Renderer
    r = Renderer(use_canonical_space=True, triplane_dim=64, triplane_ch=27, smpl_type='smpl', test=test, **kw)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(dev)
    if cpu is not None:
        r.SMPL_NEUTRAL = {k: v.to(dev) for k, v in cpu.items()}
    return r


def _render(r, tp, rays, u, N, planes):
    out = r.render(tp, None, None, *rays, planes, N, False, n_samples=N, u=u)
    return [out[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")]


def test_hook_is_a_pass_through(dev):
    from humanliff_amd.NeRF import deform
    cpu, tp, rays, u, N = _view(dev)
    r = _renderer(dev, cpu)
    planes = syn.triplane(seed=11, H=64, W=64).to(dev)
    plain = _render(r, tp, rays, u, N, planes)
    assert float(plain[1].max()) > 0.05                                        # the body is hit
    tables = deform.deform_tables(r.SMPL_NEUTRAL, tp["params"], tp["t_params"], tp["vertices"])
    for hooked in (dict(tp, deform=tables), dict(tp, deform=[tables])):
        got = _render(r, hooked, rays, u, N, planes)
        for a, b in zip(plain, got):
            assert torch.equal(a, b)


def test_hook_is_used(dev, monkeypatch):
    from humanliff_amd.NeRF import deform
    cpu, tp, rays, u, N = _view(dev)
    r = _renderer(dev, cpu)
    planes = syn.triplane(seed=11, H=64, W=64).to(dev)
    tables = deform.deform_tables(r.SMPL_NEUTRAL, tp["params"], tp["t_params"], tp["vertices"])
    grid = r.density_grid(tp, planes, resolution=8)

    def refuse(*a, **k):
        raise AssertionError("deform_tables was called although tp_input['deform'] is there")
    monkeypatch.setattr(deform, "deform_tables", refuse)
    hooked = dict(tp, deform=tables)
    _render(r, hooked, rays, u, N, planes)
    assert torch.equal(r.density_grid(hooked, planes, resolution=8), grid)
    deform.deform_target2c(r.SMPL_NEUTRAL, hooked, tp["vertices"][:, :64])
    rt = _renderer(dev, cpu, test=False)                                       # training geometry: a batch of two entries, tables per entry
    two = lambda d: {k: torch.cat([v, v]) for k, v in d.items()}  # noqa: E731
    tp2 = {"params": two(tp["params"]), "t_params": two(tp["t_params"]), "vertices": torch.cat([tp["vertices"]] * 2),
           "t_world_bounds": torch.cat([tp["t_world_bounds"]] * 2), "world_bounds": torch.cat([tp["world_bounds"]] * 2)}
    sub = [torch.cat([t[:, :128], t[:, :128]]) for t in rays]
    tri = torch.cat([planes, planes]).requires_grad_(True)
    un = torch.cat([u[:128], u[:128]])
    noise = torch.zeros((2 * 128 * 2 * N, 1), device=dev)
    out = rt.render(dict(tp2, deform=[tables, tables]), None, None, *sub, tri, N, False, n_samples=N, u=un, noise=noise)
    assert torch.isfinite(out["rgb_map"]).all() and torch.equal(out["rgb_map"][0], out["rgb_map"][1])
    for call in (lambda: _render(r, tp, rays, u, N, planes), lambda: r.density_grid(tp, planes, resolution=8),
                 lambda: rt.render(tp2, None, None, *sub, tri, N, False, n_samples=N, u=un, noise=noise)):
        with pytest.raises(AssertionError, match="deform_tables was called"):  # without the key, the three places still build the tables
            call()


def test_loader_equals_assigning_the_model_by_hand(dev):
    from humanliff_amd.body import BodyModel
    cpu, tp, rays, u, N = _view(dev)
    planes = syn.triplane(seed=11, H=64, W=64).to(dev)
    by_hand = _render(_renderer(dev, cpu), tp, rays, u, N, planes)
    r = _renderer(dev)
    assert r.SMPL_NEUTRAL is None and r.body_model is None
    model = r.load_body_model(dict(cpu), dev)
    assert isinstance(model, BodyModel) and r.body_model is model and r.SMPL_NEUTRAL is model.tensors and r.faces is model.tensors["f"]
    for got in (_render(r, tp, rays, u, N, planes), _render(_renderer(dev, body_model=model), tp, rays, u, N, planes)):
        for a, b in zip(by_hand, got):
            assert torch.equal(a, b)
