"""Posing an SMPL-X body on the device (csrc/hl_body.hip, humanliff_amd/body.py: SmplxModel), the renderer's hook for its tables and the
SynBody loader's smpl_type='smplx'.

The truth is the reference's own float64 output (tests/golden/smplx.npz: smplx.body_models.SMPLX with dtype=torch.float64) or the float64
restatement (tests/smplx_restatement.py).  The yardstick of every tolerance is an fp32 evaluation of the same rule against that truth -
the reference's own fp32 run, whose error the golden file records, or the fp32 torch path made from NeRF/deform.py's generic functions on
the CPU: the kernels may be off by at most FACTOR = 4 x what that is off by (another, but fixed, order of summation), as in
tests/test_body_gpu.py."""
import os

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import smplx_restatement as sr
from tests import synbody_fixture as fx

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplx.npz")
FACTOR = 4.0
PART_NAMES = [k for k, _ in sr.PARTS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


_MODELS = {}


def models(V, seed, cols, flat, dev):
    """(cpu dict, float64 numpy dict, SmplxModel on the device), made once per key."""
    from humanliff_amd.body import load_smplx_model
    key = (V, seed, cols)
    if key not in _MODELS:
        cpu = syn.smplx_like_model(V, seed, cols)
        _MODELS[key] = (cpu, sr.model64(cpu))
    if key + (flat,) not in _MODELS:
        _MODELS[key + (flat,)] = load_smplx_model(_MODELS[key][0], dev, flat_hand_mean=flat)
    return _MODELS[key] + (_MODELS[key + (flat,)],)


def random_inputs(F, seed, shared_betas):
    g = syn._gen(seed)
    d = {k: torch.randn((F, 3 * n), generator=g) * 0.25 for k, n in sr.PARTS}
    d["betas"] = torch.randn((1 if shared_betas else F, 10), generator=g) * 0.5
    d["expression"] = torch.randn((F, 10), generator=g) * 0.5
    d["transl"] = torch.randn((F, 3), generator=g) * 0.3
    return d


def torch_path(cpu, cols, mean, d, f, R, Th):
    """The rule in fp32 torch ops on the CPU for frame f of the inputs d: vertices, joints (world), verts4."""
    from humanliff_amd.NeRF import deform
    nb, e0, ne = cols
    poses = torch.cat([d[k][f].reshape(-1) for k in PART_NAMES]) + torch.as_tensor(mean, dtype=torch.float32)
    coef = torch.cat([d["betas"][f if d["betas"].shape[0] > 1 else 0], d["expression"][f]])
    R, Th = torch.as_tensor(R, dtype=torch.float32).reshape(3, 3), torch.as_tensor(Th, dtype=torch.float32).reshape(3)
    m = dict(cpu, shapedirs=torch.cat([cpu["shapedirs"][..., :nb], cpu["shapedirs"][..., e0:e0 + ne]], dim=-1))
    V = m["v_template"].shape[0]
    A = deform.joint_transforms(m, poses, coef)
    T = (m["weights"] @ A.reshape(-1, 16)).reshape(V, 4, 4)
    v_shaped = m["v_template"] + m["shapedirs"] @ coef
    vh = torch.cat([v_shaped + deform._pose_offsets(m, poses), torch.ones((V, 1))], dim=1)
    v = torch.matmul(T, vh[:, :, None])[:, :3, 0] + d["transl"][f]
    rest = m["J_regressor"] @ v_shaped
    joints = torch.matmul(A[:, :3, :3], rest[:, :, None])[:, :, 0] + A[:, :3, 3] + d["transl"][f]
    world = v @ R.t() + Th
    return {"vertices": world.numpy(), "joints": (joints @ R.t() + Th).numpy(), "verts4": ((world - Th) @ R).numpy()}


def truth(m64, cols, mean, d, f, R, Th):
    poses = sr.full_pose({k: d[k][f].numpy() for k in PART_NAMES}, mean)
    coef = np.concatenate([d["betas"][f if d["betas"].shape[0] > 1 else 0].numpy(), d["expression"][f].numpy()]).astype(np.float64)
    t = sr.pose(m64, syn.SMPLX_PARENTS, poses, coef, cols, d["transl"][f].numpy(), R, Th)
    t["verts4"] = (t["vertices"] - np.asarray(Th, dtype=np.float64).reshape(3)) @ np.asarray(R, dtype=np.float64).reshape(3, 3)
    return t


def errors(got, want):
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max()) for k in got}


def frame(posed, f):
    return {"vertices": posed.vertices[f].cpu().numpy(), "joints": posed.joints[f].cpu().numpy(), "verts4": posed.verts4[f, :, :3].cpu().numpy()}


def pose(model, d, dev, R=None, Th=None, f=None):
    pick = (lambda t: t.to(dev)) if f is None else (lambda t: t[f:f + 1].to(dev))
    return model.pose(pick(d["global_orient"]), pick(d["body_pose"]), d["betas"].to(dev) if d["betas"].shape[0] == 1 else pick(d["betas"]),
                      pick(d["expression"]), pick(d["jaw_pose"]), pick(d["leye_pose"]), pick(d["reye_pose"]), pick(d["left_hand_pose"]),
                      pick(d["right_hand_pose"]), pick(d["transl"]), R, Th)


# ---- the reference's own output ---------------------------------------------------------------------------------------------
def test_golden_bodies(dev, golden):
    g = golden
    for name in ("b1", "b2", "b3"):
        flat = bool(g[f"{name}_flat_hand_mean"])
        _, _, model = models(int(g["V"]), int(g["seed"]), 400, flat, dev)
        d = {k: torch.from_numpy(g[f"{name}_{k}"]) for k in PART_NAMES + ["betas", "expression", "transl"]}
        posed = pose(model, d, dev)
        got = frame(posed, 0)
        assert np.array_equal(posed.poses[0].cpu().numpy(), g[f"{name}_full_pose"]) and np.array_equal(posed.shapes.cpu().numpy(), g[f"{name}_shapes"])
        for k in ("vertices", "joints"):
            e, bound = float(np.abs(got[k].astype(np.float64) - g[f"{name}_{k}"]).max()), FACTOR * float(g[f"{name}_err_{k}"])
            print(f"{name} {k}: kernel {e:.3e}, the reference in fp32 {float(g[f'{name}_err_{k}']):.3e}")
            assert e <= bound, (name, k, e, bound)
        wb = posed.world_bounds[0].cpu().numpy()
        assert np.array_equal(wb, sr.bounds(got["vertices"]))                       # the reference arithmetic on the kernel's own vertices
        eb = float(np.abs(wb.astype(np.float64) - g[f"{name}_bounds"]).max())
        print(f"{name} bounds: {eb:.3e}")
        assert eb <= FACTOR * float(g[f"{name}_err_vertices"]) + 1e-7
        assert torch.all(posed.verts4[..., 3] == 0) and torch.isfinite(posed.table).all()
    big = model.big_pose()                                                          # body 3 is the recon twin's big pose
    assert torch.equal(big.t_vertices, posed.vertices[0]) and torch.equal(big.t_world_bounds, posed.world_bounds[0])
    assert model.big_pose() is big and model.big_pose((-3.1416, 0.0, 0.0)) is not big
    assert not torch.equal(model.big_pose((-3.1416, 0.0, 0.0)).t_vertices, big.t_vertices)


# ---- shapes where indexing can go wrong -------------------------------------------------------------------------------------
def _chunk():
    from humanliff_amd import _lib
    return int(_lib.lib().hl_smplx_chunk_frames())


@pytest.mark.parametrize("cols", [400, 20])
@pytest.mark.parametrize("V", [257, 300])
@pytest.mark.parametrize("F", ["1", "3", "chunk", "chunk+1"])
def test_small_shapes(dev, V, F, cols):
    F = {"1": 1, "3": 3, "chunk": _chunk(), "chunk+1": _chunk() + 1}[F]
    flat = V == 257                                                             # V = 300: the hand means are added
    cpu, m64, model = models(V, 3, cols, flat, dev)
    assert float((cpu["weights"] == 0).float().mean()) > 0.5 and model.two_sets == (cols == 400)
    c = sr.columns(cols)
    mean = sr.pose_mean(m64, flat).astype(np.float32)
    shared = F == 3                                                             # F = 3: betas, R and Th shared across the frames
    d = random_inputs(F, 1000 * V + 10 * F + (cols == 20), shared)
    for k in PART_NAMES + ["expression", "transl"]:
        d[k][F // 2] = 0.0                                                      # an all-zero frame
    if not shared:
        d["betas"][F // 2] = 0.0
    g = syn._gen(77 + F)
    n_rt = 1 if shared else F
    Rs = torch.stack([syn._rodrigues1(torch.randn(3, generator=g) * 0.4) for _ in range(n_rt)]).numpy()
    Ths = (torch.randn((n_rt, 3), generator=g) * 0.2).numpy()
    rt = lambda f: (Rs[f if n_rt > 1 else 0], Ths[f if n_rt > 1 else 0])  # noqa: E731
    posed = pose(model, d, dev, Rs if n_rt > 1 else Rs[0], Ths if n_rt > 1 else Ths[0])
    assert torch.isfinite(posed.vertices).all() and torch.isfinite(posed.table).all() and torch.isfinite(posed.joints).all()
    for f in range(F):
        want = truth(m64, c, mean, d, f, *rt(f))
        ek, ey = errors(frame(posed, f), want), errors(torch_path(cpu, c, mean, d, f, *rt(f)), want)
        for k in ek:
            print(f"V {V} F {F} cols {cols} frame {f} {k}: kernel {ek[k]:.3e}, fp32 torch path {ey[k]:.3e}")
        for k in ek:
            assert ek[k] <= FACTOR * ey[k], (f, k, ek[k], ey[k])
    fields = ("vertices", "joints", "world_bounds", "verts4", "table")
    again = pose(model, d, dev, Rs if n_rt > 1 else Rs[0], Ths if n_rt > 1 else Ths[0])
    for k in fields:
        assert torch.equal(getattr(posed, k), getattr(again, k)), f"{k}: two runs differ"
    for f in range(F):                                                          # a batch is its frames posed one by one, bit for bit
        one = pose(model, d, dev, *rt(f), f=f)
        for k in fields:
            assert torch.equal(getattr(posed, k)[f], getattr(one, k)[0]), f"{k}: frame {f} of the batch differs from the frame alone"


# ---- the two entry points are one set of kernels ------------------------------------------------------------------------------
class _BigRows:
    """What _pose reads of a big-pose body: rows (1,V,16)."""

    def __init__(self, rows):
        self.rows = rows


@pytest.mark.parametrize("V", [257, 300])
@pytest.mark.parametrize("F", ["1", "chunk+1"])
def test_smpl_and_smplx_entry_points_agree(dev, V, F):
    """A 55-joint model with one direction set, a zero pose mean and no transl is the same rule through hl_pose_body_margins (the
    X = false kernels) and hl_smplx_pose (X = true: t from the set-2 blend, which then copies A's last column): every output and both
    workspace arrays are equal bit for bit, with big-pose rows written (big=None) and read (the table)."""
    from humanliff_amd.body import load_body_model, load_smplx_model
    F = 1 if F == "1" else _chunk() + 1
    cpu = models(V, 3, 20, True, dev)[0]
    smpl = load_body_model({k: cpu[k] for k in cpu if not k.startswith("hands_")}, dev)
    smplx = load_smplx_model(cpu, dev, num_betas=10, num_expression_coeffs=6)
    assert (smpl.J, smpl.Sp) == (55, 16) and (smplx.S, smplx.expr_start, smplx.two_sets) == (16, 10, 0) and not smplx.pose_mean.any()
    g = syn._gen(4000 + 10 * V + F)
    full = torch.randn((F, 165), generator=g) * 0.25
    coef = torch.randn((F, 16), generator=g) * 0.5
    if F > 1:
        full[F // 2] = 0.0                                                      # an all-zero pose
    Rs = torch.stack([syn._rodrigues1(torch.randn(3, generator=g) * 0.4) for _ in range(F)]).numpy()
    Ths = (torch.randn((F, 3), generator=g) * 0.2).numpy()
    parts, at = {}, 0
    for k, n in sr.PARTS:
        parts[k] = full[:, at:at + 3 * n].to(dev)
        at += 3 * n
    rows = _BigRows(torch.randn((1, V, 16), generator=g).to(dev))
    for big in (None, rows):
        a = smpl._pose(full.to(dev), coef.to(dev), Rs, Ths, big=big, y_margin=0.1)
        b = smplx._pose(parts, coef[:, :10].to(dev), coef[:, 10:].to(dev), None, Rs, Ths, big=big, y_margin=0.1)
        assert torch.equal(a.poses, b.poses) and torch.equal(a.shapes, b.shapes)
        for k in ("vertices", "joints", "world_bounds", "verts4", "table", "rows", "A", "pose_features"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None) == (k == ("table" if big is None else "rows")), k
            if x is not None:
                assert torch.isfinite(x).all() and torch.equal(x, y), f"{k} (big {'given' if big else 'None'}): the two entry points differ"


# ---- the table: the renderer's rule, its two direction sets included ----------------------------------------------------------
def _b1(golden, dev, V, flat=True):
    cpu, m64, model = models(V, 3, 400, flat, dev)
    d = {k: torch.from_numpy(golden[f"b1_{k}"]) for k in PART_NAMES + ["betas", "expression", "transl"]}       # pose scale 0.25
    return cpu, m64, model, d, pose(model, d, dev)


def test_table_against_todays_deform_tables(dev, golden):
    from humanliff_amd.NeRF import deform
    cpu, m64, model, d, posed = _b1(golden, dev, 1200)
    tp = posed.tp_input(0)
    assert tuple(tp["params"]["poses"].shape) == (1, 165) and tuple(tp["params"]["shapes"].shape) == (1, 20)
    deform._TABLE_CACHE.clear()
    verts4_t, table_t, Rh, Th = deform.deform_tables(model.tensors, tp["params"], tp["t_params"], tp["vertices"])
    assert np.array_equal(Rh, np.eye(3, dtype=np.float32)) and np.array_equal(Th, np.zeros(3, dtype=np.float32))
    mean = sr.pose_mean(m64, True)
    poses = sr.full_pose({k: d[k][0].numpy() for k in PART_NAMES}, mean)
    coef = np.concatenate([d["betas"][0].numpy(), d["expression"][0].numpy()]).astype(np.float64)
    big = sr.full_pose({"body_pose": model.big_pose_params()["body_pose"][0]}, mean)
    want, At = sr.table(m64, syn.SMPLX_PARENTS, poses, coef, big)
    set1 = np.concatenate([m64["shapedirs"][..., :10], m64["shapedirs"][..., 300:310]], axis=-1) @ coef
    assert np.abs(set1 - want[:, 15:18]).max() > 1e-3                           # the two direction sets really differ here
    got, yard = posed.table[0].cpu().numpy().astype(np.float64), table_t.cpu().numpy().astype(np.float64)
    for name, sl in (("t", slice(0, 3)), ("pose_off", slice(12, 15)), ("shape_off", slice(15, 18)), ("pose_off_big", slice(18, 21)),
                     ("Rbig", slice(21, 30)), ("tbig", slice(30, 33)), ("pad", slice(33, 36))):
        ek, ey = np.abs(got[:, sl] - want[:, sl]).max(), np.abs(yard[:, sl] - want[:, sl]).max()
        print(f"table {name}: kernel {ek:.3e}, deform_tables {ey:.3e}")
        assert ek <= FACTOR * ey, (name, ek, ey)
    # The blended matrices must be well conditioned for an inverse's residual to say anything: it grows like cond x 2^-24.  The random
    # top-4 weights blend unrelated joints, and the finger chains are nine joints deep, so the worst vertex here is at 4.4, not below 3
    # as on the 24-joint tree.
    assert np.linalg.cond(At).max() < 10.0
    eye = np.eye(3)[None]
    rk = np.abs(got[:, 3:12].reshape(-1, 3, 3) @ At - eye).max()
    ry = np.abs(yard[:, 3:12].reshape(-1, 3, 3) @ At - eye).max()
    print(f"table Rinv residual: kernel {rk:.3e}, torch.inverse {ry:.3e}")
    assert rk <= FACTOR * ry
    assert torch.equal(posed.verts4[0, :, :3], posed.vertices[0]) and torch.equal(posed.verts4[0], verts4_t)     # R = I, Th = 0: the world vertices, w = 0


# ---- the renderer's hook ----------------------------------------------------------------------------------------------------
def _view(dev, golden, H=32, W=32, N=16):
    cpu, m64, model, d, posed = _b1(golden, dev, 1500)
    tp = posed.tp_input(0)
    vertices = posed.vertices[0].cpu()
    lo, hi = vertices.min(0).values - 0.1, vertices.max(0).values + 0.1
    ro, rd, _, _ = syn.orbit_rays(4, 36, H, W)
    ro = ro + vertices.mean(0)
    nr, fr = syn.near_far_from_bounds(torch.stack([lo, hi]).double().numpy(), ro.double().numpy(), rd.double().numpy())
    nr, fr = torch.from_numpy(nr).float(), torch.from_numpy(fr).float()
    u = torch.rand((H * W, N), generator=torch.Generator().manual_seed(9))
    tp["world_bounds"] = torch.stack([lo, hi])[None].to(dev)
    rays = (ro[None].to(dev), rd[None].to(dev), nr[None].to(dev), fr[None].to(dev))
    return model, tp, rays, u.to(dev), N


def _renderer(dev, model):
    from humanliff_amd.NeRF import Renderer
    r = Renderer(use_canonical_space=True, triplane_dim=64, triplane_ch=27, smpl_type='smplx', test=True)
    r.load_state_dict(syn.render_mlp_state(3), strict=False)
    r = r.to(dev)
    assert r.load_body_model(model) is model and r.SMPL_NEUTRAL is model.tensors and r.faces is model.tensors["f"]
    return r


def _render(r, tp, rays, u, N, planes):
    out = r.render(tp, None, None, *rays, planes, N, False, n_samples=N, u=u)
    return [out[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")]


def test_hooked_render_equals_the_renderers_own_tables(dev, golden, monkeypatch):
    """The bounds are tests/test_render_gpu.py's for a canonical-space render against its oracle (2e-5 colour and opacity, 5e-5 depth):
    both renders find the same nearest vertices (verts4 is bit-equal), the table rows differ by rounding."""
    from humanliff_amd.NeRF import deform
    model, tp, rays, u, N = _view(dev, golden)
    r = _renderer(dev, model)
    planes = syn.triplane(seed=11, H=64, W=64).to(dev)
    plain = _render(r, {k: v for k, v in tp.items() if k != "deform"}, rays, u, N, planes)
    assert float(plain[1].max()) > 0.05                                         # the body is hit
    hooked = _render(r, tp, rays, u, N, planes)
    for name, a, b, bound in zip(("rgb", "acc", "depth"), plain, hooked, (2e-5, 2e-5, 5e-5)):
        e = float((a - b).abs().max())
        print(f"hooked render vs the renderer's own tables, {name}: {e:.3e}")
        assert e <= bound, (name, e)

    def refuse(*a, **k):
        raise AssertionError("deform_tables was called although tp_input['deform'] is there")
    monkeypatch.setattr(deform, "deform_tables", refuse)
    again = _render(r, tp, rays, u, N, planes)
    for a, b in zip(hooked, again):
        assert torch.equal(a, b)
    with pytest.raises(AssertionError, match="deform_tables was called"):
        _render(r, {k: v for k, v in tp.items() if k != "deform"}, rays, u, N, planes)


# ---- the dataset ------------------------------------------------------------------------------------------------------------
def smplx_file_content(n_poses, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s, scale=0.2: (rng.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    return {"betas": f(1, 10, scale=0.5), "global_orient": f(n_poses, 3, scale=0.1), "body_pose": f(n_poses, 63), "jaw_pose": f(n_poses, 3),
            "leye_pose": f(n_poses, 3), "reye_pose": f(n_poses, 3), "left_hand_pose": f(n_poses, 45), "right_hand_pose": f(n_poses, 45),
            "expression": f(n_poses, 10, scale=0.5), "transl": f(n_poses, 3, scale=0.02)}


def test_synbody_tree_with_smplx(dev, tmp_path):
    from humanliff_amd.body import load_body_model, load_smplx_model
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import SynBodyIndex, load_view_store, smplx_params
    data_root, _ = fx.write_tree(tmp_path, n_subjects=2, layers=(0,), poses=(0, 1), n_views=2, size=16, png_images=(), radius=3.0)
    genders = ("female", "male")
    for s, gender in enumerate(genders):
        np.savez(os.path.join(str(tmp_path), f"human_{s:02d}", "smplx.npz"), smplx=np.array(smplx_file_content(2, 60 + s), dtype=object),
                 meta=np.array({"gender": gender}, dtype=object))
    index = SynBodyIndex(data_root, multi_person=True, num_instance=2, pose_start=1, pose_interval=1, poses_num=1, views_num=2, layer_idx=0)
    assert len(index) == 4 and index.smplx_path(1) == os.path.join(str(tmp_path), "human_01", "smplx.npz")
    bodies = {g: load_smplx_model(syn.smplx_like_model(256, 30 + i, 400), dev) for i, g in enumerate(genders)}
    store = load_view_store(index, bodies, image_scaling=1.0, device=dev, smpl_type="smplx")
    assert len(store) == 4 and store.instance_idx.tolist() == [0, 0, 1, 1] and store.pose_index.tolist() == [1] * 4
    for s, gender in enumerate(genders):
        params, got_gender = smplx_params(index.smplx_path(s), 1)
        assert got_gender == gender
        want = bodies[gender].pose_dict(params).world_bounds[0].cpu().numpy()
        for v in (2 * s, 2 * s + 1):
            assert np.array_equal(store.bounds[v], want.astype(store.bounds.dtype)), (s, v)
    assert not np.array_equal(store.bounds[0], store.bounds[2])
    with pytest.raises(KeyError, match="male"):
        load_view_store(index, {"female": bodies["female"]}, image_scaling=1.0, device=dev, smpl_type="smplx")
    # the 'smpl' call on the same tree is what it was: the bounds of BodyModel.pose of smpl_params
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import smpl_params
    smpl = load_body_model(syn.smpl_like_model(n_vertices=256), dev)
    plain = load_view_store(index, smpl, image_scaling=1.0, device=dev)
    p = smpl_params(index.smpl_path(0), 1)
    want = smpl.pose(torch.from_numpy(p["poses"]).to(dev), torch.from_numpy(p["shapes"].reshape(-1)).to(dev), p["R"], p["Th"]).world_bounds[0]
    assert np.array_equal(plain.bounds[0], want.double().cpu().numpy())
    assert torch.equal(plain.images, store.images) and torch.equal(plain.body, store.body)


def test_prepare_input_of_the_sampling_twin(dev):
    """SynBodyView_datasets.py:141-182 with smpl_type 'smplx': the model is run with a zero transl, the translation travels in 'Th', and
    'poses' / 'shapes' are added to params; the big pose behind the tables is that twin's (global_orient [-3.1416, 0, 0])."""
    from humanliff_amd.SynBodyView_datasets import BIG_GLOBAL_ORIENT, prepare_input
    _, _, model = models(257, 3, 400, True, dev)
    fitted = smplx_file_content(2, 71)
    params = {k: torch.from_numpy(v if k == "betas" else v[1:2]) for k, v in fitted.items()}          # host tensors, as prepare_smpl_params makes them
    params["R"], params["Th"] = np.eye(3, dtype=np.float32), fitted["transl"][0:1]
    wb, vertices, same, joints = prepare_input(model, params)
    assert same is params and tuple(wb.shape) == (2, 3) and tuple(vertices.shape) == (257, 3) and tuple(joints.shape) == (55, 3)
    assert tuple(params["poses"].shape) == (1, 165) and tuple(params["shapes"].shape) == (1, 20)
    d = {k: torch.from_numpy(v if k == "betas" else v[1:2]).to(dev) for k, v in fitted.items() if k != "transl"}
    want = model.pose_dict(d, Th=fitted["transl"][0:1], big_global_orient=BIG_GLOBAL_ORIENT)
    assert torch.equal(vertices, want.vertices[0]) and torch.equal(joints, want.joints[0]) and torch.equal(wb, want.world_bounds[0])
    moved = model.pose_dict(dict(d, transl=torch.from_numpy(fitted["transl"][0:1]).to(dev)))           # the recon twin's way: transl into the model
    assert float((moved.vertices[0] - vertices).abs().max()) < 1e-6
