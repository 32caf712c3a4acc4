"""Binding a mesh to a posed body and reposing it: the float64 restatement's own identities (tests/mesh_animate_restatement.py) and the
host-side argument checks of humanliff_amd/NeRF/animate.py that need no device.  DESIGN.md "Animating the mesh"."""
import inspect
import types

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import body_restatement as br
from tests import mesh_animate_restatement as ma


@pytest.fixture(scope="module")
def scene():
    """A 257-vertex body in two poses (float64 restatement) and 300 mesh points near the first one, with unit normals."""
    V = 257
    m64 = br.model64(syn.smpl_like_model(V, 3))
    g = syn._gen(5)
    poses = (torch.randn((2, 72), generator=g) * 0.25).numpy()
    shapes = (torch.randn((10,), generator=g) * 0.5).numpy()
    R = br.rodrigues([0.3, -0.2, 0.5])              # (orthonormal to float64: the round trip takes R^T for the inverse of R)
    Th = np.array([0.1, -0.7, 0.4])
    frames = [br.pose(m64, syn.SMPL_PARENTS, poses[f], shapes, R, Th) for f in range(2)]
    rng = np.random.default_rng(7)
    x = frames[0]["vertices"][rng.integers(0, V, 300)] + rng.normal(0.0, 0.02, (300, 3))
    n = rng.normal(size=(300, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[17] = 0.0
    return {"frames": frames, "rows": [ma.rows_from_pose(t) for t in frames], "R": R, "Th": Th, "x": x, "n": n}


@pytest.mark.parametrize("K", [1, 4, 8])
def test_float64_round_trip(scene, K):
    s = scene
    b = ma.bind(s["x"], s["n"], s["frames"][0]["v_smpl"], s["rows"][0], s["R"], s["Th"], K)
    assert np.abs(b["weights"].sum(axis=1) - 1.0).max() < 1e-15 and (np.diff(b["d_sorted"], axis=1) >= 0).all()
    world, normals = ma.repose(b["ids"], b["weights"], b["rest"], b["rest_normals"], s["rows"][0], s["R"], s["Th"])
    e, en = np.abs(world - s["x"]).max(), np.abs(normals - s["n"]).max()
    print(f"K {K}: bind then repose to the bind frame, float64: vertices {e:.3e}, normals {en:.3e}")
    assert e < 1e-12 and en < 1e-12
    assert (normals[17] == 0).all() and (b["rest_normals"][17] == 0).all()
    moved, _ = ma.repose(b["ids"], b["weights"], b["rest"], b["rest_normals"], s["rows"][1], s["R"], s["Th"])
    assert 1e-3 < np.abs(moved - s["x"]).max() < 1.0                         # the other pose is another pose
    tr = np.array([0.3, -0.1, 0.2])
    shifted, _ = ma.repose(b["ids"], b["weights"], b["rest"], None, s["rows"][0], s["R"], s["Th"], transl=tr)
    assert np.abs(shifted - (s["x"] + tr @ s["R"].T)).max() < 1e-12          # transl is added before the world transform


def test_one_neighbour_is_the_renderers_rule(scene):
    s = scene
    t = s["frames"][0]
    b = ma.bind(s["x"], None, t["v_smpl"], s["rows"][0], s["R"], s["Th"], 1)
    assert (b["weights"] == 1.0).all() and b["rest_normals"] is None
    j = b["ids"][:, 0]
    q = (s["x"] - s["Th"]) @ s["R"]
    assert np.array_equal(j, np.argmin(((q[:, None] - t["v_smpl"][None]) ** 2).sum(-1), axis=1))
    want = np.einsum("nrc,nc->nr", np.linalg.inv(t["T"][j, :3, :3]), q - t["T"][j, :3, 3]) - t["pose_off"][j]
    assert np.abs(b["rest"] - want).max() < 1e-12


def test_float32_restatement_is_float32_and_close(scene):
    s = scene
    b64 = ma.bind(s["x"], s["n"], s["frames"][0]["v_smpl"], s["rows"][0], s["R"], s["Th"], 4)
    b32 = ma.bind(s["x"], s["n"], s["frames"][0]["v_smpl"], s["rows"][0], s["R"], s["Th"], 4, dtype=np.float32)
    assert all(b32[k].dtype == np.float32 for k in ("weights", "rest", "rest_normals", "q"))
    same = (b32["ids"] == b64["ids"]).all(axis=1)
    assert same.mean() > 0.99
    e = np.abs(b32["rest"][same] - b64["rest"][same]).max()
    assert 0 < e < 1e-5
    world, normals = ma.repose(b32["ids"], b32["weights"], b32["rest"], b32["rest_normals"], s["rows"][1], s["R"], s["Th"], dtype=np.float32)
    assert world.dtype == np.float32 and normals.dtype == np.float32


# ---- the host side ------------------------------------------------------------------------------------------------------------
def _fake_posed(V=12, F=3, rows=True):
    model = types.SimpleNamespace(V=V)
    return types.SimpleNamespace(model=model, F=F, big=None, rows=torch.zeros((F, V, 16)) if rows else None, verts4=torch.zeros((F, V, 4)),
                                 rt=torch.zeros((1, 12)))


def test_bind_mesh_argument_errors():
    from humanliff_amd.NeRF import animate
    pts = np.zeros((5, 3))
    with pytest.raises(ValueError, match="forward_rows=True"):
        animate.bind_mesh(pts, _fake_posed(rows=False))
    for k in (0, 9, 13):
        with pytest.raises(ValueError, match="neighbours"):
            animate.bind_mesh(pts, _fake_posed(), neighbours=k)
    with pytest.raises(ValueError, match="neighbours"):
        animate.bind_mesh(pts, _fake_posed(V=3), neighbours=4)
    with pytest.raises(ValueError, match="frame"):
        animate.bind_mesh(pts, _fake_posed(), frame=3)
    with pytest.raises(RuntimeError, match="no CPU path"):                     # a posed body on the host
        animate.bind_mesh(pts, _fake_posed())


def test_repose_argument_errors():
    from humanliff_amd.NeRF import animate
    b = animate.MeshBinding()
    posed = _fake_posed()
    b.model, b.N, b.K, b.rest_normals = posed.model, 5, 4, None
    with pytest.raises(ValueError, match="forward_rows=True"):
        b.repose(_fake_posed(rows=False))
    with pytest.raises(ValueError, match="another body model"):
        b.repose(_fake_posed())
    with pytest.raises(ValueError, match="step 1"):
        b.repose(posed, frames=slice(0, 3, 2))
    with pytest.raises(ValueError, match="frame"):
        b.repose(posed, frames=3)
    with pytest.raises(ValueError, match="no frame"):
        b.repose(posed, frames=slice(2, 2))
    with pytest.raises(ValueError, match="margins"):
        b.repose(posed, margin=-0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        b.repose(posed)


def test_the_interface_is_there():
    from humanliff_amd import _lib, body
    from humanliff_amd.NeRF import Renderer
    from humanliff_amd.recon_NeRF import Renderer as ReconRenderer
    for fn in (body.BodyModel.pose, body.SmplxModel.pose, body.SmplxModel.pose_dict):
        assert inspect.signature(fn).parameters["forward_rows"].default is False
    for name in ("hl_mesh_bind", "hl_mesh_repose", "hl_mesh_repose_scratch_bytes"):
        assert name in _lib.SIGNATURES
    for r in (Renderer, ReconRenderer):
        assert list(inspect.signature(r.bind_mesh).parameters) == ["self", "mesh", "posed", "frame", "neighbours"]
