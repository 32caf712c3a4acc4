"""What can be said about posing an SMPL-X body without a GPU: the float64 restatement against the vectors the reference produced, the
loader's column selection, mean pose, parents and refusals, the dataset's parameter reader, the C ABI, and what stays unimplemented."""
import os
import re

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import smplx_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "smplx.npz")
EXPORTS = ("hl_smplx_packed_bytes", "hl_smplx_pack", "hl_smplx_chunk_frames", "hl_smplx_pose_workspace_bytes", "hl_smplx_pose")
PART_NAMES = [k for k, _ in sr.PARTS]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_matches_the_reference(golden):
    g = golden
    assert os.path.getsize(GOLDEN) < 1 << 20
    model = syn.smplx_like_model(int(g["V"]), int(g["seed"]), 400)
    assert model["kintree_table"][0].tolist() == syn.SMPLX_PARENTS and all(v.dtype == torch.float32 for k, v in model.items()
                                                                         if k not in ("kintree_table", "f"))
    m = sr.model64(model)
    cols = sr.columns(400)
    assert cols == (10, 300, 10)
    for name in ("b1", "b2", "b3"):
        mean = sr.pose_mean(m, bool(g[f"{name}_flat_hand_mean"]))
        # (the reference adds pose_mean in the dtype it runs in: float64 here, from the float32 inputs)
        poses = sr.full_pose({k: g[f"{name}_{k}"] for k in PART_NAMES}, mean)
        assert np.abs(poses - g[f"{name}_full_pose"]).max() < 1e-7
        coef = np.concatenate([g[f"{name}_betas"], g[f"{name}_expression"]], axis=-1)
        assert np.array_equal(coef.astype(np.float32), g[f"{name}_shapes"])
        got = sr.pose(m, syn.SMPLX_PARENTS, poses, coef, cols, g[f"{name}_transl"])
        ev, ej = np.abs(got["vertices"] - g[f"{name}_vertices"]).max(), np.abs(got["joints"] - g[f"{name}_joints"]).max()
        print(f"{name}: vertices {ev:.3e}, joints {ej:.3e}; the reference in fp32: {float(g[f'{name}_err_vertices']):.3e}, "
              f"{float(g[f'{name}_err_joints']):.3e}")
        assert ev <= 1e-12 and ej <= 1e-12, name
        assert 5e-8 < float(g[f"{name}_err_vertices"]) < 1e-6 and 5e-8 < float(g[f"{name}_err_joints"]) < 1e-6
        eb = np.abs(sr.bounds(got["vertices"].astype(np.float32)) - g[f"{name}_bounds"]).max()
        assert eb <= float(g[f"{name}_err_vertices"]) + 2.4e-7, (name, eb)          # the fp32 run's vertices, then fp32 sums of values below 2
    zb, zf = int(g["zero_body_joint"]), int(g["zero_finger_joint"])
    assert np.all(g["b1_body_pose"][0, 3 * zb:3 * zb + 3] == 0) and np.all(g["b1_left_hand_pose"][0, 3 * zf:3 * zf + 3] == 0)
    assert np.abs(g["b1_body_pose"]).max() > 0.3 and np.abs(g["b1_transl"]).min() > 0
    assert np.array_equal(g["b1_full_pose"][:75], g["b2_full_pose"][:75]) and np.abs(g["b1_full_pose"][75:] - g["b2_full_pose"][75:]).min() > 0
    assert np.count_nonzero(g["b3_body_pose"]) == 4 and np.count_nonzero(g["b3_full_pose"]) == 4


def test_loader_columns_mean_pose_parents_and_refusals(tmp_path):
    from humanliff_amd.body import SmplxModel, load_smplx_model
    for cols, want in ((400, (10, 300, 10, 1)), (20, (10, 10, 10, 0))):
        model = syn.smplx_like_model(300, 4, cols)
        got = load_smplx_model(dict(model), "cpu")
        assert isinstance(got, SmplxModel) and (got.V, got.J, got.S) == (300, 55, 20) and got.parents == syn.SMPLX_PARENTS
        assert (got.num_betas, got.expr_start, got.num_expr, got.two_sets) == want
        assert set(got.tensors) == {"v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights", "f"}
        assert torch.equal(got.tensors["shapedirs"], model["shapedirs"]) and got.tensors["kintree_table"].dtype == torch.long
        assert tuple(got.pose_mean.shape) == (165,) and not got.pose_mean.any()                       # flat_hand_mean=True
    few = load_smplx_model(dict(model), "cpu", num_betas=16, num_expression_coeffs=50)
    assert (few.num_betas, few.expr_start, few.num_expr) == (10, 10, 10)                              # a 20-column file: both cut to 10
    big = syn.smplx_like_model(300, 4, 400)
    more = load_smplx_model(dict(big), "cpu", num_betas=12, num_expression_coeffs=20)
    assert (more.num_betas, more.expr_start, more.num_expr, more.S) == (12, 300, 20, 32)
    with pytest.raises(ValueError, match="coefficients"):
        load_smplx_model(dict(big), "cpu", num_betas=20, num_expression_coeffs=20)
    hands = load_smplx_model(dict(big), "cpu", flat_hand_mean=False)
    assert not hands.pose_mean[:75].any() and torch.equal(hands.pose_mean[75:120], big["hands_meanl"]) and \
        torch.equal(hands.pose_mean[120:], big["hands_meanr"]) and bool(big["hands_meanl"].all())
    # a directory resolves to SMPLX_{GENDER}.npz; the root's parent may be 2^32 - 1 as in the official files
    kt = big["kintree_table"].numpy().astype(np.uint32)
    kt[0, 0] = 4294967295
    np.savez(tmp_path / "SMPLX_FEMALE.npz", **{k: v.numpy() for k, v in big.items() if k != "kintree_table"}, kintree_table=kt)
    from_dir = load_smplx_model(str(tmp_path), "cpu", gender="female")
    assert from_dir.parents == syn.SMPLX_PARENTS and torch.equal(from_dir.tensors["posedirs"], big["posedirs"])
    with pytest.raises(FileNotFoundError):
        load_smplx_model(str(tmp_path), "cpu", gender="male")
    with pytest.raises(NotImplementedError, match="use_pca"):
        load_smplx_model(dict(big), "cpu", use_pca=True)
    bad = dict(big)
    bad["kintree_table"] = big["kintree_table"].clone()
    bad["kintree_table"][0, 3] = 7                         # joint 3 hangs on joint 7
    with pytest.raises(ValueError, match="joint 3"):
        load_smplx_model(bad, "cpu")
    for key in ("hands_meanl", "posedirs"):
        with pytest.raises(KeyError, match=key):
            load_smplx_model({k: v for k, v in big.items() if k != key}, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        hands.pose(torch.zeros(1, 3), torch.zeros(1, 63), torch.zeros(10), torch.zeros(1, 10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        hands.big_pose()


def test_big_pose_params_of_the_two_twins():
    from humanliff_amd.body import load_smplx_model
    model = load_smplx_model(syn.smplx_like_model(300, 4, 20), "cpu")
    recon, view = model.big_pose_params(), model.big_pose_params((-3.1416, 0.0, 0.0))
    assert set(recon) == {"R", "Th", "global_orient", "betas", "body_pose", "jaw_pose", "left_hand_pose", "right_hand_pose", "leye_pose",
                          "reye_pose", "expression", "transl"}
    assert all(v.dtype == np.float32 for v in recon.values()) and not recon["global_orient"].any()
    assert np.array_equal(view["global_orient"], np.array([[-3.1416, 0, 0]], dtype=np.float32))
    for p in (recon, view):
        bp = p["body_pose"]
        assert bp.shape == (1, 63) and np.count_nonzero(bp) == 4
        assert bp[0, 2] == np.float32(np.pi / 4) and bp[0, 5] == -np.float32(np.pi / 4) and bp[0, 20] == -np.float32(np.pi / 6) and \
            bp[0, 23] == np.float32(np.pi / 6)


def test_smplx_params_follow_the_reference_rule(tmp_path):
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import smplx_params
    rng = np.random.default_rng(5)
    fitted = {"betas": rng.standard_normal((1, 10)).astype(np.float32), "expression": rng.standard_normal((3, 10)).astype(np.float32),
              "transl": rng.standard_normal((3, 3)).astype(np.float32)}
    fitted.update({k: rng.standard_normal((3, 3 * n)).astype(np.float32) for k, n in sr.PARTS})
    path = str(tmp_path / "smplx.npz")
    np.savez(path, smplx=np.array(fitted, dtype=object), meta=np.array({"gender": "female"}, dtype=object))
    params, gender = smplx_params(path, 2)
    assert gender == "female" and set(params) == set(fitted) | {"R", "Th"}
    # prepare_smpl_params, smplx branch (SynBody_dataset.py:145-155), restated: betas whole, every other key [i:i+1], R = I, Th = 0
    for k, v in fitted.items():
        want = v if k == "betas" else v[2:3]
        assert torch.is_tensor(params[k]) and params[k].dtype == torch.float32 and np.array_equal(params[k].numpy(), want), k
    assert tuple(params["betas"].shape) == (1, 10) and tuple(params["body_pose"].shape) == (1, 63)
    assert np.array_equal(params["R"], np.eye(3, dtype=np.float32)) and params["R"].dtype == np.float32
    assert np.array_equal(params["Th"], np.zeros((1, 3), dtype=np.float32)) and params["Th"].dtype == np.float32
    assert not np.array_equal(smplx_params(path, 0)[0]["transl"].numpy(), params["transl"].numpy())


def test_header_declares_the_exports():
    from humanliff_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_smplx_")) == sorted(EXPORTS)
    V, J, S, P = 10475, 55, 20, 486
    one = (P + S) * 3 * V + J * V + 3 * V + 3 * J + 3 * J * S
    assert L.hl_smplx_packed_bytes(V, J, S, 0) == 4 * one and L.hl_smplx_packed_bytes(V, J, S, 1) == 4 * (one + S * 3 * V + 3 * J * S)
    assert L.hl_smplx_packed_bytes(V, 64, 32, 1) > 0
    for bad in ((V, 65, S), (V, 1, S), (V, J, 33), (V, J, 0), (0, J, S)):
        assert L.hl_smplx_packed_bytes(*bad, 1) == 0, bad
    assert L.hl_smplx_pose_workspace_bytes(J, 3) == 4 * 3 * (J * 20 + P)
    assert L.hl_smplx_pose_workspace_bytes(J, 0) == 0 and L.hl_smplx_pose_workspace_bytes(65, 1) == 0 and L.hl_smplx_pose_workspace_bytes(1, 1) == 0
    assert L.hl_smplx_chunk_frames() >= 2
    # the staged frames of a chunk fit the default 64 KB of LDS at the limits
    assert 4 * L.hl_smplx_chunk_frames() * (15 * 64 + 9 * 63 + 32 + 16) <= 64 * 1024
    none = [None] * 8
    assert L.hl_smplx_pose(None, None, V, J, S, 1, 1, None, None, None, None, 0, *none, 0, 0.05, 0.05, None) < 0
    assert b"hl_smplx_pose" in L.hl_last_error()
    assert L.hl_smplx_pack(None, None, 400, 10, 300, 10, None, None, None, V, J, None, None) < 0 and b"hl_smplx_pack" in L.hl_last_error()


def test_what_stays_unimplemented():
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import smpl_params
    from humanliff_amd.recon_NeRF.lib.TightCap_dataset import TightCapIndex
    with pytest.raises(NotImplementedError):
        smpl_params("nowhere.npz", 0, smpl_type="smplx")
    with pytest.raises(NotImplementedError):
        TightCapIndex("nowhere", smpl_type="smplx")
