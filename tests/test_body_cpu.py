"""What can be said about posing the body model without a GPU: the float64 restatement against the vectors the reference produced, the
loader on every kind of source it accepts and on the errors it names, the big pose, the C ABI, and the refusal of CPU tensors."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from humanliff_amd import synthetic as syn
from tests import body_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "body.npz")
EXPORTS = ("hl_body_packed_bytes", "hl_body_pack", "hl_body_chunk_frames", "hl_body_pose_workspace_bytes", "hl_body_pose")
ULP = 2.4e-7      # one float32 ulp at magnitude [1, 2): both sides are float64 results rounded to float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_matches_the_reference(golden):
    g = golden
    model = syn.smpl_like_model(int(g["V"]), int(g["seed"]))
    m = br.model64(model)
    for name in ("b1", "b2"):
        got = br.pose(m, syn.SMPL_PARENTS, g[f"{name}_poses"], g[f"{name}_shapes"], g[f"{name}_R"], g[f"{name}_Th"], rot_dtype=np.float32)
        ev = np.abs(got["vertices"].astype(np.float32) - g[f"{name}_vertices"]).max()
        ej = np.abs(got["joints"].astype(np.float32) - g[f"{name}_joints"]).max()
        eb = np.abs(br.bounds(got["vertices"].astype(np.float32)) - g[f"{name}_bounds"]).max()
        print(f"{name}: vertices {ev:.3e}, joints {ej:.3e}, bounds {eb:.3e}")
        assert max(np.abs(g[f"{name}_vertices"]).max(), np.abs(g[f"{name}_joints"]).max()) < 2.0      # (the magnitude the bound is stated for)
        assert ev <= ULP and ej <= ULP and eb <= ULP, name
        assert np.array_equal(br.bounds(g[f"{name}_vertices"]), g[f"{name}_bounds"])                  # the recorded bounds are that arithmetic
    assert np.all(g["b1_poses"][0, 3 * int(g["zero_joint"]):3 * int(g["zero_joint"]) + 3] == 0) and np.abs(g["b1_poses"]).max() > 0.3
    assert not np.allclose(g["b1_R"], np.eye(3)) and np.abs(g["b1_Th"]).min() > 0
    assert g["ids"].shape == (2048,) and len(np.unique(g["ids"])) > 2048 // 8


def _official_like(model):
    """The synthetic model dressed like the official pickle: float64 arrays, a scipy-sparse regressor, the root's parent 2^32 - 1."""
    import scipy.sparse
    kt = model["kintree_table"].numpy().astype(np.uint32)
    kt[0, 0] = 4294967295
    return {"v_template": model["v_template"].double().numpy(), "shapedirs": model["shapedirs"].double().numpy(),
            "posedirs": model["posedirs"].double().numpy(), "weights": model["weights"].double().numpy(),
            "J_regressor": scipy.sparse.csc_matrix(model["J_regressor"].double().numpy()), "kintree_table": kt,
            "f": np.zeros((5, 3), dtype=np.uint32), "bs_style": "lbs"}


def test_loader_sources_and_errors(tmp_path):
    from humanliff_amd.body import BodyModel, load_body_model
    model = syn.smpl_like_model(300, 4)
    want = {k: v for k, v in model.items()}
    from_dict = load_body_model(dict(model), "cpu")
    np.savez(tmp_path / "m.npz", **{k: v.numpy() for k, v in model.items()})
    from_npz = load_body_model(str(tmp_path / "m.npz"), "cpu")
    with open(tmp_path / "m.pkl", "wb") as f:
        pickle.dump(_official_like(model), f, protocol=2)
    from_pkl = load_body_model(str(tmp_path / "m.pkl"), "cpu")
    for got in (from_dict, from_npz, from_pkl):
        assert isinstance(got, BodyModel) and got.parents == syn.SMPL_PARENTS and (got.V, got.J, got.Sp) == (300, 24, 10)
        assert set(got.tensors) == {"v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights", "f"}
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):
            assert got.tensors[k].dtype == torch.float32 and torch.equal(got.tensors[k], want[k]), k
        assert got.tensors["kintree_table"].dtype == torch.long and got.tensors["f"].dtype == torch.long
        assert torch.equal(got.tensors["kintree_table"][:, 1:], want["kintree_table"][:, 1:])
    assert int(from_pkl.tensors["kintree_table"][0, 0]) == 4294967295 and tuple(from_pkl.tensors["f"].shape) == (5, 3)

    for key in ("posedirs", "J_regressor", "kintree_table", "f"):
        with pytest.raises(KeyError, match=key):
            load_body_model({k: v for k, v in model.items() if k != key}, "cpu")
    bad = dict(model)
    bad["kintree_table"] = model["kintree_table"].clone()
    bad["kintree_table"][0, 3] = 7                         # joint 3 hangs on joint 7
    with pytest.raises(ValueError, match="joint 3"):
        load_body_model(bad, "cpu")
    with open(tmp_path / "ch.pkl", "wb") as f:             # GLOBAL chumpy.Ch, as the official files' arrays are stored
        f.write(b"cchumpy\nCh\n.")
    with pytest.raises(ImportError, match="chumpy"):
        load_body_model(str(tmp_path / "ch.pkl"), "cpu")


def test_big_pose_params_are_the_reference_values(golden):
    from humanliff_amd.body import load_body_model
    bp = load_body_model(syn.smpl_like_model(300, 4), "cpu").big_pose_params()
    assert set(bp) == {"R", "Th", "shapes", "poses"}
    for k in bp:
        assert bp[k].dtype == np.float32 and np.array_equal(bp[k], golden[f"b2_{k}"].reshape(bp[k].shape)), k
    assert bp["poses"].shape == (1, 72) and bp["shapes"].shape == (1, 10) and bp["Th"].shape == (1, 3)
    assert np.count_nonzero(bp["poses"]) == 4 and bp["poses"][0, 5] == np.float32(np.pi / 4) and bp["poses"][0, 26] == np.float32(np.pi / 6)


def test_header_declares_the_exports():
    from humanliff_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_body_")) == sorted(EXPORTS)
    # sizes: the packed model is every array once plus the regressor products; bad sizes give no size and a status before any launch
    V, J, S = 6890, 24, 10
    assert L.hl_body_packed_bytes(V, J, S) == 4 * ((207 + S) * 3 * V + J * V + 3 * V + 3 * J + 3 * J * S)
    assert L.hl_body_packed_bytes(V, 65, S) == 0 and L.hl_body_packed_bytes(V, J, 17) == 0 and L.hl_body_packed_bytes(0, J, S) == 0
    assert L.hl_body_pose_workspace_bytes(J, 3) == 4 * 3 * (J * 16 + 207) and L.hl_body_pose_workspace_bytes(J, 0) == 0
    assert L.hl_body_chunk_frames() >= 2
    assert L.hl_body_pose(None, None, V, J, S, S, 1, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 0, None) < 0
    assert b"hl_body_pose" in L.hl_last_error()
    assert L.hl_body_pack(None, None, S, None, None, None, V, J, S, None, None) < 0 and b"hl_body_pack" in L.hl_last_error()


def test_cpu_tensors_are_refused():
    from humanliff_amd.body import load_body_model
    model = load_body_model(syn.smpl_like_model(300, 4), "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.pose(torch.zeros(72), torch.zeros(10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.big_pose()
