"""The TightCap reader and the layered-ingest contract without a GPU: the numpy restatement of DESIGN.md 4j against the golden recorded from
the reference's TightCapDatasetBatch.__getitem__ (tests/golden/gen_golden_tightcap.py), TightCapIndex against a literal restatement of
the reference's index arithmetic and paths (recon_NeRF/lib/TightCap_dataset.py:218-315), a fixture tree read back, and the host-side
checks of the new library entries."""
import inspect
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import synbody_fixture as sf
from tests import tightcap_cases as tc
from tests import tightcap_fixture as fx
from tests import tightcap_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tightcap_layers.npz")
LAYER_MASKS = {0: ('full', 'person', 'top', 'bottom', 'shoes'), 1: ('full', 'person', 'top', 'shoes'), 2: ('full', 'person', 'shoes'), 3: ('full',)}


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_fixture_masks_take_every_combination_in_every_view(golden):
    planes = {n: golden["plane_" + n] for n in tr.PLANES}
    combo = tc.combinations(planes)
    black = ~golden["img_u8"].any(axis=-1)
    for v in range(combo.shape[0]):
        assert set(np.unique(combo[v])) == set(range(32)), v
        assert set(np.unique(combo[v][black[v]])) == set(range(32)), v        # ... also under pixels whose bytes are (0, 0, 0)
        assert set(np.unique(combo[v][~black[v]])) == set(range(32)), v
    assert {int(x) for n in tr.PLANES for x in np.unique(planes[n])} == {0, 1, 128, 255}  # binary means byte != 0
    # kept pixels whose bytes are (0, 0, 0): background for a layer below 3, body for layer 3
    for i, (layer, v) in enumerate(zip(golden["layers"], golden["views"])):
        full, person = planes["full"][v] != 0, planes["person"][v] != 0
        s = person.astype(int) + sum((planes[g][v] != 0).astype(int) for g in (tr.GARMENTS[layer] if layer < 3 else ()))
        kept_black = full & black[v] & (s < 2) & ~(~person & (s == 1)) if layer < 3 else full & black[v]
        assert kept_black.any(), i
        assert (golden["msk_all"][i][kept_black] == (1.0 if layer == 3 else 0.0)).all(), i
    # the cases the GPU tests run take every combination too
    for name in list(tc.REDUCTIONS) + ["copy"]:
        img, planes, layers, H, W = tc.case(name)
        combo = tc.combinations(planes)
        assert all(set(np.unique(combo[v])) == set(range(32)) for v in range(len(layers))), name
    assert (5 * 9 * 15) % 4 != 0 and tc.COPY[:3] == (5, 9, 15)


def test_restatement_equals_the_reference_bit_for_bit(golden):
    planes = {n: golden["plane_" + n] for n in tr.PLANES}
    assert golden["layers"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and golden["views"].tolist() == [0, 1] * 4
    assert golden["img_all"].dtype == np.float32 and golden["img_all"].shape == (8, 3, 24, 28)
    seen = set()
    for i, (layer, v) in enumerate(zip(golden["layers"], golden["views"])):
        named = {n: planes[n][v] for n in LAYER_MASKS[int(layer)]}                   # only what the layer names: anything else is a KeyError
        src, mask = tr.compose_view(golden["img_u8"][v], named, int(layer))
        assert src.dtype == np.float32 and mask.dtype == np.uint8
        assert np.array_equal(src.transpose(2, 0, 1), golden["img_all"][i]), i
        assert np.array_equal(mask.astype(np.float64), golden["msk_all"][i]), i
        skin = (src == tr.SKIN).all(axis=-1)
        assert skin.any() == (layer < 3) and mask[skin].all()
        seen.add(src.tobytes())
    assert len(seen) == 8                                                            # every layer of every view is another image
    batch_src, batch_mask = tr.compose(golden["img_u8"][golden["views"]], {n: p[golden["views"]] for n, p in planes.items()}, golden["layers"])
    assert np.array_equal(batch_src.transpose(0, 3, 1, 2), golden["img_all"]) and np.array_equal(batch_mask, golden["msk_all"].astype(np.uint8))


def test_order_of_the_table_rows():
    """Two garments and no body give skin, not zero; full == 0 wins over everything."""
    img = np.full((1, 6, 3), 200, dtype=np.uint8)
    z = lambda *bits: np.array([bits], dtype=np.uint8) * 255  # noqa: E731
    #                    pixel: 0  1  2  3  4  5
    planes = {"full": z(1, 1, 1, 0, 1, 1), "person": z(0, 0, 1, 1, 1, 0), "top": z(1, 1, 1, 1, 0, 0), "bottom": z(1, 0, 0, 1, 0, 0),
              "shoes": z(0, 0, 0, 1, 0, 0)}
    keep = np.float32(200) / np.float32(255)
    src, mask = tr.compose_view(img, planes, 0)
    assert np.array_equal(src[0, 0], tr.SKIN) and not src[0, 1].any() and np.array_equal(src[0, 2], tr.SKIN) and not src[0, 3].any()
    assert (src[0, 4] == keep).all() and (src[0, 5] == keep).all() and mask.tolist() == [[1, 0, 1, 0, 1, 1]]
    src1, mask1 = tr.compose_view(img, {k: v for k, v in planes.items() if k != "bottom"}, 1)    # layer 1 does not see the bottom
    assert not src1[0, 0].any() and mask1.tolist() == [[0, 0, 1, 0, 1, 1]]
    src3, mask3 = tr.compose_view(img, {"full": planes["full"]}, 3)
    assert mask3.tolist() == [[1, 1, 1, 0, 1, 1]] and (src3[0, :3] == keep).all() and not src3[0, 3].any()
    with pytest.raises(ValueError):
        tr.compose_view(img, planes, 4)
    assert tr.SKIN.dtype == np.float32 and tr.SKIN.view(np.uint32).tolist() == [1058762891, 1056726055, 1054882872]


def test_world_bounds_pad_y_by_a_further_tenth(golden):
    """prepare_input :163-168: - / + 0.05 on every axis, then y by 0.1, in float32 and in that order."""
    for verts, got in zip(golden["vertices"], golden["world_bounds"]):
        lo, hi = verts.min(axis=0), verts.max(axis=0)
        lo, hi = lo - np.float32(0.05), hi + np.float32(0.05)
        lo[1], hi[1] = lo[1] - np.float32(0.1), hi[1] + np.float32(0.1)
        assert got.dtype == np.float32 and np.array_equal(got, np.stack([lo, hi]))


# ---- the index --------------------------------------------------------------------------------------------------------------------
def reference_item(root_list, cams_all, index, multi_person, cloth_layer_num, ni, n_views, i_intv, i, layer_idx):
    """__getitem__ :218-302 with its own expressions (self.output_view has n_views entries)."""
    instance_idx = index // (cloth_layer_num * ni * n_views) if multi_person else 0
    cloth_layer_index = (index - instance_idx * cloth_layer_num * ni * n_views) // (ni * n_views)
    pose_index = (index - instance_idx * cloth_layer_num * ni * n_views - cloth_layer_index * ni * n_views) // n_views * i_intv + i
    view_index = index % n_views
    data_root = root_list[instance_idx]
    cams = cams_all[instance_idx]
    if layer_idx is not None:
        cloth_layer_index = layer_idx
    img_path = os.path.join(data_root, 'person-top-bottom-shoes', 'img', f'camera{str(view_index).zfill(4)}', str(pose_index).zfill(4) + '.jpg')
    mask = lambda d: os.path.join(data_root, d, 'mask', f'camera{str(view_index).zfill(4)}', str(pose_index).zfill(4) + '.png')  # noqa: E731
    masks = {'full': mask('person-top-bottom-shoes')}
    if cloth_layer_index < 3:
        masks['person'], masks['shoes'] = mask('person'), mask('shoes')
    if cloth_layer_index < 2:
        masks['top'] = mask('top')
    if cloth_layer_index < 1:
        masks['bottom'] = mask('bottom')
    K = np.array(cams[f'camera{str(view_index).zfill(4)}']['K'])
    R = np.array(cams[f'camera{str(view_index).zfill(4)}']['R'])
    T = np.array(cams[f'camera{str(view_index).zfill(4)}']['T']).reshape(-1, 1)
    return instance_idx, cloth_layer_index, pose_index, view_index, img_path, masks, K, R, T


@pytest.fixture(scope="module")
def index_tree(tmp_path_factory):
    """TightCap_human_list.txt (three names, two used) and per-subject cameras.json with distinct numbers; the index needs no image files."""
    base = tmp_path_factory.mktemp("tightcap_index")
    names = ['human_a', 'human_b', 'human_c']
    (base / 'TightCap_human_list.txt').write_text(''.join(n + '\n' for n in names))
    cams_all = []
    for s, n in enumerate(names):
        cams = sf.orbit_cameras(3, 32)
        for v, c in enumerate(cams.values()):
            c['K'][0][0] += s + 0.25 * v
        (base / n / 'person-top-bottom-shoes').mkdir(parents=True)
        (base / n / 'person-top-bottom-shoes' / 'cameras.json').write_text(json.dumps(cams))
        cams_all.append(cams)
    return str(base), names, cams_all


@pytest.mark.parametrize("layer_idx", [None, 1])
def test_index_equals_the_reference_arithmetic_for_every_index(index_tree, layer_idx):
    from humanliff_amd.recon_NeRF.lib.TightCap_dataset import TightCapIndex
    base, names, cams_all = index_tree
    data_root = os.path.join(base, names[0])
    idx = TightCapIndex(data_root, multi_person=True, num_instance=2, pose_start=1, pose_interval=5, poses_num=2, views_num=3, layer_idx=layer_idx)
    layers = 4 if layer_idx is None else 1
    assert len(idx) == 2 * layers * 2 * 3                                              # __len__ :385-386
    root_list = [os.path.join(base, n) for n in names[:2]]
    assert idx.root_list == root_list
    seen = set()
    for i in range(len(idx)):
        got = idx.item(i)
        want = reference_item(root_list, cams_all, i, True, layers, 2, 3, 5, 1, layer_idx)
        assert got[:6] == want[:6], i
        assert tuple(sorted(got[5])) == tuple(sorted(LAYER_MASKS[got[1]])), i               # the masks the layer names and no other
        for g, w in zip(got[6:], want[6:]):
            assert g.shape == w.shape and g.dtype == np.float64 and np.array_equal(g, w), i
        seen.add(got[:4])
    assert len(seen) == len(idx)
    assert {s[2] for s in seen} == {1, 6} and {s[1] for s in seen} == ({0, 1, 2, 3} if layer_idx is None else {1})
    assert idx.smpl_path(1) == os.path.join(root_list[1], 'person-top-bottom-shoes/outputs_re_fitting/refit_smpl_2nd.npz')


def test_index_single_person_defaults_and_refusals(index_tree):
    from humanliff_amd.recon_NeRF.lib import TightCap_dataset as td
    base, names, cams_all = index_tree
    data_root = os.path.join(base, names[1])
    idx = td.TightCapIndex(data_root, multi_person=False, num_instance=1, pose_start=0, pose_interval=1, poses_num=1, views_num=3, layer_idx=3)
    assert idx.root_list == [data_root] and len(idx) == 3
    for i in range(len(idx)):
        got, want = idx.item(i), reference_item([data_root], cams_all[1:], i, False, 1, 1, 3, 1, 0, 3)
        assert got[:6] == want[:6] and np.array_equal(got[6], want[6]) and list(got[5]) == ['full']
    assert inspect.signature(td.TightCapIndex).parameters['views_num'].default == 382      # :20
    assert inspect.signature(td.load_view_store).parameters['image_scaling'].default == 1.0
    with pytest.raises(NotImplementedError):
        td.TightCapIndex(data_root, smpl_type='smplx')
    for bad in (4, -1):
        with pytest.raises(ValueError):
            td.TightCapIndex(data_root, layer_idx=bad)
    with pytest.raises(RuntimeError):
        td.load_view_store(idx, None, device="cpu", items=[0])
    # the helpers are SynBody_dataset's own, not copies
    from humanliff_amd.recon_NeRF.lib import SynBody_dataset as sd
    for name in ("read_image", "read_mask", "smpl_params", "scaled_size", "scaled_intrinsics", "store_bytes", "store_test_views"):
        assert getattr(td, name) is getattr(sd, name)
    src = inspect.getsource(td)
    assert "cpu_count" not in src and "import cv2" not in src and "import imageio" not in src


def test_fixture_tree_is_read_back(tmp_path):
    from humanliff_amd.recon_NeRF.lib import TightCap_dataset as td
    data_root, files = fx.write_tree(tmp_path, n_subjects=1, poses=(0, 2), n_views=2, size=16, radius=4.0, jpeg=False)
    idx = td.TightCapIndex(data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=2, poses_num=2, views_num=2)
    assert len(idx) == 16
    for i in range(16):
        inst, layer, pose, view, img_path, mask_paths, K, R, T = idx.item(i)
        want_img, want_paths = files[(inst, pose, view)]
        assert img_path == want_img and img_path.endswith('.png')                        # (only the PNG exists)
        assert mask_paths == {n: want_paths[n] for n in LAYER_MASKS[layer]}
        img, planes = fx.view_arrays(16, pose * 100 + view, 4.0)
        assert np.array_equal(td.read_image(img_path), img)
        for n, p in mask_paths.items():
            assert np.array_equal(td.read_mask(p), planes[n])
    img, planes = fx.view_arrays(64, 0, 7.0)
    combo = set(np.unique(tc.combinations(planes)))
    # body under the top, under both garments, bare body, garment beside the body, garment outside `full`, background
    assert {0b00011, 0b00111, 0b01111, 0b00101, 0b00100, 0} <= combo, sorted(combo)


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    from humanliff_amd import _lib, view_ingest
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in ("hl_view_ingest_layers", "hl_pose_body_margins"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # arguments are checked before anything is launched (the pointers are never read: 16 is only an aligned non-NULL value)
    f = L.hl_view_ingest_layers
    assert f(16, 16, 16, 16, 16, 16, 16, 1, 8, 8, 9, 8, 16, 16, 16, 16, None) < 0 and b"enlarges" in L.hl_last_error()
    assert f(16, None, 16, 16, 16, 16, 16, 1, 8, 8, 4, 4, 16, 16, 16, 16, None) < 0 and b"hl_view_ingest_layers" in L.hl_last_error()
    assert f(16, 16, 16, 16, 16, 16, None, 1, 8, 8, 4, 4, 16, 16, 16, 16, None) < 0 and b"NULL" in L.hl_last_error()
    assert f(16, 16, 16, 24, 16, 16, 16, 1, 8, 8, 4, 4, 16, 16, 16, 16, None) < 0 and b"aligned" in L.hl_last_error()
    assert f(16, 16, None, None, None, None, 16, 1, 8, 8, 4, 4, None, 16, 16, 16, None) < 0 and b"tap table" in L.hl_last_error()
    assert f(16, 16, 16, 16, 16, 16, 16, 1, 8, 64000, 4, 100, 16, 16, 16, 16, None) < 0 and b"LDS" in L.hl_last_error()
    g = L.hl_pose_body_margins
    assert g(None, None, 8, 24, 10, 10, 1, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 0, -0.05, 0.1, None) < 0
    assert b"margins" in L.hl_last_error()
    assert g(None, None, 8, 24, 10, 10, 1, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 0, 0.05, 0.1, None) < 0
    assert b"NULL" in L.hl_last_error()
    # the wrapper's own checks that need no device
    assert view_ingest.planes_read([3, 3]) == ("full",) and view_ingest.planes_read([2]) == ("full", "person", "shoes")
    assert view_ingest.planes_read([1, 3]) == ("full", "person", "top", "shoes") and view_ingest.planes_read([2, 0]) == view_ingest.PLANES
    assert view_ingest.LAYER_PLANES == tuple(LAYER_MASKS[i] for i in range(4)) and view_ingest.PLANES == tr.PLANES
    for bad in ([0, 4], [-1]):
        with pytest.raises(ValueError):
            view_ingest.planes_read(bad)
    import torch
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        view_ingest.ingest_layered_views(x, (x[..., 0], None, None, None, None), [3], 4, 4)   # no CPU path


def test_layered_kernels_use_no_scratch_and_the_existing_ones_are_still_there():
    from humanliff_amd import build
    src = os.path.join(build.CSRC, "hl_view_ingest.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "view_ingest.s")
        r = subprocess.run([build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        text = open(out).read()
    meta = text[text.index(".amdgpu_metadata"):]
    seen = {}
    for entry in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+\S*?(k_(?:view|layers)_[a-z]+)E", entry)
        if m:
            md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
            assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (m.group(1), md)
            assert md["group_segment_fixed_size"] == 0, (m.group(1), md)                       # (the staging area is dynamic LDS)
            seen[m.group(1)] = md
    assert sorted(seen) == ["k_layers_convert", "k_layers_ingest", "k_view_convert", "k_view_ingest"]
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in seen.items()})
