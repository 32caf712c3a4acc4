"""GPU, end to end: a TightCap-shaped fixture tree (tests/tightcap_fixture.py: 1 subject x 1 pose x 4 orbit views of 64 x 64, one photograph
and five masks per view, synthetic.smpl_like_model(256) as the body) through TightCapIndex and load_view_store - the four cloth layers of
every view composed on the device, at image_scaling 1.0 and 0.5 - into the device-resident fitting path."""
import numpy as np
import pytest
import torch

from tests import tightcap_fixture as fx
from tests import tightcap_restatement as tr

pytestmark = pytest.mark.gpu
SIZE, VIEWS = 64, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def body_model(dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.body import load_body_model
    return load_body_model(syn.smpl_like_model(n_vertices=256), dev)


@pytest.fixture(scope="module")
def loaded(dev, body_model, tmp_path_factory):
    """(index, {image_scaling: store}, files): the 16 views (4 layers x 4 cameras) loaded once per scaling (read only)."""
    from humanliff_amd.recon_NeRF.lib.TightCap_dataset import TightCapIndex, load_view_store
    base = tmp_path_factory.mktemp("tightcap_gpu")
    data_root, files = fx.write_tree(base, n_subjects=1, poses=(0,), n_views=VIEWS, size=SIZE)
    index = TightCapIndex(data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=1, poses_num=1, views_num=VIEWS)
    assert len(index) == 16
    stores = {1.0: load_view_store(index, body_model, device=dev, decode_threads=4),                      # (image_scaling defaults to 1.0)
              0.5: load_view_store(index, body_model, image_scaling=0.5, device=dev, decode_threads=4)}
    return index, stores, files


def decoded(index):
    """(img_u8 (16, 64, 64, 3), {plane: (16, 64, 64)}, layers): the files every item names, decoded; planes it does not name are None-like zeros."""
    from humanliff_amd.recon_NeRF.lib.TightCap_dataset import read_image, read_mask
    items = [index.item(i) for i in range(len(index))]
    img = np.stack([read_image(it[4]) for it in items])
    planes = {n: np.stack([read_mask(it[5][n]) if n in it[5] else np.zeros((SIZE, SIZE), dtype=np.uint8) for it in items]) for n in tr.PLANES}
    return img, planes, [it[1] for it in items]


@pytest.mark.parametrize("scaling", [1.0, 0.5])
def test_store_follows_the_index(loaded, dev, scaling):
    index, stores, files = loaded
    store, side = stores[scaling], int(SIZE * scaling)
    assert len(store) == 16 and (store.H, store.W) == (side, side)
    assert store.images.dtype == torch.float32 and tuple(store.images.shape) == (16, side, side, 3) and store.images.device == dev
    counts = store.class_counts().cpu().numpy()
    print("class counts (body, background) per view:", counts.tolist())
    assert (counts > 0).all()
    assert store.instance_idx.tolist() == [0] * 16 and store.cloth_layer_index.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    assert store.view_index.tolist() == [0, 1, 2, 3] * 4 and store.pose_index.tolist() == [0] * 16 and store.dataset_index.tolist() == list(range(16))
    for i in range(16):
        K = index.item(i)[6]
        assert np.array_equal(store.K[i][:2], K[:2] * scaling) and np.array_equal(store.K[i][2], K[2])
        assert np.array_equal(store.R[i], index.item(i)[7]) and np.array_equal(store.T[i], index.item(i)[8][:, 0])


@pytest.mark.parametrize("scaling", [1.0, 0.5])
def test_images_are_the_restated_ingest_of_the_decoded_files(loaded, scaling):
    index, stores, files = loaded
    store, side = stores[scaling], int(SIZE * scaling)
    img, planes, layers = decoded(index)
    ref = tr.ingest(img, planes, layers, side, side)
    got, body = store.images.cpu().numpy(), store.body.cpu().numpy()
    if scaling == 1.0:
        assert np.array_equal(got, ref["source"])                                          # the composed source itself
    else:
        bound = 2 * float(np.abs(ref["f32"].astype(np.float64) - ref["f64"]).max())        # the rule of tests/view_ingest_cases.py for this shape
        err = float(np.abs(got.astype(np.float64) - ref["f64"]).max())
        print(f"max |store.images - float64 restatement| {err:.4e} (bound {bound:.4e})")
        assert err <= bound
    assert np.array_equal(body, ref["body"])
    per_layer = body.reshape(4, -1).sum(axis=1)
    print("body pixels per layer:", per_layer.tolist())
    assert (np.diff(per_layer) > 0).all()                                                  # every layer adds a garment to the one below
    assert (ref["source"] == tr.SKIN).all(axis=-1).reshape(4, -1).any(axis=1).tolist() == [True, True, True, False]


def test_world_bounds_carry_the_tightcap_margin(loaded, body_model, dev):
    """prepare_input (:163-168): min / max of the posed vertices, - / + 0.05 on every axis and another 0.1 on y; pose() without y_margin
    keeps SynBody's 0.05."""
    from humanliff_amd.recon_NeRF.lib.TightCap_dataset import smpl_params
    index, stores, files = loaded
    p = smpl_params(index.smpl_path(0), 0)
    args = (torch.from_numpy(p['poses']).to(dev), torch.from_numpy(p['shapes'].reshape(-1)).to(dev), p['R'], p['Th'])
    xyz = body_model.pose(*args).vertices[0].cpu().numpy()

    def padded(y):
        lo, hi = np.min(xyz, axis=0), np.max(xyz, axis=0)
        lo, hi = lo - np.float32(0.05), hi + np.float32(0.05)
        lo[1], hi[1] = lo[1] - np.float32(y), hi[1] + np.float32(y)
        return np.stack([lo, hi])

    assert np.array_equal(body_model.pose(*args).world_bounds[0].cpu().numpy(), padded(0.05))                # unchanged, bit for bit
    assert np.array_equal(body_model.pose(*args, y_margin=0.05).world_bounds[0].cpu().numpy(), padded(0.05))
    assert np.array_equal(body_model.pose(*args, y_margin=0.1).world_bounds[0].cpu().numpy(), padded(0.1))
    for store in stores.values():
        assert store.bounds.shape == (16, 2, 3)
        for v in range(16):
            assert np.array_equal(store.bounds[v], padded(0.1).astype(np.float64)), v
    assert not np.array_equal(padded(0.1), padded(0.05))


def test_ray_batch_and_fit_step(loaded, dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.recon_NeRF import Renderer
    from humanliff_amd.recon_NeRF.fit import FitLoop
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader, sample_ray_batch
    index, stores, files = loaded
    store = stores[0.5]
    view_ids = torch.tensor([13, 2], device=dev)
    out = sample_ray_batch(store, view_ids, 128, seed=3, step=0)
    assert (out["n_valid"] > 0).all()
    for b, v in enumerate(view_ids.tolist()):
        n = int(out["n_valid"][b])
        yx = out["coord"][b, 0, :n].long()
        assert torch.equal(out["rgb"][b, 0, :n], store.images[v, yx[:, 0], yx[:, 1]])
        assert torch.equal(out["bkgd_msk"][b, 0, :n, 0], store.body[v, yx[:, 0], yx[:, 1]].float())
    torch.manual_seed(0)
    model = Renderer(use_canonical_space=False, num_instances=1, triplane_dim=64, triplane_ch=27, test=False)
    model.load_state_dict(syn.render_mlp_state(3), strict=False)
    model = model.to(dev)
    loader = RayBatchLoader(store, batch_size=2, n_rays=128, seed=1)
    loop = FitLoop(model, loader, lrate=5e-4, tri_plane_lrate=1e-2, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4, use_clamp=True,
                   n_samples=16, n_importance=16)
    tp = next(iter(loader))
    assert tp["cloth_layer_index"].tolist() == [int(store.cloth_layer_index[i]) for i in tp["image_idx"].tolist()]
    losses = torch.stack(loop.step(tp))
    print("losses of one step:", losses.tolist())
    assert bool(torch.isfinite(losses).all())


def test_memory_error_names_the_views_that_fit(loaded, body_model, dev, monkeypatch):
    from humanliff_amd.recon_NeRF.lib import TightCap_dataset as td
    index, stores, files = loaded
    one = td.store_bytes(1, 32, 32)
    staging = 16 * (SIZE * SIZE * 8 + 32 * 32 * 13)                                       # 8 source bytes a pixel: the image and five planes
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (staging + 3 * one + 5, 1 << 40))
    with pytest.raises(MemoryError, match=r"\b3 views would fit"):
        td.load_view_store(index, body_model, image_scaling=0.5, device=dev)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1024, 1 << 40))
    with pytest.raises(MemoryError, match=r"\b0 views would fit"):
        td.load_view_store(index, body_model, image_scaling=0.5, device=dev)


def test_bad_inputs_raise(loaded, body_model, dev, tmp_path):
    from PIL import Image
    from humanliff_amd.recon_NeRF.lib import TightCap_dataset as td
    index, stores, files = loaded
    with pytest.raises(ValueError):
        td.load_view_store(index, body_model, image_scaling=1.5, device=dev, items=range(4))
    with pytest.raises(ValueError):
        td.load_view_store(index, body_model, device=dev, items=[])
    # a tree whose second view has a shoes mask of another size: the error names the file, and only a layer that reads it trips
    data_root, other = fx.write_tree(tmp_path, n_subjects=1, poses=(0,), n_views=2, size=16, radius=3.0)
    Image.fromarray(np.zeros((16, 20), dtype=np.uint8)).save(other[(0, 0, 1)][1]['shoes'])
    kw = dict(multi_person=True, num_instance=1, pose_start=0, pose_interval=1, poses_num=1, views_num=2)
    with pytest.raises(ValueError, match=r"shoes.*camera0001"):
        td.load_view_store(td.TightCapIndex(data_root, layer_idx=2, **kw), body_model, device=dev)
    assert len(td.load_view_store(td.TightCapIndex(data_root, layer_idx=3, **kw), body_model, device=dev)) == 2
