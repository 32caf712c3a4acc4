"""GPU, end to end: a SynBody-shaped fixture tree (tests/synbody_fixture.py: 1 subject x 2 layers x 1 pose x 4 orbit views of 64 x 64, a
disc mask inside the projected bounds, synthetic.smpl_like_model(256) as the body) through load_view_store(image_scaling=0.5) into the
device-resident fitting path."""
import numpy as np
import pytest
import torch

from tests import synbody_fixture as fx
from tests import view_ingest_restatement as vr

pytestmark = pytest.mark.gpu
SIZE, VIEWS, SCALING = 64, 4, 0.5


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
    """(index, store, files): the 8 views of the two layers on disk, loaded once (read only)."""
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import SynBodyIndex, load_view_store
    base = tmp_path_factory.mktemp("synbody_gpu")
    data_root, files = fx.write_tree(base, n_subjects=1, layers=(0, 1), poses=(0,), n_views=VIEWS, size=SIZE, png_images=((0, 1, 0, 2),))
    index = SynBodyIndex(data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=1, poses_num=1, views_num=VIEWS)
    assert len(index) == 16
    store = load_view_store(index, body_model, image_scaling=SCALING, device=dev, items=range(8), decode_threads=4)
    return index, store, files


def test_store_follows_the_index(loaded, dev):
    index, store, files = loaded
    assert len(store) == 8 and (store.H, store.W) == (32, 32)
    assert store.images.dtype == torch.float32 and tuple(store.images.shape) == (8, 32, 32, 3) and store.images.device == dev
    counts = store.class_counts().cpu().numpy()
    print("class counts (body, background) per view:", counts.tolist())
    assert (counts > 0).all()                                                             # every view has pixels of both classes
    assert store.instance_idx.tolist() == [0] * 8 and store.cloth_layer_index.tolist() == [0] * 4 + [1] * 4
    assert store.view_index.tolist() == [0, 1, 2, 3] * 2 and store.pose_index.tolist() == [0] * 8 and store.dataset_index.tolist() == list(range(8))
    for i in range(8):
        K = index.item(i)[6]
        assert np.array_equal(store.K[i][:2], K[:2] * SCALING) and np.array_equal(store.K[i][2], K[2])
        assert np.array_equal(store.R[i], index.item(i)[7]) and np.array_equal(store.T[i], index.item(i)[8][:, 0])


def test_images_are_the_restated_ingest_of_the_decoded_files(loaded):
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import read_image, read_mask
    index, store, files = loaded
    img = np.stack([read_image(index.item(i)[4]) for i in range(8)])
    msk = np.stack([read_mask(index.item(i)[5]) for i in range(8)])
    src = vr.masked_source(img, msk)
    want64, want32 = vr.resize_area_f64(src, 32, 32), vr.resize_area_f32(src, 32, 32)
    bound = 2 * float(np.abs(want32.astype(np.float64) - want64).max())                   # the rule of tests/view_ingest_cases.py for this shape
    got = store.images.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want64).max())
    print(f"max |store.images - float64 restatement| {err:.4e} (bound {bound:.4e})")
    assert err <= bound
    assert np.array_equal(store.body.cpu().numpy(), vr.resize_nearest(msk, 32, 32))
    assert 0 < store.body.sum().item() < store.body.numel()


def test_world_bounds_follow_prepare_input(loaded, body_model, dev):
    """prepare_input (:186-192): min / max of the posed vertices, - / + 0.05 on every axis and another 0.05 on y."""
    from humanliff_amd.recon_NeRF.lib.SynBody_dataset import smpl_params
    index, store, files = loaded
    p = smpl_params(index.smpl_path(0), 0)
    posed = body_model.pose(torch.from_numpy(p['poses']).to(dev), torch.from_numpy(p['shapes'].reshape(-1)).to(dev), p['R'], p['Th'])
    xyz = posed.vertices[0].cpu().numpy()
    min_xyz, max_xyz = np.min(xyz, axis=0), np.max(xyz, axis=0)
    min_xyz -= 0.05
    max_xyz += 0.05
    min_xyz[1] -= 0.05
    max_xyz[1] += 0.05
    want = np.stack([min_xyz, max_xyz], axis=0)
    assert store.bounds.shape == (8, 2, 3)
    for v in range(8):
        assert np.abs(store.bounds[v] - want).max() <= 2 * np.spacing(np.float32(2.0)), v   # float32 sums of values below 2, in either order
    assert (want[1] - want[0] > 0.1).all()


def test_ray_batch_and_fit_step(loaded, dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.recon_NeRF import Renderer
    from humanliff_amd.recon_NeRF.fit import FitLoop
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader, sample_ray_batch
    index, store, files = loaded
    view_ids = torch.tensor([5, 2], device=dev)
    out = sample_ray_batch(store, view_ids, 128, seed=3, step=0)
    assert (out["n_valid"] > 0).all()
    for b, v in enumerate(view_ids.tolist()):
        n = int(out["n_valid"][b])
        yx = out["coord"][b, 0, :n].long()
        assert torch.equal(out["rgb"][b, 0, :n], store.images[v, yx[:, 0], yx[:, 1]])
        body = store.body[v, yx[:, 0], yx[:, 1]]
        assert torch.equal(out["bkgd_msk"][b, 0, :n, 0], body.float())
    torch.manual_seed(0)
    model = Renderer(use_canonical_space=False, num_instances=1, triplane_dim=64, triplane_ch=27, test=False)
    model.load_state_dict(syn.render_mlp_state(3), strict=False)
    model = model.to(dev)
    loader = RayBatchLoader(store, batch_size=2, n_rays=128, seed=1)
    loop = FitLoop(model, loader, lrate=5e-4, tri_plane_lrate=1e-2, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4, use_clamp=True,
                   n_samples=16, n_importance=16)
    tp = next(iter(loader))
    assert tp["cloth_layer_index"].tolist() == [int(store.cloth_layer_index[i]) for i in tp["image_idx"].tolist()]
    assert tp["instance_idx"].tolist() == [0, 0]
    losses = torch.stack(loop.step(tp))
    print("losses of one step:", losses.tolist())
    assert bool(torch.isfinite(losses).all())


def test_memory_error_names_the_views_that_fit(loaded, body_model, dev, monkeypatch):
    from humanliff_amd.recon_NeRF.lib import SynBody_dataset as sd
    index, store, files = loaded
    one = sd.store_bytes(1, 32, 32)
    staging = 8 * (SIZE * SIZE * 4 + 32 * 32 * 13)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (staging + 3 * one + 5, 1 << 40))
    with pytest.raises(MemoryError, match=r"\b3 views would fit"):
        sd.load_view_store(index, body_model, image_scaling=SCALING, device=dev, items=range(8))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1024, 1 << 40))
    with pytest.raises(MemoryError, match=r"\b0 views would fit"):
        sd.load_view_store(index, body_model, image_scaling=SCALING, device=dev, items=range(8))


def test_bad_inputs_raise(loaded, body_model, dev, tmp_path):
    from PIL import Image
    from humanliff_amd.recon_NeRF.lib import SynBody_dataset as sd
    index, store, files = loaded
    with pytest.raises(ValueError):
        sd.load_view_store(index, body_model, image_scaling=1.5, device=dev, items=range(8))
    with pytest.raises(ValueError):
        sd.load_view_store(index, body_model, image_scaling=SCALING, device=dev, items=[])
    # a tree whose second image has another size: the error names the file
    data_root, other = fx.write_tree(tmp_path, n_subjects=1, layers=(0,), poses=(0,), n_views=2, size=16, png_images=(), radius=3.0)
    odd = other[(0, 0, 0, 1)][0]
    Image.fromarray(np.zeros((16, 20, 3), dtype=np.uint8)).save(odd)
    idx = sd.SynBodyIndex(data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=1, poses_num=1, views_num=2, layer_idx=0)
    with pytest.raises(ValueError, match="camera0001"):
        sd.load_view_store(idx, body_model, image_scaling=SCALING, device=dev)
