"""GPU: training ray batches drawn on the device (csrc/hl_ray_batch.hip through humanliff_amd.recon_NeRF.lib.if_nerf_data_utils) against
the reference's own output (tests/golden/ray_batch.npz, with its np.random.randint draws injected) and the numpy restatement
(tests/ray_batch_restatement.py, pinned to that golden in tests/test_ray_batch_cpu.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ray_batch_restatement as rs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_batch.npz")
CASES = ["a", "b", "c", "d", "e"]
STORE_OF = {"a": ("s64", 0), "c": ("s64", 1), "e": ("s64", 2), "b": ("b", 0), "d": ("d", 0)}      # case -> (store, view in it)
MAX_ROUNDS = 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _add(store, g, name, u8=False, inst=0, layer=0):
    p = name + "_"
    img = g[p + "img_u8"] if u8 else g[p + "img_u8"].astype(np.float32) / 255.
    store.add(img[None], g[p + "body"][None], g[p + "K"][None], g[p + "R"][None], g[p + "T"][None], g[p + "bounds"], inst, layer)


@pytest.fixture(scope="module")
def stores(dev, golden):
    """Float32 stores of the golden views (a, c, e share one of 64 x 64) and a uint8 twin of the 64 x 64 one; prepared once."""
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import ViewStore
    out = {}
    for key, names, u8 in (("s64", "ace", False), ("s64_u8", "ace", True), ("b", "b", False), ("d", "d", False)):
        H, W = (int(v) for v in golden[names[0] + "_HW"])
        s = ViewStore(H, W, dev)
        for i, n in enumerate(names):
            _add(s, golden, n, u8, inst=i, layer=i + 1)
        out[key] = s.prepare()
    return out


@pytest.fixture(scope="module")
def restated(golden):
    """name -> the restatement's bound mask and classes (computed once, read only)."""
    out = {}
    for n in CASES:
        H, W = (int(v) for v in golden[n + "_HW"])
        bm = rs.bound_mask(golden[n + "_corners"], H, W)
        out[n] = (bm, *rs.classes(bm, golden[n + "_body"]))
    return out


def padded_picks(g, name, dev, max_rounds=MAX_ROUNDS):
    p = g[name + "_picks"]
    full = np.zeros((1, max_rounds, 2, p.shape[2]), dtype=np.int32)
    full[0, :p.shape[0]] = p
    return torch.from_numpy(full).to(dev)


def sample(stores, name, g, dev, store_key=None, **kw):
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import sample_ray_batch
    key, v = STORE_OF[name]
    kw.setdefault("picks", padded_picks(g, name, dev))
    kw.setdefault("max_rounds", MAX_ROUNDS)
    return sample_ray_batch(stores[store_key or key], torch.tensor([v], device=dev), int(g[name + "_n"]), **kw)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def within_one_ulp(got, want):
    """The bound of tests/test_render_gpu.py:283-288: at most one float32 ulp, fewer than 1 % of the values differing."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    ulp = np.spacing(np.abs(want).astype(np.float32))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
    print(f"max error {err.max():.1f} ulp, {100 * (got != want).mean():.1f} % of {got.size} values differ")
    assert (err <= 1).all()
    assert (got != want).mean() < 0.01


def view_rays(stores, name, g, dev, split="train"):
    """camera_rays of a golden view in the training split's arithmetic: what every sampled ray must equal bit for bit."""
    from humanliff_amd.SynBodyView_datasets import camera_rays
    p = name + "_"
    H, W = (int(v) for v in g[p + "HW"])
    return camera_rays(H, W, g[p + "K"], g[p + "R"], g[p + "T"], g[p + "bounds"], dev, split=split)


# ---- preparation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_preparation_equals_restatement(stores, golden, restated, name):
    key, v = STORE_OF[name]
    s = stores[key]
    bm, c0, c1 = restated[name]
    assert np.array_equal(bm, golden[name + "_bound_mask"])
    assert np.array_equal(s.bound_mask(v).cpu().numpy(), bm == 1)
    masks = s.class_masks(v).cpu().numpy()
    assert np.array_equal(masks[0], c0) and np.array_equal(masks[1], c1)
    assert np.array_equal(rs.unpack_bits(s.bitmaps[v].cpu().numpy(), s.W), np.stack([c0, c1]))
    assert s.class_counts()[v].tolist() == [int(c0.sum()), int(c1.sum())]
    table = s.row_table[v].cpu().numpy()
    for c, m in enumerate((c0, c1)):
        assert np.array_equal(table[c], np.concatenate([[0], np.cumsum(m.sum(axis=1))]))


def test_empty_class_raises(dev, golden):
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import ViewStore
    g = golden
    for body in (np.ones_like(g["c_body"]), np.zeros_like(g["c_body"])):                  # no background pixel / no body pixel
        s = ViewStore(64, 64, dev)
        s.add(g["c_img_u8"][None], body[None], g["c_K"][None], g["c_R"][None], g["c_T"][None], g["c_bounds"], 0, 0)
        with pytest.raises(ValueError):
            s.prepare()


def test_select_is_argwhere_order(stores, golden, restated, dev):
    """Case d (a row spans two words, nothing is rejected): picks 0 .. count - 1 return the class's pixels in np.argwhere order."""
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import sample_ray_batch
    _, c0, c1 = restated["d"]
    for c, m, ratio in ((0, c0, 1.0), (1, c1, 0.0)):
        want = np.argwhere(m)
        n = len(want)
        assert c == 0 or ((want[:, 1] >= 64).any() and (want[:, 1] < 64).any())      # the background class has pixels in both words of a row
        picks = torch.zeros((1, 1, 2, n), dtype=torch.int32, device=dev)
        picks[0, 0, c] = torch.arange(n, dtype=torch.int32, device=dev)
        out = host(sample_ray_batch(stores["d"], torch.tensor([0], device=dev), n, ratio=ratio, picks=picks, max_rounds=1))
        assert out["n_valid"].tolist() == [n]
        assert np.array_equal(out["coord"][0, 0], want)
        assert (out["bkgd_msk"] == (1 - c)).all()


# ---- injected picks against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_injected_picks_match_reference_golden(stores, golden, dev, name):
    """coord, bkgd_msk, n_valid, the row order and rgb equal the reference's exactly; ray_o / ray_d within the 1-ulp / 1 % bound; every
    ray, near, far and mask_at_box bit-equal to camera_rays(..., split='train') at coord, and the rays also to the default camera_rays
    (whose near / far are the reference's test-split values: a few ulp away)."""
    g, p = golden, name + "_"
    n = int(g[p + "n"])
    out = sample(stores, name, g, dev)
    for k, shape in (("rgb", (1, 1, n, 3)), ("ray_o", (1, 1, n, 3)), ("ray_d", (1, 1, n, 3)), ("near", (1, 1, n, 1)), ("far", (1, 1, n, 1)),
                     ("bkgd_msk", (1, 1, n, 1)), ("mask_at_box", (1, 1, n)), ("coord", (1, 1, n, 2)), ("n_valid", (1,))):
        assert tuple(out[k].shape) == shape
        assert out[k].dtype == {"mask_at_box": torch.bool, "coord": torch.int32, "n_valid": torch.int32}.get(k, torch.float32)
    ro, rd, near, far, mask = view_rays(stores, name, g, dev)
    W = int(g[p + "HW"][1])
    flat = (out["coord"][0, 0, :, 0].long() * W + out["coord"][0, 0, :, 1].long())
    assert torch.equal(out["ray_o"][0, 0], ro[flat]) and torch.equal(out["ray_d"][0, 0], rd[flat])
    assert torch.equal(out["near"][0, 0, :, 0], near[flat]) and torch.equal(out["far"][0, 0, :, 0], far[flat])
    assert torch.equal(out["mask_at_box"][0, 0], mask[flat]) and bool(mask[flat].all())
    ro_t, rd_t, _, _, mask_t = view_rays(stores, name, g, dev, split="test")
    assert torch.equal(ro, ro_t) and torch.equal(rd, rd_t) and torch.equal(mask, mask_t)
    h = host(out)
    assert h["n_valid"].tolist() == [n]
    assert np.array_equal(h["coord"][0, 0], g[p + "coord"])
    assert np.array_equal(h["bkgd_msk"][0, 0], g[p + "bkgd_msk"].astype(np.float32))
    assert np.array_equal(h["mask_at_box"][0, 0], g[p + "mask_at_box"])
    assert np.array_equal(h["rgb"][0, 0], g[p + "rgb"])
    within_one_ulp(h["ray_o"][0, 0], g[p + "ray_o"])
    within_one_ulp(h["ray_d"][0, 0], g[p + "ray_d"])


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_injected_picks_near_far_match_reference_golden(stores, golden, dev, name):
    """near and far against the reference's training split within the 1-ulp / 1 % bound: the kernel runs get_near_far on the float64
    rays and rounds afterwards, as if_nerf_data_utils.py:146-149, 163-167 does.  (The values of the default camera_rays - the reference's
    test split, which rounds the rays first - differ from these in 51 - 81 % of the entries by up to 3 ulp.)"""
    g, p = golden, name + "_"
    h = host(sample(stores, name, g, dev))
    within_one_ulp(h["near"][0, 0, :, 0], g[p + "near"])
    within_one_ulp(h["far"][0, 0, :, 0], g[p + "far"])


@pytest.mark.parametrize("name", ["a", "d", "e"])
def test_camera_rays_train_split_matches_restatement(stores, golden, dev, name):
    """camera_rays(..., split='train') over the whole view against the float64 restatement of get_rays / get_near_far as the training
    split calls them (rays that miss: near 0, far 1); the default split gives the same rays and hit mask."""
    g, p = golden, name + "_"
    H, W = (int(v) for v in g[p + "HW"])
    o64, d64 = rs.get_rays(H, W, g[p + "K"], g[p + "R"], g[p + "T"])
    o64, d64 = o64.reshape(-1, 3).copy(), d64.reshape(-1, 3).copy()
    near, far, hit = rs.get_near_far(g[p + "bounds"], o64, d64)
    want_near, want_far = np.zeros(H * W, dtype=np.float32), np.ones(H * W, dtype=np.float32)
    want_near[hit], want_far[hit] = near.astype(np.float32), far.astype(np.float32)
    ro, rd, gn, gf, mask = (t.cpu().numpy() for t in view_rays(stores, name, g, dev))
    assert np.array_equal(mask, hit) and 0 < hit.sum() < hit.size
    within_one_ulp(ro, o64.astype(np.float32))
    within_one_ulp(rd, d64.astype(np.float32))
    within_one_ulp(gn, want_near)
    within_one_ulp(gf, want_far)


def test_batch_entries_equal_single_calls(stores, golden, dev):
    """bs = 3 over the 64 x 64 store with one view repeated: every entry is its own single-entry call."""
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import sample_ray_batch
    g = golden
    names = ["a", "c", "a"]
    n = 256
    picks = torch.cat([padded_picks(g, nm, dev) for nm in names])
    picks[2] = (picks[2].flip(-1) + 7) % 1000                                 # the repeated view with other draws (1000 < both class counts)
    idx = torch.tensor([STORE_OF[nm][1] for nm in names], device=dev)
    out = sample_ray_batch(stores["s64"], idx, n, picks=picks, max_rounds=MAX_ROUNDS)
    assert out["n_valid"][:2].tolist() == [n, n] and int(out["n_valid"][2]) > 0
    assert not torch.equal(out["coord"][0], out["coord"][2])
    for b in range(3):
        one = sample_ray_batch(stores["s64"], idx[b:b + 1], n, picks=picks[b:b + 1].contiguous(), max_rounds=MAX_ROUNDS)
        for k in one:
            assert torch.equal(one[k][0], out[k][b]), k


def test_uint8_store(stores, golden, dev):
    """rgb of a uint8 store is np.float32(u8) / np.float32(255), bit for bit; everything else equals the float32 store's."""
    g = golden
    f = sample(stores, "a", g, dev)
    u = sample(stores, "a", g, dev, store_key="s64_u8")
    coord = u["coord"][0, 0].cpu().numpy()
    want = g["a_img_u8"][coord[:, 0], coord[:, 1]].astype(np.float32) / np.float32(255)
    assert np.array_equal(u["rgb"][0, 0].cpu().numpy(), want)
    for k in f:
        assert torch.equal(f[k], u[k]), k


def test_round_cap(stores, golden, restated, dev):
    """Case a, every pick pointing at the rejected column, max_rounds = 2: nothing is kept, the rows are zeros with near 0 / far 1."""
    g = golden
    _, c0, c1 = restated["a"]
    *_, mask = view_rays(stores, "a", g, dev)
    hit = mask.cpu().numpy().reshape(64, 64)
    ranks = []
    for m in (c0, c1):
        rejected = np.flatnonzero(~hit[m])                                 # ranks, in argwhere order, of the class's rejected pixels
        assert len(rejected) > 0
        ranks.append(int(rejected[len(rejected) // 2]))
    picks = torch.zeros((1, 2, 2, 256), dtype=torch.int32, device=dev)
    picks[:, :, 0], picks[:, :, 1] = ranks[0], ranks[1]
    out = sample(stores, "a", g, dev, picks=picks, max_rounds=2)
    assert out["n_valid"].tolist() == [0]
    for k in ("rgb", "ray_o", "ray_d", "near", "bkgd_msk", "coord", "mask_at_box"):
        assert not out[k].any(), k
    assert bool((out["far"] == 1).all())


def test_pick_out_of_range_is_flagged(stores, golden, dev):
    g = golden
    picks = padded_picks(g, "c", dev)
    picks[0, 0, 0, 5] = int(stores["s64"].class_counts()[1, 0])            # one past the last body pixel
    assert sample(stores, "c", g, dev, picks=picks)["n_valid"].tolist() == [-1]


# ---- the kernel's own generator ---------------------------------------------------------------------------------------------------
def test_own_generator(stores, golden, restated, dev):
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import sample_ray_batch
    g = golden
    s = stores["s64"]
    idx = torch.tensor([0, 1, 2], device=dev)                              # a (rejections), c, e
    n = 256
    one = sample_ray_batch(s, idx, n, seed=7, step=3)
    again = sample_ray_batch(s, idx, n, seed=7, step=3)
    nxt = sample_ray_batch(s, idx, n, seed=7, step=4)
    other = sample_ray_batch(s, idx, n, seed=8, step=3)
    for k in one:
        assert torch.equal(one[k], again[k]), k
    assert not torch.equal(one["coord"], nxt["coord"]) and not torch.equal(one["coord"], other["coord"])
    assert not torch.equal(one["coord"][0], one["coord"][1])               # entries draw from different counters
    assert one["n_valid"].tolist() == [n, n, n]
    h = host(one)
    for b, name in enumerate("ace"):
        _, c0, c1 = restated[name]
        ro, rd, near, far, mask = (t.cpu().numpy() for t in view_rays(stores, name, g, dev))
        y, x = h["coord"][b, 0, :, 0], h["coord"][b, 0, :, 1]
        body = h["bkgd_msk"][b, 0, :, 0] == 1
        assert c0[y[body], x[body]].all() and c1[y[~body], x[~body]].all()
        img = g[name + "_img_u8"].astype(np.float32) / np.float32(255)
        assert np.array_equal(h["rgb"][b, 0], img[y, x])
        flat = y * 64 + x
        assert np.array_equal(h["ray_o"][b, 0], ro[flat]) and np.array_equal(h["ray_d"][b, 0], rd[flat])
        assert np.array_equal(h["near"][b, 0, :, 0], near[flat]) and np.array_equal(h["far"][b, 0, :, 0], far[flat]) and mask[flat].all()
    body_c = h["bkgd_msk"][1, 0, :, 0]                                       # case c: one round, nothing rejected
    assert body_c[:int(n * 0.8)].all() and not body_c[int(n * 0.8):].any()


def test_own_generator_is_uniform(stores, restated, dev):
    """16 384 body picks on case c (int(20480 * 0.8) rows, all kept) over 16 equal rank bins: each within 6 standard deviations of
    1024 (sigma = sqrt(16384 * (1 / 16) * (15 / 16)) = 30.98, so +-186).  The seed is fixed: deterministic."""
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import sample_ray_batch
    _, c0, _ = restated["c"]
    out = sample_ray_batch(stores["s64"], torch.tensor([1], device=dev), 20480, seed=11, step=0)
    assert out["n_valid"].tolist() == [20480]
    coord = out["coord"][0, 0, :16384].cpu().numpy()
    assert (out["bkgd_msk"][0, 0, :16384] == 1).all() and not out["bkgd_msk"][0, 0, 16384:].any()
    rank_of = np.full(c0.shape, -1, dtype=np.int64)
    rank_of[c0] = np.arange(int(c0.sum()))
    ranks = rank_of[coord[:, 0], coord[:, 1]]
    assert (ranks >= 0).all()
    bins = np.bincount(ranks * 16 // int(c0.sum()), minlength=16)
    print("bins", bins.tolist())
    assert (np.abs(bins - 1024) <= 186).all()


# ---- FitLoop on a RayBatchLoader ----------------------------------------------------------------------------------------------------
def test_fit_loop_on_loader(dev):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.recon_NeRF import Renderer
    from humanliff_amd.recon_NeRF.fit import FitLoop
    from humanliff_amd.recon_NeRF.lib.if_nerf_data_utils import RayBatchLoader, ViewStore
    H = W = 64
    rng = np.random.RandomState(2)
    yy, xx = np.mgrid[0:H, 0:W]
    body = (((xx - 32) / 14.0) ** 2 + ((yy - 32) / 23.0) ** 2 <= 1.0).astype(np.uint8)
    store = ViewStore(H, W, dev)
    for v in range(4):
        K, c2w, cam = syn.orbit_camera(2 * v, 8, H, W)
        R = c2w.T.copy()
        store.add(rng.randint(0, 256, (1, H, W, 3)).astype(np.uint8), body[None], K[None], R[None], (-R @ cam)[None], syn.WORLD_BOUNDS,
                  [v % 3], [v])
    store.prepare()
    torch.manual_seed(0)
    base = Renderer(use_canonical_space=False, num_instances=3, triplane_dim=64, triplane_ch=27, test=False)
    base.load_state_dict(syn.render_mlp_state(3), strict=False)
    base = base.to(dev)

    def run():
        model = copy.deepcopy(base)
        loader = RayBatchLoader(store, batch_size=2, n_rays=256, seed=5)
        assert len(loader) == 2
        loop = FitLoop(model, loader, lrate=5e-4, tri_plane_lrate=1e-2, lrate_decay=10, tv_loss_coef=1e-2, l1_loss_coef=5e-4, use_clamp=True,
                       n_samples=32, n_importance=32)
        torch.manual_seed(1)
        losses, seen = [], []
        while len(losses) < 6:
            for tp in loader:
                if not losses:
                    for k, shape, dt in (("rgb_all", (2, 1, 256, 3), torch.float32), ("ray_o_all", (2, 1, 256, 3), torch.float32),
                                         ("ray_d_all", (2, 1, 256, 3), torch.float32), ("near_all", (2, 1, 256, 1), torch.float32),
                                         ("far_all", (2, 1, 256, 1), torch.float32), ("bkgd_msk_all", (2, 1, 256, 1), torch.float32),
                                         ("instance_idx", (2,), torch.int64), ("cloth_layer_index", (2,), torch.int64),
                                         ("world_bounds", (2, 2, 3), torch.float32)):
                        assert tuple(tp[k].shape) == shape and tp[k].dtype == dt and tp[k].device == dev, k
                seen.append(tp["image_idx"].tolist())
                assert tp["instance_idx"].tolist() == [v % 3 for v in seen[-1]] and tp["cloth_layer_index"].tolist() == seen[-1]
                losses.append(torch.stack(loop.step(tp)))
        assert sorted(seen[0] + seen[1]) == [0, 1, 2, 3] and sorted(seen[2] + seen[3]) == [0, 1, 2, 3]
        return torch.stack(losses), model.tri_planes.detach().clone()

    l1, p1 = run()
    l2, p2 = run()
    assert l1.shape == (6, 5) and bool(torch.isfinite(l1).all())
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
    assert not torch.equal(p1, base.tri_planes.detach())
