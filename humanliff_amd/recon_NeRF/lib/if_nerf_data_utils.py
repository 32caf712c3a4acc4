"""Training ray batches drawn on the device from resident views: sample_ray_batch of recon_NeRF/lib/if_nerf_data_utils.py (:87-190)
without its per-call host work (csrc/hl_ray_batch.hip; contract: DESIGN.md 4g).

    store = ViewStore(H, W, device)
    store.add(images, body, K, R, T, bounds, instance_idx, cloth_layer_index)      # V views at a time; uint8 or float32 images
    store.prepare()                                                                # once: bound masks, pixel classes, camera table
    loader = RayBatchLoader(store, batch_size=2, n_rays=2048, seed=0)
    FitLoop(renderer, loader, ...).run_loop()

The reference runs this in a DataLoader worker per item: float64 rays for the whole image, cv2.fillPoly, np.argwhere twice, a
rejection loop.  Here the views stay in HBM, everything that depends on the view alone is computed once by prepare(), and a batch is one
launch with no host work and no upload.  SynBody_dataset.load_view_store fills a store from a dataset on disk.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from ... import _lib
from ...SynBodyView_datasets import camera_rays

CORNER_LIMIT = 1 << 30      # |projected corner| the integer fill accepts (csrc/hl_ray_batch.hip: products stay inside int64)


def bound_corners_2d(bounds, K, R, T):
    """np.round(project(get_bound_corners(bounds), K, [R|T])).astype(int) of get_bound_2d_mask (:20-39, 192-201): the 8 corners of
    the bounds as integer pixel coordinates (x, y), (8, 2) int64.  Host, numpy float64, the reference's expressions."""
    bounds = np.asarray(bounds, dtype=np.float64)
    min_x, min_y, min_z = bounds[0]
    max_x, max_y, max_z = bounds[1]
    corners_3d = np.array([
        [min_x, min_y, min_z],
        [min_x, min_y, max_z],
        [min_x, max_y, min_z],
        [min_x, max_y, max_z],
        [max_x, min_y, min_z],
        [max_x, min_y, max_z],
        [max_x, max_y, min_z],
        [max_x, max_y, max_z],
    ])
    RT = np.concatenate([np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(T, dtype=np.float64).reshape(3, 1)], axis=1)
    xyz = np.dot(corners_3d, RT[:, :3].T) + RT[:, 3:].T
    xyz = np.dot(xyz, np.asarray(K, dtype=np.float64).T)
    with np.errstate(all="ignore"):
        xy = np.round(xyz[:, :2] / xyz[:, 2:])
    if not np.isfinite(xy).all() or np.abs(xy).max() >= CORNER_LIMIT:
        raise ValueError("bound_corners_2d: a corner of the bounds projects to infinity or beyond 2^30 pixels (it lies on the camera plane)")
    return xy.astype(np.int64)


def _camera_row(K, R, T, bounds):
    f64 = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))  # noqa: E731
    Ki, Rm, Tm, Bm = f64(np.linalg.inv(np.asarray(K, dtype=np.float64)), (3, 3)), f64(R, (3, 3)), f64(T, (3,)), f64(bounds, (2, 3))
    row = np.empty(30, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().hl_camera_table_row(p(Ki), p(Rm), p(Tm), p(Bm), p(row)), "hl_camera_table_row")
    return row


def _void(t):
    return C.c_void_p(t.data_ptr())


class ViewStore:
    """Views of one size resident on the device, with what sample_ray_batch derives from a view alone.

    add() takes V views: images (V, H, W, 3) uint8 or float32 (one dtype per store; a float image is what the reference has after
    imread / 255), body (V, H, W) non-zero where the reference's msk == 1, K (V, 3, 3), R (V, 3, 3), T (V, 3[, 1]), bounds (V, 2, 3)
    or (2, 3), instance_idx and cloth_layer_index (V,) or scalars.  Tensors or arrays; images and body that are already device
    tensors are not copied through the host.  prepare() must follow the last add()."""

    def __init__(self, H, W, device=None):
        if int(H) <= 0 or int(W) <= 0:
            raise ValueError(f"ViewStore: bad image size {H} x {W}")
        self.H, self.W = int(H), int(W)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ViewStore needs a HIP device; humanliff_amd has no CPU path")
        _lib.lib()
        self._images, self._body, self._cams, self._corners, self._bounds, self._inst, self._layer = [], [], [], [], [], [], []
        self._K, self._R, self._T = [], [], []
        self.images = self.body = self.bitmaps = self.row_table = self.cameras = None

    def __len__(self):
        return sum(t.shape[0] for t in self._images) if self.images is None else self.images.shape[0]

    def add(self, images, body, K, R, T, bounds, instance_idx, cloth_layer_index):
        H, W = self.H, self.W
        images, body = torch.as_tensor(images), torch.as_tensor(body)
        if images.dim() == 3:
            images, body = images[None], body[None]
        V = images.shape[0]
        if tuple(images.shape) != (V, H, W, 3) or tuple(body.shape) != (V, H, W):
            raise ValueError(f"ViewStore.add: images must be (V, {H}, {W}, 3) and body (V, {H}, {W}); got {tuple(images.shape)}, {tuple(body.shape)}")
        if images.dtype not in (torch.uint8, torch.float32) or (self._images and images.dtype != self._images[0].dtype):
            raise TypeError("ViewStore.add: images must be uint8 or float32, one dtype per store")
        K = np.asarray(K, dtype=np.float64).reshape(V, 3, 3)
        R = np.asarray(R, dtype=np.float64).reshape(V, 3, 3)
        T = np.asarray(T, dtype=np.float64).reshape(V, 3)
        bounds = np.broadcast_to(np.asarray(bounds, dtype=np.float64), (V, 2, 3))
        for v in range(V):
            self._corners.append(bound_corners_2d(bounds[v], K[v], R[v], T[v]))
            self._cams.append(_camera_row(K[v], R[v], T[v], bounds[v]))
        self._K.append(K), self._R.append(R), self._T.append(T), self._bounds.append(bounds.copy())
        self._images.append(images.to(self.device).contiguous())
        self._body.append((body != 0).to(self.device, torch.uint8).contiguous())
        self._inst.append(np.broadcast_to(np.asarray(instance_idx, dtype=np.int64), (V,)).copy())
        self._layer.append(np.broadcast_to(np.asarray(cloth_layer_index, dtype=np.int64), (V,)).copy())
        self.images = None
        return self

    def prepare(self):
        """Upload the tables and compute every view's pixel classes (hl_ray_views_prepare).  Reads the class totals back once:
        ValueError for a view with an empty class, as np.random.randint(0, 0, n) raises in the reference."""
        if not self._images:
            raise ValueError("ViewStore.prepare: no views")
        dev, H, W = self.device, self.H, self.W
        self.images, self.body = torch.cat(self._images), torch.cat(self._body)
        self._images, self._body = [self.images], [self.body]
        V = self.images.shape[0]
        self.K, self.R, self.T = np.concatenate(self._K), np.concatenate(self._R), np.concatenate(self._T)
        self.bounds = np.concatenate(self._bounds)
        self.corners = torch.from_numpy(np.stack(self._corners).astype(np.int32)).to(dev)
        self.cameras = torch.from_numpy(np.stack(self._cams)).to(dev)
        self.world_bounds = torch.from_numpy(self.bounds.astype(np.float32)).to(dev)
        self.instance_idx = torch.from_numpy(np.concatenate(self._inst)).to(dev)
        self.cloth_layer_index = torch.from_numpy(np.concatenate(self._layer)).to(dev)
        nw = (W + 63) // 64
        self.bitmaps = torch.empty((V, 2, H, nw), dtype=torch.int64, device=dev)          # (the bits of uint64 words)
        self.row_table = torch.empty((V, 2, H + 1), dtype=torch.int32, device=dev)
        with _lib.on(dev):
            _lib.check(_lib.lib().hl_ray_views_prepare(_void(self.corners), _void(self.body), V, H, W, _void(self.bitmaps),
                                                       _void(self.row_table), _lib.stream_ptr(dev)), "hl_ray_views_prepare")
        counts = self.class_counts().cpu().numpy()
        empty = np.argwhere(counts == 0)
        if len(empty):
            v, c = (int(i) for i in empty[0])
            raise ValueError(f"ViewStore.prepare: view {v} has no pixel of class {c} ({'bound & body' if c == 0 else 'bound & ~body'}): "
                             "sample_ray_batch cannot draw from it (np.random.randint: low >= high)")
        return self

    def _ready(self):
        if self.images is None or self.bitmaps is None:
            raise RuntimeError("ViewStore: call prepare() after the last add()")

    def class_counts(self):
        """(V, 2) int32 device tensor: pixels of class 0 (bound & body) and class 1 (bound & ~body) per view."""
        if self.row_table is None:
            raise RuntimeError("ViewStore: call prepare() after the last add()")
        return self.row_table[:, :, self.H]

    def class_masks(self, v):
        """(2, H, W) bool device tensor: the two class bitmaps of view v, unpacked."""
        self._ready()
        bits = (self.bitmaps[v][..., None] >> torch.arange(64, device=self.device)) & 1
        return bits.reshape(2, self.H, -1)[:, :, :self.W].bool()

    def bound_mask(self, v):
        """get_bound_2d_mask of view v: (H, W) bool device tensor (the union of its two classes)."""
        m = self.class_masks(v)
        return m[0] | m[1]

    def test_view(self, v):
        """The split != 'train' tuple of sample_ray_batch (:172-190) for view v, on the device:
        rgb (H*W, 3) float32 with the pixels outside bound_mask zeroed, ray_o, ray_d (H*W, 3), near, far (H*W), coord (H*W, 2) int64
        zeros, mask_at_box (H*W) bool, bkgd_msk (H, W) ones - the ground truth evaluate_views scores against."""
        self._ready()
        H, W = self.H, self.W
        img = self.images[v]
        img = img.float() / 255.0 if img.dtype == torch.uint8 else img
        rgb = torch.where(self.bound_mask(v)[..., None], img, torch.zeros_like(img)).reshape(-1, 3)
        ray_o, ray_d, near, far, mask_at_box = camera_rays(H, W, self.K[v], self.R[v], self.T[v], self.bounds[v], self.device)
        coord = torch.zeros((H * W, 2), dtype=torch.int64, device=self.device)
        return rgb, ray_o, ray_d, near, far, coord, mask_at_box, torch.ones_like(self.body[v])


def sample_ray_batch(store, image_idx, n_rays, ratio=0.8, picks=None, seed=0, step=0, max_rounds=32):
    """One training batch: entry b samples n_rays rays of view image_idx[b] as the split == 'train' loop of the reference does
    (:102-170): in every round int(missing * ratio) pixels of class 0 (body) and the rest of class 1, kept when their ray crosses the
    0.01-padded bounds exactly twice, until n_rays are kept or max_rounds rounds are done.  image_idx: (bs,) int64 device tensor (or
    anything torch.as_tensor takes).  picks (bs, max_rounds, 2, n_rays) int32 device tensor injects the reference's
    np.random.randint draws (round, class, slot); without it they come from a counter-based generator keyed by (seed, step).
    Enqueue-only.  Returns device tensors
        rgb, ray_o, ray_d (bs, 1, n, 3), near, far, bkgd_msk (bs, 1, n, 1) float32, mask_at_box (bs, 1, n) bool,
        coord (bs, 1, n, 2) int32 (y, x), n_valid (bs,) int32
    rows from n_valid[b] on are zeros with near 0 / far 1; n_valid[b] is -1 for an image_idx or a pick out of range."""
    store._ready()
    dev, H, W = store.device, store.H, store.W
    image_idx = torch.as_tensor(image_idx, dtype=torch.int64).to(dev).reshape(-1).contiguous()
    bs, n = image_idx.shape[0], int(n_rays)
    if bs < 1 or n < 1 or int(max_rounds) < 1:
        raise ValueError(f"sample_ray_batch: bad sizes (bs {bs}, n_rays {n}, max_rounds {max_rounds})")
    if picks is not None:
        if not torch.is_tensor(picks) or picks.device != dev or picks.dtype != torch.int32 or tuple(picks.shape) != (bs, max_rounds, 2, n) \
                or not picks.is_contiguous():
            raise ValueError(f"sample_ray_batch: picks must be a contiguous int32 device tensor of shape {(bs, max_rounds, 2, n)}")
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"rgb": f(bs, 1, n, 3), "ray_o": f(bs, 1, n, 3), "ray_d": f(bs, 1, n, 3), "near": f(bs, 1, n, 1), "far": f(bs, 1, n, 1),
           "bkgd_msk": f(bs, 1, n, 1), "mask_at_box": torch.empty((bs, 1, n), dtype=torch.uint8, device=dev),
           "coord": torch.empty((bs, 1, n, 2), dtype=torch.int32, device=dev), "n_valid": torch.empty((bs,), dtype=torch.int32, device=dev)}
    with _lib.on(dev):
        _lib.check(_lib.lib().hl_ray_batch(_void(image_idx), bs, _void(store.images), 1 if store.images.dtype == torch.uint8 else 0,
                                           _void(store.bitmaps), _void(store.row_table), _void(store.cameras), store.images.shape[0], H, W,
                                           n, float(ratio), None if picks is None else _void(picks), int(seed) & (2 ** 64 - 1),
                                           int(step) & (2 ** 64 - 1), int(max_rounds), *(_void(out[k]) for k in
                                           ("rgb", "ray_o", "ray_d", "near", "far", "bkgd_msk", "mask_at_box", "coord", "n_valid")),
                                           _lib.stream_ptr(dev)), "hl_ray_batch")
    out["mask_at_box"] = out["mask_at_box"].view(torch.bool)
    return out


def epoch_order(n, seed, epoch):
    """The order in which epoch `epoch` visits n stored views: a permutation from a torch.Generator seeded by (seed, epoch).  Host."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch)) & (2 ** 63 - 1))
    return torch.randperm(int(n), generator=g)


class RayBatchLoader:
    """The `data` iterable of FitLoop over a prepared ViewStore: one pass is one epoch, the views in epoch_order taken in groups of
    batch_size (a last smaller group is dropped; a store smaller than batch_size is an error).  Every batch is one hl_ray_batch launch
    with the loader's own step counter as the generator's `step`, so a run is reproducible from `seed`.  Yields tp_input with the keys
    FitLoop.step reads: rgb_all, ray_o_all, ray_d_all, near_all, far_all, bkgd_msk_all, mask_at_box_all, instance_idx,
    cloth_layer_index (int64 device tensors), world_bounds (bs, 2, 3)."""

    def __init__(self, store, batch_size, n_rays, seed=0, ratio=0.8, max_rounds=32):
        store._ready()
        if not 1 <= int(batch_size) <= len(store):
            raise ValueError(f"RayBatchLoader: batch_size {batch_size} with {len(store)} stored views")
        self.store, self.batch_size, self.n_rays, self.seed, self.ratio, self.max_rounds = store, int(batch_size), int(n_rays), int(seed), ratio, max_rounds
        self.epoch, self.step = 0, 0

    def __len__(self):
        return len(self.store) // self.batch_size

    def __iter__(self):
        s, bs = self.store, self.batch_size
        order = epoch_order(len(s), self.seed, self.epoch).to(s.device, non_blocking=True)
        self.epoch += 1
        for i in range(len(self)):
            idx = order[i * bs:(i + 1) * bs]
            b = sample_ray_batch(s, idx, self.n_rays, self.ratio, None, self.seed, self.step, self.max_rounds)
            self.step += 1
            yield {"rgb_all": b["rgb"], "ray_o_all": b["ray_o"], "ray_d_all": b["ray_d"], "near_all": b["near"], "far_all": b["far"],
                   "bkgd_msk_all": b["bkgd_msk"], "mask_at_box_all": b["mask_at_box"], "n_valid": b["n_valid"], "image_idx": idx,
                   "instance_idx": s.instance_idx[idx], "cloth_layer_index": s.cloth_layer_index[idx], "world_bounds": s.world_bounds[idx]}
