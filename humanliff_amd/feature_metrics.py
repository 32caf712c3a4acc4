"""Metrics on two sets of Inception features beyond the Frechet distance: the Kernel Inception Distance (an unbiased cubic-kernel
MMD^2, defined at any set size), improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) -
hl_feat (csrc/hl_feature_metrics.hip; contract: DESIGN.md 4m "Feature metrics").  All of them are functions of the pairwise structure
of the two sets, formed in float64 on the device with a Gram entry that depends on the two rows' contents alone.  There is no CPU path.

The subset rule of kernel_inception_distance is torch-fidelity's as recalled; it has not been verified against the package
(DESIGN.md 4m)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_K = 8
_KINDS = {"gram": 0, "d2": 1}
_OP_PAIRWISE, _OP_KID, _OP_KNN, _OP_MANIFOLD = 0, 1, 2, 3


def _features(t, what, device=None):
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"{what} must be (n, D) float32 with n, D >= 1, got {(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a HIP tensor; humanliff_amd has no CPU path")
    if device is not None and t.device != device:
        raise RuntimeError(f"{what} is on {t.device}, the other set on {device}")
    return t.contiguous()


def _pair(x, y, name):
    x = _features(x, f"{name}: x")
    y = _features(y, f"{name}: y", x.device)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"{name}: the sets have {x.shape[1]} and {y.shape[1]} dimensions")
    return x, y


def _workspace(op, n, m, s, sub, split, device, name):
    nbytes = _lib.lib().hl_feat_workspace_bytes(op, n, m, s, sub, split)
    if nbytes == 0:
        raise ValueError(f"{name}: sizes outside what the library serves (N {n}, M {m}, subsets {s} of {sub})")
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def pairwise(x, y, kind="d2"):
    """(N, M) float64: kind "gram": g(x_i, y_j) = sum_k x_ik y_jk; "d2": max(0, g(x_i,x_i) + g(y_j,y_j) - 2 g(x_i,y_j)).  For small sets and tests."""
    if kind not in _KINDS:
        raise ValueError(f"pairwise: kind must be 'd2' or 'gram', got {kind!r}")
    x, y = _pair(x, y, "pairwise")
    n, m, d = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(_OP_PAIRWISE, n, m, 0, 0, 0, x.device, "pairwise")
    out = torch.empty((n, m), dtype=torch.float64, device=x.device)
    with _lib.on(x.device):
        _lib.check(_lib.lib().hl_feat_pairwise(_lib.ptr(x), n, _lib.ptr(y), m, d, _KINDS[kind], _vp(out), _vp(ws), ws.numel() * 8, _lib.stream_ptr(x.device)),
                   "hl_feat_pairwise")
    return out


def subset_indices(n, m, subsets, subset_size, seed=2020):
    """The two (subsets, subset_size) int32 index tables: rng = RandomState(seed); per subset, rng.choice(n, size, replace=False) for x, then
    rng.choice(m, size, replace=False) for y."""
    subsets, subset_size = int(subsets), int(subset_size)
    if subset_size < 2 or subset_size > min(n, m):
        raise ValueError(f"kernel_inception_distance: subset_size {subset_size} must be in 2 .. min(N, M) = {min(n, m)}")
    if subsets < 1:
        raise ValueError(f"kernel_inception_distance: subsets {subsets} must be at least 1")
    rng = np.random.RandomState(seed)
    xi, yi = np.empty((subsets, subset_size), dtype=np.int32), np.empty((subsets, subset_size), dtype=np.int32)
    for s in range(subsets):
        xi[s] = rng.choice(n, subset_size, replace=False)
        yi[s] = rng.choice(m, subset_size, replace=False)
    return xi, yi


def kid_subsets(x, y, x_index, y_index):
    """(S,) float64 on the device: the unbiased MMD^2 of the cubic kernel (gamma = 1 / D, coef0 = 1) per subset; x_index, y_index (S, m) rows of x, y."""
    x, y = _pair(x, y, "kernel_inception_distance")
    xi, yi = (np.ascontiguousarray(np.asarray(t), dtype=np.int32) for t in (x_index, y_index))
    if xi.ndim != 2 or xi.shape != yi.shape:
        raise ValueError(f"kernel_inception_distance: index tables {xi.shape} and {yi.shape} must be one (S, m) shape")
    n, m, d = x.shape[0], y.shape[0], x.shape[1]
    s, sub = xi.shape
    if sub < 2 or sub > min(n, m) or s < 1:
        raise ValueError(f"kernel_inception_distance: {s} subsets of {sub}; the size must be in 2 .. min(N, M) = {min(n, m)}")
    if xi.min() < 0 or xi.max() >= n or yi.min() < 0 or yi.max() >= m:
        raise ValueError("kernel_inception_distance: an index lies outside its set")
    dxi, dyi = torch.from_numpy(xi).to(x.device), torch.from_numpy(yi).to(x.device)
    ws = _workspace(_OP_KID, n, m, s, sub, 0, x.device, "kernel_inception_distance")
    out = torch.empty(s, dtype=torch.float64, device=x.device)
    with _lib.on(x.device):
        _lib.check(_lib.lib().hl_feat_kid(_lib.ptr(x), n, _lib.ptr(y), m, d, _vp(dxi), _vp(dyi), s, sub, _vp(out), _vp(ws), ws.numel() * 8,
                                          _lib.stream_ptr(x.device)), "hl_feat_kid")
    return out


def kernel_inception_distance(x, y, subsets=100, subset_size=1000, seed=2020):
    """(mean, std, per_subset): KID over `subsets` random subsets of `subset_size` rows of each set (subset_indices); per_subset (S,) float64
    on the device, mean = np.mean and std = np.std of it in float64 on the host after one read-back."""
    x, y = _pair(x, y, "kernel_inception_distance")
    xi, yi = subset_indices(x.shape[0], y.shape[0], subsets, subset_size, seed)
    per = kid_subsets(x, y, xi, yi)
    host = per.cpu().numpy()
    return float(np.mean(host)), float(np.std(host)), per


def _split_of(rows, cols, split):
    return _lib.lib().hl_feat_split(rows, cols, int(split))


def knn_radii(x, k=3, _split=0):
    """(N,) float64: the k-th smallest d2 of every row to the other rows of the set (the row's own index is left out; a duplicate stays, at 0)."""
    x = _features(x, "knn_radii: x")
    n, d = x.shape
    if not 1 <= k <= MAX_K or k >= n:
        raise ValueError(f"knn_radii: k = {k}; 1 <= k <= {MAX_K} and k < N = {n}")
    ws = _workspace(_OP_KNN, n, n, 0, 0, int(_split), x.device, "knn_radii")
    r2 = torch.empty(n, dtype=torch.float64, device=x.device)
    with _lib.on(x.device):
        _lib.check(_lib.lib().hl_feat_knn_radii(_lib.ptr(x), n, d, int(k), int(_split), _vp(r2), _vp(ws), ws.numel() * 8, _lib.stream_ptr(x.device)),
                   "hl_feat_knn_radii")
    return r2


def manifold(real, fake, r2_real, r2_fake, _split=0):
    """One pass over the real x fake distances: (hits_fake (M,) int32, hits_real (N,) int32, nearest_real (N,) float64)."""
    real, fake = _pair(real, fake, "manifold")
    n, m, d = real.shape[0], fake.shape[0], real.shape[1]
    for t, cnt, what in ((r2_real, n, "r2_real"), (r2_fake, m, "r2_fake")):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != (cnt,) or t.device != real.device:
            raise RuntimeError(f"manifold: {what} must be ({cnt},) float64 on {real.device}")
    r2_real, r2_fake = r2_real.contiguous(), r2_fake.contiguous()
    ws = _workspace(_OP_MANIFOLD, n, m, 0, 0, 0, real.device, "manifold")
    hits_fake = torch.empty(m, dtype=torch.int32, device=real.device)
    hits_real = torch.empty(n, dtype=torch.int32, device=real.device)
    nearest = torch.empty(n, dtype=torch.float64, device=real.device)
    with _lib.on(real.device):
        _lib.check(_lib.lib().hl_feat_manifold(_lib.ptr(real), n, _lib.ptr(fake), m, d, _vp(r2_real), _vp(r2_fake), int(_split), _vp(hits_fake), _vp(hits_real),
                                               _vp(nearest), _vp(ws), ws.numel() * 8, _lib.stream_ptr(real.device)), "hl_feat_manifold")
    return hits_fake, hits_real, nearest


def precision_recall(real, fake, k=3, _split=0):
    """Improved precision / recall and density / coverage with k-NN radii: a dict with
        precision = mean(hits_fake > 0)       hits_fake[j] = #{i : d2(r_i, f_j) <= r2_real[i]}
        recall    = mean(hits_real > 0)       hits_real[i] = #{j : d2(r_i, f_j) <= r2_fake[j]}
        density   = sum(hits_fake) / (k M)
        coverage  = mean(nearest_real <= r2_real)
    and the device tensors r2_real, r2_fake, hits_fake, hits_real, nearest_real.  The scalars are formed on the host, from integers,
    after one read-back."""
    real, fake = _pair(real, fake, "precision_recall")
    r2_real, r2_fake = knn_radii(real, k, _split), knn_radii(fake, k, _split)
    hits_fake, hits_real, nearest = manifold(real, fake, r2_real, r2_fake, _split)
    n, m = real.shape[0], fake.shape[0]
    covered = (nearest <= r2_real).to(torch.int32)
    host = torch.cat([hits_fake, hits_real, covered]).cpu().numpy()
    hf, hr, cv = host[:m], host[m:m + n], host[m + n:]
    return {"precision": int((hf > 0).sum()) / m, "recall": int((hr > 0).sum()) / n, "density": int(hf.astype(np.int64).sum()) / (k * m),
            "coverage": int(cv.sum()) / n, "r2_real": r2_real, "r2_fake": r2_fake, "hits_fake": hits_fake, "hits_real": hits_real,
            "nearest_real": nearest}


class FeatureCollector:
    """Views in, pool3 features out, `batch` views per InceptionFID call: add(image (3, h, w) float32 in [0, 1]) buffers a view; every
    `batch` views, on a view of another size, or on flush(), the buffered views go through the network in one call, then into `stats` (a
    FidStatistics) and / or the kept features.  An image's features do not depend on the batch it is in and the moments do not depend
    on how the images are split into updates, so neither differs by a bit from feeding the views one at a time."""

    def __init__(self, model, batch=64, stats=None, keep=True):
        if batch < 1:
            raise ValueError(f"FeatureCollector: batch {batch} must be at least 1")
        if stats is None and not keep:
            raise ValueError("FeatureCollector: neither statistics nor features are asked for")
        self.model, self.batch, self.stats, self.keep = model, int(batch), stats, bool(keep)
        self.count = 0
        self._pending, self._kept = [], []

    def add(self, image):
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
            raise RuntimeError(f"FeatureCollector: a view must be (3, h, w) float32, got "
                               f"{(tuple(image.shape), image.dtype) if torch.is_tensor(image) else type(image).__name__}")
        if not image.is_cuda:
            raise RuntimeError("FeatureCollector: a view must be a HIP tensor; humanliff_amd has no CPU path")
        if self._pending and image.shape != self._pending[0].shape:
            self.flush()
        self._pending.append(image.detach())
        if len(self._pending) == self.batch:
            self.flush()
        return self

    def flush(self):
        if self._pending:
            f = self.model(torch.stack(self._pending))
            self.count += len(self._pending)
            self._pending = []
            if self.stats is not None:
                self.stats.update(f)
            if self.keep:
                self._kept.append(f)
        return self

    def features(self):
        """(n, 2048) float32 on the device: the features of every view added so far, in order."""
        if not self.keep:
            raise RuntimeError("FeatureCollector: built with keep=False, the features were not kept")
        self.flush()
        if not self._kept:
            raise ValueError("FeatureCollector: no views were added")
        if len(self._kept) > 1:
            self._kept = [torch.cat(self._kept)]
        return self._kept[0]
