"""The feature metrics (humanliff_amd/feature_metrics.py) restated in numpy float64, with the error bounds the tests allow.

The Gram entry g(a, b) = sum_k a_k b_k of two float32 rows: the products are exact in float64, so `gram_exact` (math.fsum over them) is
the exact sum rounded once - the correctly rounded value.  `gram` is the same quantity by a float64 matrix product: some summation order,
so it carries an error within e_g itself; the larger cases use it, which is why a test allows twice the first-order bound (the
kernel's error plus the restatement's).

Bounds, u = 2^-53, first order:
    e_g  = (D - 1) u sum_k |a_k b_k| + u |g|                      any summation order, fused or not
    e_d2 = e_g(a,a) + e_g(b,b) + 2 e_g(a,b) + 3 u (g(a,a) + g(b,b) + 2 |g(a,b)|)
    e_k  = 3 (|g| / D + 1)^2 e_g / D + 8 u |k|                    k = (g / D + 1)^3
    a sum of n terms adds (n - 1) u sum |terms|"""
import math

import numpy as np

U = 2.0 ** -53


def f64(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


def gram_exact(x, y):
    x, y = f64(x), f64(y)
    out = np.empty((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        p = x[i][None, :] * y                    # exact: 24-bit x 24-bit significands
        for j in range(y.shape[0]):
            out[i, j] = math.fsum(p[j])
    return out


def gram(x, y):
    return f64(x) @ f64(y).T


def abs_gram(x, y):
    return np.abs(f64(x)) @ np.abs(f64(y)).T


def e_g(x, y, g=None):
    g = gram(x, y) if g is None else g
    return (x.shape[1] - 1) * U * abs_gram(x, y) + U * np.abs(g)


def norms(x, exact=False):
    """g(a, a) per row."""
    x64 = f64(x)
    if exact:
        return np.array([math.fsum(r * r) for r in x64])
    return np.einsum("ij,ij->i", x64, x64)


def e_norms(x, n=None):
    n = norms(x) if n is None else n
    return (x.shape[1] - 1) * U * n + U * n       # sum |a_k a_k| = g(a, a)


def d2(x, y, exact=False):
    g = gram_exact(x, y) if exact else gram(x, y)
    return np.maximum(norms(x, exact)[:, None] + norms(y, exact)[None, :] - 2.0 * g, 0.0)


def e_d2(x, y):
    g, nx, ny = gram(x, y), norms(x), norms(y)
    return e_norms(x, nx)[:, None] + e_norms(y, ny)[None, :] + 2.0 * e_g(x, y, g) + 3.0 * U * (nx[:, None] + ny[None, :] + 2.0 * np.abs(g))


def poly(g, dim):
    return (g / dim + 1.0) ** 3


def e_k(x, y, g=None):
    g = gram(x, y) if g is None else g
    dim = x.shape[1]
    return 3.0 * (np.abs(g) / dim + 1.0) ** 2 * e_g(x, y, g) / dim + 8.0 * U * np.abs(poly(g, dim))


def subset_indices(n, m, subsets, size, seed=2020):
    """torch-fidelity's rule as recalled: one RandomState; per subset a choice without replacement for x, then one for y."""
    rng = np.random.RandomState(seed)
    xi, yi = [], []
    for _ in range(subsets):
        xi.append(rng.choice(n, size, replace=False))
        yi.append(rng.choice(m, size, replace=False))
    return np.array(xi, dtype=np.int32), np.array(yi, dtype=np.int32)


def kid_subset(x, y, xi, yi):
    """(mmd^2, its first-order bound) of one subset: the unbiased estimator of the cubic kernel; the diagonal is left out by position."""
    a, b = x[xi], y[yi]
    m, dim = a.shape[0], a.shape[1]
    off = ~np.eye(m, dtype=bool)
    total, bound = [], []
    for (p, q, mask) in ((a, a, off), (b, b, off), (a, b, np.ones((m, m), dtype=bool))):
        g = gram(p, q)
        k = poly(g, dim)
        terms = k[mask]
        total.append(math.fsum(terms))
        bound.append(float(e_k(p, q, g)[mask].sum()) + (terms.size - 1) * U * float(np.abs(terms).sum()))
    mm1, mm = m * (m - 1.0), float(m * m)
    parts = (total[0] / mm1, total[1] / mm1, 2.0 * total[2] / mm)
    value = parts[0] + parts[1] - parts[2]
    err = bound[0] / mm1 + bound[1] / mm1 + 2.0 * bound[2] / mm + 4.0 * U * sum(abs(p) for p in parts)
    return value, err


def kid(x, y, xi, yi):
    rows = [kid_subset(x, y, xi[s], yi[s]) for s in range(xi.shape[0])]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def knn_radii(x, k, dist=None):
    """The k-th smallest d2 of every row to the other rows (its own index left out; duplicates of it stay)."""
    dist = d2(x, x) if dist is None else dist
    n = dist.shape[0]
    others = dist[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.sort(others, axis=1)[:, k - 1]


def prc(real, fake, k, exact=False):
    """exact: from the correctly rounded Gram entries, where bit-equal rows are at exactly 0 (the matrix product gives them a d2 of rounding size)."""
    n, m = real.shape[0], fake.shape[0]
    r2_real, r2_fake = knn_radii(real, k, d2(real, real, exact)), knn_radii(fake, k, d2(fake, fake, exact))
    cross = d2(real, fake, exact)
    hits_fake = (cross <= r2_real[:, None]).sum(0).astype(np.int32)
    hits_real = (cross <= r2_fake[None, :]).sum(1).astype(np.int32)
    nearest = cross.min(1)
    return {"precision": int((hits_fake > 0).sum()) / m, "recall": int((hits_real > 0).sum()) / n, "density": int(hits_fake.sum()) / (k * m),
            "coverage": int((nearest <= r2_real).sum()) / n, "r2_real": r2_real, "r2_fake": r2_fake, "hits_fake": hits_fake, "hits_real": hits_real,
            "nearest_real": nearest, "cross": cross}


def smallest_gap(real, fake, k):
    """(the smallest |d2 - threshold| over every comparison precision_recall makes, the largest first-order bound on a d2 or a threshold in
    them, the largest d2): while the gap exceeds the bounds by orders of magnitude no comparison is ambiguous."""
    p = prc(real, fake, k)
    cross = p["cross"]
    gap = min(np.abs(cross - p["r2_real"][:, None]).min(), np.abs(cross - p["r2_fake"][None, :]).min(), np.abs(p["nearest_real"] - p["r2_real"]).min())
    # the k-th neighbour must also be apart from the (k+1)-th or tied exactly: the radius is a value, not an index, so no gap is needed there
    err = max(e_d2(real, fake).max(), e_d2(real, real).max(), e_d2(fake, fake).max())
    return float(gap), float(err), float(cross.max())
