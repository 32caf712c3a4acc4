"""What can be said about the feature metrics without a GPU: the cases' own conditions (no comparison of a distance with a radius is
within reach of float64 error, so the GPU test may demand equal integers), the restatement against scikit-learn, the subset rule, the
degenerate KID, and the library's names and argument checks."""
import os
import re

import numpy as np
import pytest

from tests import feature_metrics_cases as fcs
from tests import feature_metrics_restatement as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hl_feat_workspace_bytes", "hl_feat_split", "hl_feat_pairwise", "hl_feat_kid", "hl_feat_knn_radii", "hl_feat_manifold")


@pytest.mark.parametrize("case", fcs.CASES, ids=fcs.case_id)
def test_no_comparison_is_within_reach_of_rounding(case):
    real, fake = fcs.sets(case)
    assert real.shape == (case[0], case[4]) and fake.shape == (case[1], case[4]) and real.dtype == np.float32
    for k in fcs.KS:
        gap, err, largest = fm.smallest_gap(real, fake, k)
        p = fcs.reference(case, k)
        print(f"{fcs.case_id(case)} k={k}: precision {p['precision']:.3f} recall {p['recall']:.3f} density {p['density']:.3f} coverage {p['coverage']:.3f}; "
              f"smallest gap {gap:.3e} = {gap / largest:.2e} of the largest d2, e_d2 {err:.3e}, ratio {gap / err:.2e}")
        assert gap > 1e3 * err, (case, k)


def test_the_cases_are_not_trivial():
    rows = [fcs.reference(c, 3) for c in fcs.CASES]
    for key, lo, hi in (("precision", 0.05, 1.0), ("recall", 0.05, 0.99), ("density", 0.02, 2.5), ("coverage", 0.05, 0.95)):
        v = [r[key] for r in rows]
        print(f"{key}: {min(v):.3f} .. {max(v):.3f}")
        assert lo <= min(v) and max(v) <= hi and max(v) - min(v) > 0.3, key


def test_exact_gram_and_the_bounds():
    """The matrix-product Gram is within e_g of the correctly rounded one; e_g is far above |g| u only where the products cancel."""
    for x, y in ((fcs.random_features(9, 333, 1), fcs.random_features(7, 333, 2)), (fcs.signed(9, 300, 3), fcs.signed(7, 300, 4))):
        exact, quick, bound = fm.gram_exact(x, y), fm.gram(x, y), fm.e_g(x, y)
        assert np.all(np.abs(exact - quick) <= bound)
        assert np.array_equal(fm.norms(x, exact=True), np.diag(fm.gram_exact(x, x)))
        dd = fm.d2(x, x, exact=True)
        assert np.all(np.diag(dd) == 0.0) and np.all(np.abs(dd - fm.d2(x, x)) <= 2.0 * fm.e_d2(x, x))
    s = fcs.signed(9, 300, 3)
    assert np.median(fm.abs_gram(s, s) / np.maximum(np.abs(fm.gram(s, s)), 1e-300)) > 3.0


def test_restatement_agrees_with_scikit_learn():
    pytest.importorskip("sklearn")
    from sklearn.metrics.pairwise import polynomial_kernel
    from sklearn.neighbors import NearestNeighbors
    real, fake = fcs.sets(fcs.CASES[6])                     # D = 70
    dim = real.shape[1]
    want = polynomial_kernel(real.astype(np.float64), fake.astype(np.float64), degree=3, gamma=1.0 / dim, coef0=1.0)
    got = fm.poly(fm.gram(real, fake), dim)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    for k in fcs.KS:
        dist, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(real.astype(np.float64)).kneighbors(real.astype(np.float64))
        want_r2 = dist[:, k] ** 2                           # column 0 is the row itself
        got_r2 = fm.knn_radii(real, k)
        assert np.all(np.abs(got_r2 - want_r2) <= 1e-9 * want_r2.max()), k
    # the unbiased estimator, written the long way
    xi, yi = fm.subset_indices(real.shape[0], fake.shape[0], 2, 20)
    for s in range(2):
        a, b = real[xi[s]].astype(np.float64), fake[yi[s]].astype(np.float64)
        kxx, kyy, kxy = (polynomial_kernel(p, q, degree=3, gamma=1.0 / dim, coef0=1.0) for p, q in ((a, a), (b, b), (a, b)))
        m = 20
        want_kid = (kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2.0 * kxy.mean()
        value, err = fm.kid_subset(real, fake, xi[s], yi[s])
        assert abs(value - want_kid) <= 1e-11 * abs(kxy.mean()) and err < 1e-11 * abs(kxy.mean())


def test_subset_tables_follow_the_stated_sequence():
    from humanliff_amd.feature_metrics import subset_indices
    xi, yi = subset_indices(50, 40, 3, 7, seed=2020)
    rng = np.random.RandomState(2020)
    for s in range(3):
        assert np.array_equal(xi[s], rng.choice(50, 7, replace=False)) and np.array_equal(yi[s], rng.choice(40, 7, replace=False))
    assert xi.dtype == yi.dtype == np.int32 and xi.shape == (3, 7)
    assert all(np.array_equal(a, b) for a, b in zip(fm.subset_indices(50, 40, 3, 7), (xi, yi)))
    assert all(len(set(row)) == 7 for row in xi) and xi.max() < 50 and yi.max() < 40
    for bad in (1, 41):
        with pytest.raises(ValueError, match="subset_size"):
            subset_indices(50, 40, 3, bad)


def test_all_ones_features_give_kid_zero():
    x, y = np.ones((5, 1), dtype=np.float32), np.ones((4, 1), dtype=np.float32)
    assert np.all(fm.poly(fm.gram(x, y), 1) == 8.0)
    xi, yi = fm.subset_indices(5, 4, 3, 3)
    values, bounds = fm.kid(x, y, xi, yi)
    assert np.all(values == 0.0) and np.all(bounds < 1e-13)


def test_python_checks_arguments_before_the_library():
    import torch
    from humanliff_amd import feature_metrics as hm
    x = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hm.pairwise(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hm.kernel_inception_distance(x, x, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hm.precision_recall(x, x, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hm.knn_radii(x, 1)
    with pytest.raises(RuntimeError):
        hm.pairwise(x.double(), x)
    with pytest.raises(ValueError, match="kind"):
        hm.pairwise(x, x, kind="cosine")
    with pytest.raises(RuntimeError, match="no CPU path"):
        hm.FeatureCollector(None).add(torch.zeros(3, 75, 75))
    with pytest.raises(ValueError):
        hm.FeatureCollector(None, keep=False)


def test_header_bindings_and_library_agree():
    from humanliff_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_feat_")) == sorted(NAMES)
    assert sorted(set(re.findall(r"\b(hl_feat_\w+)\s*\(", hdr))) == sorted(NAMES)
    assert int(re.search(r"#define HL_FEAT_MAX_K (\d+)", hdr).group(1)) == 8
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)


def test_bad_arguments_come_back_as_a_status_before_any_launch():
    from humanliff_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    L = _lib.lib()
    p, big = 4096, 1 << 30          # a non-NULL, aligned address that is never dereferenced: every call below is refused on the host

    def refused(rc, name):
        return rc < 0 and name.encode() in L.hl_last_error()

    # workspace sizes: 0 for what is not served
    assert L.hl_feat_workspace_bytes(0, 10, 20, 0, 0, 0) >= 8 * 30 and L.hl_feat_workspace_bytes(0, 0, 20, 0, 0, 0) == 0
    assert L.hl_feat_workspace_bytes(1, 10, 20, 3, 5, 0) == 3 * 3 * 8 and L.hl_feat_workspace_bytes(1, 10, 20, 3, 1, 0) == 0
    assert L.hl_feat_workspace_bytes(1, 500, 500, 2, 130, 0) == 2 * 3 * 9 * 8
    assert L.hl_feat_workspace_bytes(2, 1, 1, 0, 0, 0) == 0 and L.hl_feat_workspace_bytes(2, 100, 100, 0, 0, 2) >= 8 * 100 + 2 * 100 * 8 * 8
    assert L.hl_feat_workspace_bytes(9, 10, 10, 1, 2, 0) == 0
    # the split rule: at most one chunk per 64-column tile, a caller's value taken as given up to that
    assert L.hl_feat_split(257, 64, 0) == 1 and L.hl_feat_split(257, 257, 3) == 3 and L.hl_feat_split(257, 257, 9) == 5
    assert L.hl_feat_split(10000, 10000, 0) == 7 and L.hl_feat_split(0, 5, 0) == 0
    # pairwise
    assert refused(L.hl_feat_pairwise(None, 4, p, 4, 8, 1, p, p, big, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 4, p, 4, 8, 1, None, p, big, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 4, p, 4, 0, 1, p, p, big, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 0, p, 4, 8, 1, p, p, big, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 4, p, 4, 8, 2, p, p, big, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 4, p, 4, 8, 1, p, p, 8, None), "hl_feat_pairwise")
    assert refused(L.hl_feat_pairwise(p, 4, p, 4, 8, 1, p, None, big, None), "hl_feat_pairwise")
    # KID
    assert refused(L.hl_feat_kid(p, 10, p, 10, 8, p, p, 2, 1, p, p, big, None), "hl_feat_kid")           # m < 2
    assert refused(L.hl_feat_kid(p, 10, p, 9, 8, p, p, 2, 10, p, p, big, None), "hl_feat_kid")           # m > M
    assert refused(L.hl_feat_kid(p, 10, p, 10, 8, None, p, 2, 5, p, p, big, None), "hl_feat_kid")
    assert refused(L.hl_feat_kid(p, 10, p, 10, 0, p, p, 2, 5, p, p, big, None), "hl_feat_kid")           # D = 0
    assert refused(L.hl_feat_kid(p, 10, p, 10, 8, p, p, 0, 5, p, p, big, None), "hl_feat_kid")
    assert refused(L.hl_feat_kid(p, 10, p, 10, 8, p, p, 2, 5, p, p, 8, None), "hl_feat_kid")
    # k-NN radii
    assert refused(L.hl_feat_knn_radii(p, 10, 8, 0, 0, p, p, big, None), "hl_feat_knn_radii")            # k = 0
    assert refused(L.hl_feat_knn_radii(p, 10, 8, 9, 0, p, p, big, None), "hl_feat_knn_radii")            # k > 8
    assert refused(L.hl_feat_knn_radii(p, 5, 8, 5, 0, p, p, big, None), "hl_feat_knn_radii")             # k >= N
    assert refused(L.hl_feat_knn_radii(p, 1, 8, 1, 0, p, p, big, None), "hl_feat_knn_radii")
    assert refused(L.hl_feat_knn_radii(None, 10, 8, 3, 0, p, p, big, None), "hl_feat_knn_radii")
    assert refused(L.hl_feat_knn_radii(p, 10, 0, 3, 0, p, p, big, None), "hl_feat_knn_radii")
    assert refused(L.hl_feat_knn_radii(p, 10, 8, 3, 0, p, p, 16, None), "hl_feat_knn_radii")
    # manifold
    assert refused(L.hl_feat_manifold(p, 4, p, 4, 8, None, p, 0, p, p, p, p, big, None), "hl_feat_manifold")
    assert refused(L.hl_feat_manifold(p, 4, p, 4, 8, p, p, 0, p, p, None, p, big, None), "hl_feat_manifold")
    assert refused(L.hl_feat_manifold(p, 4, p, 4, 0, p, p, 0, p, p, p, p, big, None), "hl_feat_manifold")
    assert refused(L.hl_feat_manifold(p, 4, p, 0, 8, p, p, 0, p, p, p, p, big, None), "hl_feat_manifold")
    assert refused(L.hl_feat_manifold(p, 4, p, 4, 8, p, p, 0, p, p, p, p, 8, None), "hl_feat_manifold")
