"""hl_feat on the MI355X (humanliff_amd/feature_metrics.py, csrc/hl_feature_metrics.hip) against the numpy float64 restatement
(tests/feature_metrics_restatement.py).  Every tolerance is twice the first-order bound computed from the test's own inputs (the
restatement's docstring); hit counts and the four scalars must be equal, which tests/test_feature_metrics_cpu.py shows to be a fair
demand on these cases.  Each test prints its worst ratio of error to (single) bound.

Observed on one MI355X (ratio of the error to the first-order bound, worst over the case): DESIGN.md 4m."""
import os
import sys

import numpy as np
import pytest
import torch

from humanliff_amd import feature_metrics as hm
from tests import feature_metrics_cases as fcs
from tests import feature_metrics_restatement as fm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def worst(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


def check_pairwise(x, y, label):
    g, dd = host(hm.pairwise(dev(x), dev(y), "gram")), host(hm.pairwise(dev(x), dev(y)))
    assert g.shape == dd.shape == (x.shape[0], y.shape[0]) and g.dtype == dd.dtype == np.float64
    want_g = fm.gram_exact(x, y)
    want_d = np.maximum(fm.norms(x, exact=True)[:, None] + fm.norms(y, exact=True)[None, :] - 2.0 * want_g, 0.0)
    rg, rd = worst(np.abs(g - want_g), fm.e_g(x, y, want_g)), worst(np.abs(dd - want_d), fm.e_d2(x, y))
    print(f"pairwise {label}: error / bound: gram {rg:.3f}, d2 {rd:.3f}")
    assert rg <= 2.0 and rd <= 2.0, label
    assert np.all(dd >= 0.0)


@pytest.mark.parametrize("n,m,d", [(2, 1, 1), (63, 65, 70), (64, 64, 2048), (65, 130, 2048), (257, 33, 333)])
def test_pairwise_against_the_correctly_rounded_gram(n, m, d):
    check_pairwise(fcs.random_features(n, d, 11), fcs.random_features(m, d, 12), f"({n}, {m}, {d})")


def test_pairwise_on_signed_features_over_six_decades():
    x, y = fcs.signed(40, 301, 13), fcs.signed(70, 301, 14)
    assert np.median(fm.abs_gram(x, y) / np.abs(fm.gram_exact(x, y))) > 3.0
    check_pairwise(x, y, "signed 1e-3 .. 1e3 (40, 70, 301)")


@pytest.mark.parametrize("d", [2048, 70])
def test_an_entry_depends_on_the_two_rows_alone(d):
    a, b = fcs.random_features(1, d, 21), fcs.random_features(1, d, 22)
    fx, fy = fcs.random_features(130, d, 23), fcs.random_features(200, d, 24)
    alone = {k: hm.pairwise(dev(a), dev(b), k) for k in ("gram", "d2")}
    for i, j in ((0, 0), (129, 199), (63, 64), (64, 63), (64, 127), (65, 128)):       # start, end, and both sides of the 64-row tile edges
        x, y = fx.copy(), fy.copy()
        x[i], y[j] = a[0], b[0]
        for k in ("gram", "d2"):
            there = hm.pairwise(dev(x), dev(y), k)
            assert torch.equal(there[i, j], alone[k][0, 0]), (k, i, j)
            swapped = hm.pairwise(dev(y), dev(x), k)
            assert torch.equal(swapped, there.T.contiguous()), (k, i, j, "sides swapped")
    x = dev(fx)
    dd = hm.pairwise(x, x)
    assert torch.equal(torch.diagonal(dd), torch.zeros(130, dtype=torch.float64, device=DEV)) and float(dd.max()) > 1.0
    assert torch.equal(dd, dd.T) and torch.equal(dd, hm.pairwise(x, x))
    # a copy of a row elsewhere is at distance exactly 0 as well
    y = fy.copy()
    y[77] = fx[5]
    assert float(hm.pairwise(x, dev(y))[5, 77]) == 0.0


@pytest.mark.parametrize("n,m,d,s,sub", [(65, 63, 2048, 4, 33), (130, 257, 70, 3, 64), (64, 64, 2048, 1, 64), (5, 7, 3, 2, 2)])
def test_kid_per_subset_against_the_restatement(n, m, d, s, sub):
    x, y = fcs.random_features(n, d, 31), fcs.random_features(m, d, 32) * np.float32(1.1)
    mean, std, per = hm.kernel_inception_distance(dev(x), dev(y), subsets=s, subset_size=sub, seed=2020)
    again = hm.kernel_inception_distance(dev(x), dev(y), subsets=s, subset_size=sub, seed=2020)[2]
    assert per.shape == (s,) and per.dtype == torch.float64 and per.device == DEV and torch.equal(per, again)
    xi, yi = fm.subset_indices(n, m, s, sub, 2020)
    want, bound = fm.kid(x, y, xi, yi)
    got = host(per)
    r = worst(np.abs(got - want), bound)
    print(f"KID ({n}, {m}, {d}, {s} x {sub}): {got} (restatement {want}); error / bound {r:.3f}")
    assert r <= 2.0
    assert mean == float(np.mean(got)) and std == float(np.std(got))
    assert torch.equal(hm.kid_subsets(dev(x), dev(y), xi, yi), per)


def test_kid_of_all_ones_is_zero_and_bad_subsets_raise():
    x, y = torch.ones((5, 1), device=DEV), torch.ones((4, 1), device=DEV)
    assert torch.equal(hm.pairwise(x, y, "gram"), torch.ones((5, 4), dtype=torch.float64, device=DEV))
    mean, std, per = hm.kernel_inception_distance(x, y, subsets=3, subset_size=3)
    assert mean == 0.0 and std == 0.0 and torch.equal(per, torch.zeros(3, dtype=torch.float64, device=DEV))
    for bad in (1, 5):
        with pytest.raises(ValueError, match="subset_size"):
            hm.kernel_inception_distance(x, y, subsets=3, subset_size=bad)
    with pytest.raises(ValueError, match="outside"):
        hm.kid_subsets(x, y, np.array([[0, 5]]), np.array([[0, 1]]))


@pytest.mark.parametrize("case", fcs.CASES, ids=fcs.case_id)
def test_precision_recall_counts_are_the_restatements(case):
    real, fake = fcs.sets(case)
    dr, df = dev(real), dev(fake)
    e_rr, e_ff, e_rf = fm.e_d2(real, real).max(1), fm.e_d2(fake, fake).max(1), fm.e_d2(real, fake).max(1)
    for k in fcs.KS:
        want = fcs.reference(case, k)
        got = hm.precision_recall(dr, df, k)
        assert got["hits_fake"].dtype == got["hits_real"].dtype == torch.int32 and got["nearest_real"].dtype == torch.float64
        assert np.array_equal(host(got["hits_fake"]), want["hits_fake"]), k
        assert np.array_equal(host(got["hits_real"]), want["hits_real"]), k
        ratios = [worst(np.abs(host(got[key]) - want[key]), e) for key, e in (("r2_real", e_rr), ("r2_fake", e_ff), ("nearest_real", e_rf))]
        print(f"{fcs.case_id(case)} k={k}: error / bound: r2_real {ratios[0]:.3f}, r2_fake {ratios[1]:.3f}, nearest_real {ratios[2]:.3f}")
        assert max(ratios) <= 2.0, k
        for key in ("precision", "recall", "density", "coverage"):
            assert got[key] == want[key], (key, k)


def test_ties_at_zero_and_own_index():
    k, d = 3, 70
    real, fake = fcs.random_features(40, d, 41), fcs.random_features(20, d, 42)
    real[[3, 17, 38]] = real[9]                                   # one row k + 1 times: its k nearest others are copies, at 0
    fake[4] = real[9]                                             # a copy among the fake rows: inside (0 <= 0)
    fake[5] = real[9]
    fake[5, 0] += np.float32(2.0 ** -10)                          # a fake row at a small positive distance: outside a radius of 0
    got = hm.precision_recall(dev(real), dev(fake), k)
    r2, hits_fake, nearest = host(got["r2_real"]), host(got["hits_fake"]), host(got["nearest_real"])
    assert np.all(r2[[3, 9, 17, 38]] == 0.0) and np.all(np.delete(r2, [3, 9, 17, 38]) > 0.0)
    want = fm.prc(real, fake, k, exact=True)
    assert np.array_equal(hits_fake, want["hits_fake"]) and np.array_equal(host(got["hits_real"]), want["hits_real"])
    assert hits_fake[4] >= 4 and np.all(nearest[[3, 9, 17, 38]] == 0.0)
    cross = host(hm.pairwise(dev(real), dev(fake)))
    assert 0.0 < cross[9, 5] < 1e-5 and hits_fake[5] == int((cross[:, 5] <= r2).sum()) and not np.any(cross[[3, 9, 17, 38], 5] <= 0.0)
    # own index by position: k = 1 on a set with one duplicated pair gives 0 for the pair only, and never the row's own 0
    pair = fcs.random_features(10, d, 43)
    pair[7] = pair[2]
    r1 = host(hm.knn_radii(dev(pair), 1))
    assert r1[2] == 0.0 and r1[7] == 0.0 and np.all(np.delete(r1, [2, 7]) > 0.0)
    assert np.array_equal(host(hm.knn_radii(dev(pair), 2)) > 0.0, np.ones(10, dtype=bool))
    for bad in (0, 9, 10):
        with pytest.raises(ValueError, match="knn_radii"):
            hm.knn_radii(dev(pair), bad)


@pytest.mark.parametrize("d", [2048, 70])
def test_column_split_does_not_change_a_bit(d):
    case = (257, 64, 0.4, 0.8, d)
    real, fake = (dev(a) for a in fcs.sets(case))
    one = hm.precision_recall(real, fake, 3, _split=1)
    assert np.array_equal(host(one["hits_fake"]), fcs.reference(case, 3)["hits_fake"])
    for split in (0, 2, 3, 5):
        other = hm.precision_recall(real, fake, 3, _split=split)
        for key in ("r2_real", "r2_fake", "hits_fake", "hits_real", "nearest_real"):
            assert torch.equal(one[key], other[key]), (split, key)
    for k in (1, 8):
        assert torch.equal(hm.knn_radii(real, k, _split=1), hm.knn_radii(real, k, _split=5)), k
        err = np.abs(host(hm.knn_radii(real, k, _split=4)) - fm.knn_radii(fcs.sets(case)[0], k))
        assert worst(err, fm.e_d2(fcs.sets(case)[0], fcs.sets(case)[0]).max(1)) <= 2.0, k


def test_nothing_is_read_back_before_the_results():
    x, y = dev(fcs.random_features(70, 64, 51)), dev(fcs.random_features(66, 64, 52))
    xi, yi = fm.subset_indices(70, 66, 2, 9)
    dxi = hm.kid_subsets(x, y, xi, yi)                              # (warm: the library is loaded, the allocator has its blocks)
    r2x, r2y = hm.knn_radii(x, 2), hm.knn_radii(y, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        hm.pairwise(x, y)
        hm.knn_radii(x, 2)
        hm.manifold(x, y, r2x, r2y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert dxi.shape == (2,)


@pytest.fixture(scope="module")
def inception():
    from humanliff_amd.fid import InceptionFID
    from tests import fid_cases as fc
    sd = fc.weights().state_dict()
    return sd, InceptionFID.from_state_dict(sd, DEV, resize_input=False)


def _images(seed, n=5, side=75):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, 3, side, side), generator=g) * 255.0).round().to(torch.uint8)


def test_collector_changes_no_bit(inception):
    from humanliff_amd.fid import FidStatistics
    _, model = inception
    imgs = (_images(61).float() / 255.0).to(DEV)
    batched = hm.FeatureCollector(model, batch=2, stats=FidStatistics(DEV))
    single = hm.FeatureCollector(model, batch=1, stats=FidStatistics(DEV))
    by_hand = FidStatistics(DEV)
    for im in imgs:
        batched.add(im)
        single.add(im)
        by_hand.update(model(im.clone()))                 # (a fresh allocation: the network wants 16-byte aligned images)
    fb, fs = batched.features(), single.features()
    assert fb.shape == (5, 2048) and fb.dtype == torch.float32 and batched.count == single.count == 5
    assert torch.equal(fb, fs) and torch.equal(fb, torch.cat([model(im.clone()) for im in imgs]))
    assert torch.equal(batched.stats._state, single.stats._state) and torch.equal(batched.stats._state, by_hand._state)
    assert batched.stats.count == 5 and float(fb.abs().max()) > 0.1
    only_stats = hm.FeatureCollector(model, batch=4, stats=FidStatistics(DEV), keep=False)
    for im in imgs:
        only_stats.add(im)
    only_stats.flush()
    assert torch.equal(only_stats.stats._state, by_hand._state)
    with pytest.raises(RuntimeError, match="keep=False"):
        only_stats.features()


def test_script_prints_the_numbers_of_the_direct_calls(inception, tmp_path, capsys):
    from PIL import Image
    from humanliff_amd.fid import FidStatistics, frechet_distance
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import triplane_fid
    finally:
        sys.path.pop(0)
    sd, _ = inception
    weights = str(tmp_path / "w.pt")
    torch.save(sd, weights)
    sets = {"a": _images(61), "b": _images(62)}
    for name, imgs in sets.items():
        os.makedirs(tmp_path / name)
        for i, im in enumerate(imgs):
            Image.fromarray(im.permute(1, 2, 0).numpy()).save(str(tmp_path / name / f"{i:02d}.png"))
    out_a, out_b = str(tmp_path / "fa.npy"), str(tmp_path / "fb.npy")
    argv = [str(tmp_path / "a"), str(tmp_path / "b"), "--inception-weights", weights, "--batch", "2", "--save-features", out_a, out_b,
            "--kid", "--kid-subsets", "3", "--kid-subset-size", "4", "--prc", "--prc-k", "2"]
    triplane_fid.main(argv)
    lines = capsys.readouterr().out.strip().splitlines()
    # the direct calls (the script resizes to 299 x 299, as pytorch-fid does)
    from humanliff_amd.fid import InceptionFID
    model = InceptionFID.from_state_dict(sd, DEV)
    feats, stats = [], []
    for name in ("a", "b"):
        f = model(sets[name].to(DEV).float() / 255.0)             # (scaled on the device, as the script does)
        feats.append(f)
        stats.append(FidStatistics(DEV).update(f).finalize())
    assert np.array_equal(np.load(out_a), host(feats[0])) and np.array_equal(np.load(out_b), host(feats[1]))
    fid = frechet_distance(*stats[0], *stats[1])
    mean, std, _ = hm.kernel_inception_distance(feats[0], feats[1], subsets=3, subset_size=4)
    p = hm.precision_recall(feats[0], feats[1], 2)
    assert len(lines) == 3 and lines[0].startswith(f"FID {fid:.6f}  (") and "5 images" in lines[0]
    assert lines[1] == triplane_fid.kid_line(mean, std, 3, 4) and lines[2] == triplane_fid.prc_line(p, 2)
    assert all(np.isfinite(v) for v in (fid, mean, std, p["precision"], p["recall"], p["density"], p["coverage"]))
    # the saved features score the same without the network; statistics alone cannot give KID
    triplane_fid.main([out_a, out_b, "--kid", "--kid-subsets", "3", "--kid-subset-size", "4", "--prc", "--prc-k", "2"])
    again = capsys.readouterr().out.strip().splitlines()
    assert again[1:] == lines[1:] and again[0].split("  (")[0] == lines[0].split("  (")[0]
    stats_file = str(tmp_path / "a.npz")
    triplane_fid.main([out_a, out_b, "--save-stats", stats_file])
    capsys.readouterr()
    with pytest.raises(SystemExit, match="features"):
        triplane_fid.main([stats_file, out_b, "--kid"])
