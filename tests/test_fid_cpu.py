"""What can be said about the native FID without a GPU: the test recipe's own conditions (the bound constants against the recomputed
float32 noise), the loader against both spellings of the state-dict keys and its float64 BatchNorm fold, the distance against
pytorch-fid's formula restated with scipy's sqrtm, the moment rule against numpy's mean and covariance, the statistics file, and the
layer table of the library against the loader's and the restatement's."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fid_cases as fc
from tests import fid_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bound_constants_follow_the_float32_noise():
    fig = fc.float32_noise()
    pipe = fc.float32_pipeline_noise()
    print(f"float32-CPU noise: blocks {['%.3e' % f for f in fig]}, pipeline {pipe:.3e} (distance {fc.pipeline_reference():.6f})")
    for k in range(4):
        assert fig[k] <= fc.BLOCK_BOUND[k] <= 4.0 * fig[k], k
    assert pipe <= fc.PIPELINE_BOUND <= 4.0 * pipe


def test_the_restatement_is_the_network_of_the_loader():
    from humanliff_amd import fid
    P = fc.weights()
    assert len(fid.LAYERS) == 94 and [(n, d[:4]) for n, d in fid.LAYERS] == P.rows
    assert sum(p[0].numel() for p in P.p.values()) == 21751136
    assert all(fid.wrapper_name(n) == fr.wrapper_name(n) for n, _ in fid.LAYERS)
    for name, shapes in fc.BLOCK_SHAPES.items():
        ref = fc.reference(name)
        assert [tuple(b.shape) for b in ref] == [(fc.CASES[name][0],) + s for s in shapes], name
        f = ref[3]
        assert 0.05 < float(f.mean()) < 2.0 and float(f.max()) < 20.0 and 0.05 < float((f == 0).double().mean()) < 0.6, name


def test_library_and_python_layer_tables_agree():
    from humanliff_amd import _lib, fid
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    assert fid.library_layers() == fid.LAYERS
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    names = ("hl_fid_layer", "hl_fid_workspace_bytes", "hl_fid_block_shape", "hl_fid_features", "hl_fid_moments_update", "hl_fid_moments_finalize")
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("hl_fid_")) == sorted(names)
    assert _lib.HL_FID_LAYERS == int(re.search(r"#define HL_FID_LAYERS (\d+)", hdr).group(1)) == len(fid.LAYERS)
    # below 75 on a side without resize, or no images: no workspace; bad arguments come back as a status, before any launch
    assert L.hl_fid_workspace_bytes(1, 74, 75, 0) == 0 and L.hl_fid_workspace_bytes(1, 75, 74, 0) == 0 and L.hl_fid_workspace_bytes(0, 75, 75, 0) == 0
    assert L.hl_fid_workspace_bytes(1, 75, 75, 0) > 0 and L.hl_fid_workspace_bytes(1, 8, 8, 1) == L.hl_fid_workspace_bytes(1, 300, 20, 1)
    assert L.hl_fid_workspace_bytes(2, 107, 139, 0) >= 2 * 4 * (107 * 139 * 16 + 25 * 33 * 64 + 11 * 15 * 192 + 5 * 7 * 768 + 2048)
    assert L.hl_fid_features(None, None, 1, 75, 75, 0, 1, None, None, 0, None) < 0 and b"hl_fid_features" in L.hl_last_error()
    assert L.hl_fid_moments_finalize(None, 5, None, None, None) < 0
    assert L.hl_fid_layer(94, None, 0, None) < 0


def _same_weights(model, P):
    ok = len(model._host) == 94
    for (name, _), (w, b) in zip(fc.weights().rows, model._host):
        cw, gamma, beta, mean, var = P.p[name]
        scale = gamma.double() / torch.sqrt(var.double() + 1e-3)
        ok = ok and torch.equal(w, (cw.double() * scale.view(-1, 1, 1, 1)).float()) and torch.equal(b, (beta.double() - mean.double() * scale).float())
    return ok


def test_loader_takes_both_key_spellings_and_ignores_the_rest():
    from humanliff_amd.fid import InceptionFID
    P = fc.weights()
    plain, wrapped = P.state_dict(), P.state_dict(fr.wrapper_name)
    assert len(plain) == len(wrapped) == 5 * 94 and "Mixed_6c.branch7x7dbl_4.bn.running_var" in plain and "blocks.2.5.branch7x7dbl_4.bn.running_var" in wrapped
    assert "blocks.0.0.conv.weight" in wrapped and "blocks.1.1.bn.bias" in wrapped and "blocks.3.2.branch_pool.conv.weight" in wrapped
    extra = {"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1),
             "Mixed_5b.branch1x1.bn.num_batches_tracked": torch.tensor(0), "blocks.0.0.bn.num_batches_tracked": torch.tensor(0)}
    for sd in (plain, wrapped, {**plain, **extra}, {**wrapped, **extra}):
        model = InceptionFID.from_state_dict(sd)
        assert _same_weights(model, P) and model.resize_input and model.normalize_input
    mixed = {k: v for k, v in plain.items() if not k.startswith("Mixed_7")}
    mixed.update({k: v for k, v in wrapped.items() if k.startswith("blocks.3.")})
    assert _same_weights(InceptionFID.from_state_dict(mixed, resize_input=False), P)


def test_loader_names_missing_and_misshaped_keys():
    from humanliff_amd.fid import InceptionFID
    sd = fc.weights().state_dict()
    with pytest.raises(KeyError, match=r"Mixed_6e\.branch7x7_3\.conv\.weight.*blocks\.2\.7\.branch7x7_3\.conv\.weight"):
        InceptionFID.from_state_dict({k: v for k, v in sd.items() if k != "Mixed_6e.branch7x7_3.conv.weight"})
    with pytest.raises(KeyError, match=r"Conv2d_3b_1x1\.bn\.running_mean"):
        InceptionFID.from_state_dict({k: v for k, v in sd.items() if k != "Conv2d_3b_1x1.bn.running_mean"})
    with pytest.raises(ValueError, match=r"Mixed_7a\.branch7x7x3_2\.conv\.weight"):
        InceptionFID.from_state_dict({**sd, "Mixed_7a.branch7x7x3_2.conv.weight": sd["Mixed_7a.branch7x7x3_2.conv.weight"].transpose(2, 3)})
    with pytest.raises(ValueError, match=r"Mixed_5c\.branch_pool\.bn\.weight"):
        InceptionFID.from_state_dict({**sd, "Mixed_5c.branch_pool.bn.weight": sd["Mixed_5c.branch_pool.bn.weight"][:32]})
    with pytest.raises(ValueError, match=r"Conv2d_1a_3x3\.bn\.bias"):
        InceptionFID.from_state_dict({**sd, "Conv2d_1a_3x3.bn.bias": [0.0] * 32})
    with pytest.raises(RuntimeError, match="no CPU path"):
        InceptionFID.from_state_dict(sd, device="cpu")


def test_batchnorm_fold_is_the_convolution_and_batchnorm_in_float64():
    from humanliff_amd.fid import fold_batchnorm
    P = fc.weights()
    g = torch.Generator().manual_seed(3)
    for name in ("Conv2d_1a_3x3", "Mixed_5b.branch5x5_2", "Mixed_6b.branch7x7dbl_2", "Mixed_7c.branch3x3_2a"):
        cw, gamma, beta, mean, var = (t.double() for t in P.p[name])
        w, b = fold_batchnorm(*P.p[name])
        assert w.dtype == torch.float64 and b.dtype == torch.float64
        x = torch.randn((2, cw.shape[1], 9, 11), generator=g, dtype=torch.float64)
        pad = (cw.shape[2] // 2, cw.shape[3] // 2)
        want = F.batch_norm(F.conv2d(x, cw, None, padding=pad), mean, var, gamma, beta, False, 0.0, 1e-3)
        got = F.conv2d(x, w, b, padding=pad)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


def test_arguments_are_checked_before_any_launch():
    from humanliff_amd.fid import FidStatistics, InceptionFID
    sd = fc.weights().state_dict()
    model = InceptionFID.from_state_dict(sd, resize_input=False)
    for bad in (torch.zeros(1, 3, 74, 75), torch.zeros(3, 80, 74)):
        with pytest.raises(ValueError, match="74"):
            model(bad)
        with pytest.raises(ValueError, match="74"):
            model.blocks(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 3, 75, 75))
    with pytest.raises(RuntimeError, match="no CPU path"):
        InceptionFID.from_state_dict(sd)(torch.zeros(1, 3, 20, 20))            # with resize any size is served - on the device
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 1, 80, 80))
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 3, 80, 80).double())
    assert model._params is None, "nothing was uploaded or launched"
    with pytest.raises(RuntimeError, match="no CPU path"):
        FidStatistics("cpu")


def _relu_features(d, n, seed):
    g = np.random.default_rng(seed)
    w = g.standard_normal((d, d)) / np.sqrt(d)
    return np.maximum(g.standard_normal((n, d)) @ w + 0.3 * g.standard_normal(d), 0.0)


@pytest.mark.parametrize("d,n", [(256, 600), (512, 3000)])
def test_frechet_distance_is_pytorch_fids_formula(d, n):
    pytest.importorskip("scipy")
    from humanliff_amd.fid import frechet_distance
    a, b = _relu_features(d, n, 1), _relu_features(d, n, 2)
    stats = (a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False))
    want = fr.frechet_sqrtm(*stats)
    got = frechet_distance(*stats)
    print(f"D = {d}, N = {n}: {got!r} (sqrtm {want!r}), relative difference {abs(got - want) / want:.2e}")
    assert want > 1.0 and abs(got - want) <= 1e-10 * want
    assert got == pytest.approx(frechet_distance(*(torch.from_numpy(s) for s in stats)), rel=1e-14)


def test_frechet_distance_identity_symmetry_and_few_images():
    from humanliff_amd.fid import frechet_distance
    a, b = _relu_features(256, 600, 3), _relu_features(256, 600, 4)
    ma, sa, mb, sb = a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)
    assert abs(frechet_distance(ma, sa, ma, sa)) <= 1e-9 * np.trace(sa)
    ab, ba = frechet_distance(ma, sa, mb, sb), frechet_distance(mb, sb, ma, sa)
    assert ab > 1.0 and abs(ab - ba) <= 1e-10 * ab
    # fewer images than dimensions: singular covariances, where sqrtm goes complex; the distance stays real, finite and behaves
    few_a, few_b = a[:40], b[:40]
    fa, fb = (few_a.mean(0), np.cov(few_a, rowvar=False)), (few_b.mean(0), np.cov(few_b, rowvar=False))
    d = frechet_distance(*fa, *fb)
    assert isinstance(d, float) and np.isfinite(d) and d > 0.0
    assert abs(frechet_distance(*fa, *fa)) <= 1e-9 * np.trace(fa[1])
    with pytest.raises(ValueError):
        frechet_distance(ma, sa, mb[:100], sb[:100, :100])


def test_moment_rule_is_mean_and_covariance():
    g = np.random.default_rng(5)
    for n, d in ((9, 2048), (50, 300), (2, 64)):
        x = np.maximum(g.standard_normal((n, d)) + 0.4, 0.0).astype(np.float32)
        mu, sigma = fr.moments(x)
        want_mu, want_sigma = x.astype(np.float64).mean(0), np.cov(x.astype(np.float64), rowvar=False)
        scale = np.abs(want_sigma).max()
        err = np.abs(sigma - want_sigma).max() / scale
        print(f"n = {n}, D = {d}: sigma differs by {err:.2e} of max|sigma|, mu by {np.abs(mu - want_mu).max():.2e}")
        assert err <= 1e-12 and np.abs(mu - want_mu).max() <= 1e-12 * np.abs(want_mu).max()
        assert np.array_equal(sigma, sigma.T)


def test_statistics_file_round_trip(tmp_path):
    from humanliff_amd.fid import FidStatistics, load_statistics, save_statistics
    g = np.random.default_rng(6)
    x = g.standard_normal((20, 32))
    mu, sigma = x.mean(0), np.cov(x, rowvar=False)
    path = str(tmp_path / "stats.npz")
    save_statistics(path, torch.from_numpy(mu), sigma)
    with np.load(path) as z:                       # pytorch-fid's --save-stats layout
        assert sorted(z.files) == ["mu", "sigma"] and z["mu"].dtype == np.float64 and z["sigma"].shape == (32, 32)
    got_mu, got_sigma = load_statistics(path)
    assert got_mu.dtype == torch.float64 and np.array_equal(got_mu.numpy(), mu) and np.array_equal(got_sigma.numpy(), sigma)
    assert all(torch.equal(a, b) for a, b in zip(FidStatistics.load(path), (got_mu, got_sigma)))
    np.savez(str(tmp_path / "bad.npz"), mu=mu)
    with pytest.raises(KeyError, match="sigma"):
        load_statistics(str(tmp_path / "bad.npz"))
    np.savez(str(tmp_path / "odd.npz"), mu=mu, sigma=sigma[:5])
    with pytest.raises(ValueError):
        load_statistics(str(tmp_path / "odd.npz"))
