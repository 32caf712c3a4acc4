"""hl_fid on the MI355X (humanliff_amd/fid.py, csrc/hl_fid.hip) against the float64 restatement of pytorch-fid's InceptionV3
(tests/fid_restatement.py) on seeded random weights, the moment kernels against the numpy restatement of their rule bit for bit, and the
whole pipeline images -> features -> moments -> distance.

Bounds (tests/fid_cases.py): each block output may differ from float64 by 3.5 x what the restatement run in float32 on the CPU
differs from it, pooled over the cases; the pipeline's distance likewise."""
import numpy as np
import pytest
import torch

from humanliff_amd.fid import DIMS, FidStatistics, InceptionFID, frechet_distance
from tests import fid_cases as fc
from tests import fid_restatement as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def state_dict():
    return fc.weights().state_dict()


@pytest.fixture(scope="module")
def model(state_dict):
    return InceptionFID.from_state_dict(state_dict, DEV)


@pytest.fixture(scope="module")
def model_as_is(state_dict):
    return InceptionFID.from_state_dict(state_dict, DEV, resize_input=False)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_case_matches_the_restatement(model, model_as_is, name):
    n, h, w, resize = fc.CASES[name]
    net = model if resize else model_as_is
    x = fc.case(name).to(DEV)
    keep = x.clone()
    want = fc.reference(name)
    got = net.blocks(x)
    feats = net(x)
    assert feats.shape == (n, DIMS) and feats.dtype == torch.float32 and feats.device == DEV
    for k in range(4):
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32 and got[k].device == DEV, k
    assert torch.equal(feats, got[3].reshape(n, DIMS)), "model(x) is block 3"
    err = fc.errors(got, want)
    print(f"{name}: block errors over abs-max {['%.3e' % e for e in err]} (bounds {['%.1e' % b for b in fc.BLOCK_BOUND]})")
    for k in range(4):
        assert err[k] <= fc.BLOCK_BOUND[k], (name, k)
    assert torch.equal(x, keep), "the input is only read"


def test_repeatable_batched_and_without_a_sync(model_as_is):
    a = fc.case("107x139").to(DEV)[:1]
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.rand((1, 3, 107, 139), generator=g).to(DEV), a, torch.rand((1, 3, 107, 139), generator=g).to(DEV)])
    keep = x.clone()
    first, again = model_as_is.blocks(x), model_as_is.blocks(x)
    alone = model_as_is.blocks(a)
    for k in range(4):
        assert torch.equal(first[k], again[k]), k
        assert torch.equal(alone[k][0], first[k][1]), f"block {k}: an image alone and inside a batch of 3"
    assert torch.equal(model_as_is(x), first[3].reshape(3, DIMS)) and torch.equal(model_as_is(a[0]), model_as_is(a))
    assert torch.equal(x, keep)
    # nothing is read back on the way
    stats = FidStatistics(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats.update(model_as_is(x))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert stats.count == 3


def test_resize_of_a_299_input_changes_nothing(model, model_as_is):
    g = torch.Generator().manual_seed(6)
    x = torch.rand((1, 3, 299, 299), generator=g).to(DEV)
    with_resize, without = model.blocks(x), model_as_is.blocks(x)
    for k in range(4):
        assert torch.equal(with_resize[k], without[k]), k
    assert float(without[3].abs().max()) > 0.1


def test_moments_are_the_stated_rule_bit_for_bit():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((9, DIMS), generator=g) + 0.4).clamp_min(0.0) * (1.0 + 3.0 * torch.rand((1, DIMS), generator=g))
    xd = x.to(DEV)
    keep = xd.clone()
    once = FidStatistics(DEV).update(xd)
    split = FidStatistics(DEV)
    for part in (xd[:3], xd[3:4], xd[4:]):
        split.update(part)
    assert once.count == split.count == 9
    (mu, sigma), (mu_s, sigma_s) = once.finalize(), split.finalize()
    assert mu.shape == (DIMS,) and sigma.shape == (DIMS, DIMS) and mu.dtype == sigma.dtype == torch.float64 and sigma.device == DEV
    assert torch.equal(mu, mu_s) and torch.equal(sigma, sigma_s), "one update and updates of 3 + 1 + 5"
    assert torch.equal(sigma, sigma.T)
    want_mu, want_sigma = fr.moments(x.numpy())
    assert np.array_equal(mu.cpu().numpy(), want_mu)
    assert np.array_equal(sigma.cpu().numpy(), want_sigma)
    assert torch.equal(xd, keep)
    one = FidStatistics(DEV).update(xd[:1])
    with pytest.raises(ValueError, match="at least 2"):
        one.finalize()
    with pytest.raises(ValueError, match="at least 2"):
        FidStatistics(DEV).finalize()
    with pytest.raises(RuntimeError):
        once.update(xd[:, :100])


def test_images_to_distance(model, tmp_path):
    set_a, set_b = (s.to(DEV) for s in fc.pipeline_sets())
    stats = []
    for s in (set_a, set_b):
        st = FidStatistics(DEV)
        st.update(model(s[:4]))
        st.update(model(s[4:]))
        stats.append(st)
    (mu_a, sig_a), (mu_b, sig_b) = stats[0].finalize(), stats[1].finalize()
    got = frechet_distance(mu_a, sig_a, mu_b, sig_b)
    want = fc.pipeline_reference()
    err = abs(got - want) / want
    print(f"distance {got!r} (float64 features {want!r}): relative error {err:.3e} (bound {fc.PIPELINE_BOUND:.1e})")
    assert want > 1.0 and err <= fc.PIPELINE_BOUND
    same = frechet_distance(mu_a, sig_a, mu_a, sig_a)
    print(f"a set against itself: {same!r}, tr sigma {float(torch.trace(sig_a))!r}")
    assert abs(same) <= 1e-6 * float(torch.trace(sig_a))
    stats[0].save(str(tmp_path / "a.npz"))
    mu_f, sig_f = FidStatistics.load(str(tmp_path / "a.npz"))
    assert torch.equal(mu_f, mu_a.cpu()) and torch.equal(sig_f, sig_a.cpu())
