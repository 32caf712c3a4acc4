"""What can be said about the native LPIPS without a GPU: the float64 restatement against a twin of the package's module tree, the
test recipe's own conditions (every term contributes; the bound constants against the recomputed float32 noise), the loader against
the package's state-dict keys, and the argument checks that come before any launch."""
import os
import re

import pytest
import torch

from tests import lpips_cases as lc
from tests import lpips_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return lr.Twin(*lc.weights())


def test_restatement_equals_the_twin_module(twin):
    """The functional restatement and the module tree are the same arithmetic: the same values in float32 and in float64."""
    for name in ("16x16", "17x19", "37x50"):
        in0, in1 = lc.case(name)
        for dtype, net, (convs, lins) in ((torch.float32, twin, lc.weights()), (torch.float64, lr.Twin(*lc.weights()).double(), lc.weights64())):
            with torch.no_grad():
                val, res = net(in0.to(dtype), in1.to(dtype), retPerLayer=True)
                terms, want = lr.lpips(convs, lins, in0.to(dtype), in1.to(dtype))
            assert val.shape == (1, 1, 1, 1) and torch.equal(val, want), (name, dtype)
            for k in range(5):
                assert torch.equal(res[k], terms[k]), (name, dtype, k)
    ref = lc.reference("37x50")
    assert [tuple(f.shape[1:]) for f in ref["f0"]] == [(64, 37, 50), (128, 18, 25), (256, 9, 12), (512, 4, 6), (512, 2, 3)]


def test_every_term_contributes():
    for name in lc.CASES:
        ref = lc.reference(name)
        shares = [t / ref["total"] for t in ref["terms"]]
        print(f"{name}: total {ref['total']:.6f}, shares {[round(s, 4) for s in shares]}")
        assert min(shares) >= lc.MIN_SHARE, name
        assert 0.1 < ref["total"] < 0.5, name


def test_bound_constants_follow_the_float32_noise():
    feat, term, total = lc.float32_noise()
    print(f"float32-CPU noise: features {['%.3e' % f for f in feat]}, terms {term:.3e}, total {total:.3e}")
    for k in range(5):
        assert feat[k] <= lc.FEATURE_BOUND[k] <= 4.0 * feat[k], k
    assert term <= lc.TERM_BOUND <= 4.0 * term
    assert total <= lc.TOTAL_BOUND <= 4.0 * total


def _same_weights(model, convs, lins):
    got_convs, got_lins = model._host
    return (all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got_convs, convs)) and len(got_convs) == 13
            and all(torch.equal(a, b.reshape(-1)) for a, b in zip(got_lins, lins)) and len(got_lins) == 5)


def test_loader_takes_the_package_keys(twin, tmp_path):
    from humanliff_amd.lpips import SCALE, SHIFT, LpipsVGG
    convs, lins = lc.weights()
    sd = twin.state_dict()
    assert "net.slice3.14.bias" in sd and "lin2.model.1.weight" in sd and "lins.2.model.1.weight" in sd and "scaling_layer.shift" in sd
    assert sum(k.startswith("net.") for k in sd) == 26
    both = LpipsVGG.from_state_dict(sd)
    assert _same_weights(both, convs, lins)
    assert both.shift == pytest.approx(SHIFT, rel=1e-6) and both.scale == pytest.approx(SCALE, rel=1e-6)
    only_lin = {k: v for k, v in sd.items() if not k.startswith(("lins.", "scaling_layer."))}
    only_lins = {k: v for k, v in sd.items() if not re.match(r"lin\d", k)}
    assert _same_weights(LpipsVGG.from_state_dict(only_lin), convs, lins) and LpipsVGG.from_state_dict(only_lin).shift == SHIFT
    assert _same_weights(LpipsVGG.from_state_dict(only_lins), convs, lins)
    # the two-file form: torchvision's features.{i} names plus the package's lin file
    it = iter(convs)
    vgg = {}
    for idx in lr.CONV_INDEX:
        for i in idx:
            vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"] = next(it)
    vgg["classifier.0.weight"] = torch.zeros(2, 2)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": lins[k] for k in range(5)}, tmp_path / "vgg.pth")
    assert _same_weights(LpipsVGG.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")), convs, lins)
    del vgg["features.19.bias"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    with pytest.raises(KeyError, match=r"features\.19\.bias"):
        LpipsVGG.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))


def test_loader_names_missing_and_misshaped_keys(twin):
    from humanliff_amd.lpips import LpipsVGG
    sd = dict(twin.state_dict())
    with pytest.raises(KeyError, match=r"net\.slice4\.21\.weight"):
        LpipsVGG.from_state_dict({k: v for k, v in sd.items() if k != "net.slice4.21.weight"})
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight.*lins\.3\.model\.1\.weight"):
        LpipsVGG.from_state_dict({k: v for k, v in sd.items() if k not in ("lin3.model.1.weight", "lins.3.model.1.weight")})
    with pytest.raises(ValueError, match=r"net\.slice2\.5\.weight"):
        LpipsVGG.from_state_dict({**sd, "net.slice2.5.weight": sd["net.slice2.5.weight"][:, :32]})
    with pytest.raises(ValueError, match=r"net\.slice1\.0\.bias"):
        LpipsVGG.from_state_dict({**sd, "net.slice1.0.bias": sd["net.slice1.0.bias"][None]})
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        LpipsVGG.from_state_dict({**sd, "lin1.model.1.weight": sd["lin1.model.1.weight"].reshape(-1)})
    with pytest.raises(KeyError, match=r"scaling_layer\.scale"):
        LpipsVGG.from_state_dict({k: v for k, v in sd.items() if k != "scaling_layer.scale"})
    with pytest.raises(ValueError, match=r"scaling_layer\.shift"):
        LpipsVGG.from_state_dict({**sd, "scaling_layer.shift": [-.030, -.088, -.188]})
    with pytest.raises(ValueError, match=r"scaling_layer\.scale"):
        LpipsVGG.from_state_dict({**sd, "scaling_layer.scale": sd["scaling_layer.scale"].reshape(3)})
    with pytest.raises(RuntimeError, match="no CPU path"):
        LpipsVGG.from_state_dict(sd, device="cpu")


def test_arguments_are_checked_before_any_launch(twin):
    from humanliff_amd.lpips import LpipsVGG
    model = LpipsVGG.from_state_dict(twin.state_dict())
    x = torch.zeros(3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.features(x[None])
    for bad in (torch.zeros(3, 15, 32), torch.zeros(2, 3, 16, 15)):
        with pytest.raises(ValueError, match="15"):
            model(bad, bad)
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 32, 32), torch.zeros(1, 32, 32))
    with pytest.raises(RuntimeError):
        model(x.double(), x.double())
    assert model._params is None, "nothing was uploaded or launched"


def test_header_declares_the_exports():
    from humanliff_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "humanliff_hip.h")).read()
    for name in ("hl_lpips", "hl_lpips_features", "hl_lpips_workspace_bytes", "hl_lpips_tap_shape"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # below 16 on a side, or no images: no workspace; bad arguments come back as a status, before any launch
    assert L.hl_lpips_workspace_bytes(2, 15, 64) == 0 and L.hl_lpips_workspace_bytes(2, 64, 15) == 0 and L.hl_lpips_workspace_bytes(0, 64, 64) == 0
    taps = sum(2 * (37 >> k) * (50 >> k) * c * 4 for k, c in enumerate(lr.TAP_CHANNELS))
    assert L.hl_lpips_workspace_bytes(2, 37, 50) >= taps + 2 * 2 * 37 * 50 * 64 * 4
    assert L.hl_lpips(None, None, None, 1, 32, 32, None, None, 0, None) < 0
    assert b"hl_lpips" in L.hl_last_error()
