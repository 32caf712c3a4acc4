"""The PyTorch-op twin (tests/unet_autograd_twin.py) as a statement of the reference's BACKWARD for the 3-D-aware and cross-attention
UNets: training_losses + loss.mean().backward() through the twin equal the reference's losses and parameter gradients
(tests/golden/gen_golden_train_variants.py).  CPU; tests/test_unet_train_variants_gpu.py holds the HIP training path to the same vectors."""
import os

import numpy as np
import pytest
import torch
from tests.train_variants_cases import CASES, case_inputs, case_overrides
from tests.unet_autograd_twin import forward_autograd

from tests.golden_util import GOLDEN
from humanliff_amd import synthetic as syn
from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults


def build(tag):
    a = model_and_diffusion_defaults()
    a.update(case_overrides(tag))
    model, diffusion = create_model_and_diffusion(**a)
    ks = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(syn.state_from_shapes(ks, 1), strict=True)
    return model.train(), diffusion


@pytest.mark.parametrize("tag", CASES)
def test_twin_training_gradients_match_reference(tag):
    g = np.load(os.path.join(GOLDEN, "train_loss_variants.npz"))
    model, diffusion = build(tag)
    sd = dict(model.named_parameters())
    assert len(sd) == int(g[f"{tag}_nparams"])
    x0, xc, t, y, noise = case_inputs(tag)
    losses = diffusion.training_losses(lambda *a, **k: forward_autograd(model, *a, **k), x0, xc, t, model_kwargs={"y": y}, noise=noise)
    assert np.abs(losses["loss"].detach().numpy() - g[f"{tag}_loss"]).max() < 1e-5
    losses["loss"].mean().backward()
    assert all(p.grad is not None for p in sd.values())
    tot = sum(float(p.grad.double().abs().sum()) for p in sd.values())
    assert abs(tot - float(g[f"{tag}_grad_abs_sum"])) < 1e-4 * float(g[f"{tag}_grad_abs_sum"])
    zeros = 0
    for k in map(str, g[f"{tag}_keys"]):
        ref = torch.from_numpy(g[f"{tag}_g_{k}"])
        if not ref.abs().max() > 0:          # attn2.to_q / to_k / norm2: exact zeros in the reference and in the twin
            assert torch.equal(sd[k].grad, torch.zeros_like(ref)), k
            zeros += 1
            continue
        assert (sd[k].grad - ref).abs().max() < 1e-6 + 1e-4 * ref.abs().max(), k
    assert zeros == (4 if tag == "xattn" else 0)
