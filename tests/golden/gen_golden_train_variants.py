"""Generate golden vectors for training the 3-D-aware and cross-attention UNets FROM THE REFERENCE: GaussianDiffusion.training_losses
(gaussian_diffusion.py:688-772) with autograd on use_3d_aware=True (unet.py:158-166, 208-214, 566-570, 613-614) and on
cond_type='cross_attention' (unet.py:404-405, 579-582; spatial_transformer.py:115-178), then loss.mean().backward().  Runs only where
the reference is importable (CPU).

    python tests/golden/gen_golden_train_variants.py

Cases (the nets of tests/golden/gen_golden_variants.py): aware3d_controlnet / aware3d_concat / aware3d_plain, 32 px, 9-channel planes;
xattn, the narrow 256 px net.  Per case the fixture holds the losses, the sum of |grad| over every parameter and about ten picked
parameter gradients; for xattn these include attn2.to_q / to_k and norm2, whose gradients are exact zeros (the softmax over the single
context token is 1).  Weights, inputs and the q_sample noise are rebuilt from seeds (humanliff_amd.synthetic, torch.Generator) by the tests.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference/human_diffusion")

from improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults  # noqa: E402

from humanliff_amd import synthetic as syn  # noqa: E402
from tests.train_variants_cases import AWARE_PICK, CASES, XATTN_PICK, case_inputs, case_overrides  # noqa: E402

if __name__ == "__main__":
    out = {}
    for tag in CASES:
        a = model_and_diffusion_defaults()
        a.update(case_overrides(tag))
        model, diffusion = create_model_and_diffusion(**a)
        ks = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict(syn.state_from_shapes(ks, 1), strict=True)
        model.train()
        x0, xc, t, y, noise = case_inputs(tag)
        losses = diffusion.training_losses(model, x0, xc, t, model_kwargs={"y": y}, noise=noise)
        losses["loss"].mean().backward()
        sd = dict(model.named_parameters())
        pick = [k for k in (XATTN_PICK if tag == "xattn" else AWARE_PICK) if k in sd]
        assert len(pick) >= 10, (tag, pick)
        assert all(sd[k].grad is not None for k in sd), tag
        tot = sum(float(p.grad.double().abs().sum()) for p in sd.values())
        out[f"{tag}_loss"] = losses["loss"].detach().numpy()
        out[f"{tag}_grad_abs_sum"] = np.float64(tot)
        out[f"{tag}_nparams"] = len(sd)
        out[f"{tag}_keys"] = np.array(pick)
        for k in pick:
            out[f"{tag}_g_{k}"] = sd[k].grad.numpy()
        print(tag, "loss", losses["loss"].tolist(), "grad abs sum", tot, "zero grads",
              [k for k in pick if not sd[k].grad.abs().max() > 0])
    np.savez_compressed(os.path.join(HERE, "train_loss_variants.npz"), **out)
