"""k_linear_small (time_embed, label add, and all emb_layers as one product) through the network: it has no export of its own.  A tiny controlnet UNet -
the tiny32 golden case's construction, and the same with model_channels = 96 so that K = 96 / 384 are no multiples of 256 and the emb_layers product takes the
four-rows-per-wave form - at batch sizes on both sides of each of the kernel's three batch variants (<= 4, <= 8, <= 16), against oracle/unet_oracle.py at
the bound of tests/test_unet_gpu.py::test_unet_forward_matches_reference_golden for this net."""
import functools

import pytest
import torch

from tests.test_oracle_diffusion import load_unet_case

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
BMAX = 9


@functools.lru_cache(maxsize=None)
def _case(channels):
    """model on the device, inputs of BMAX images and the oracle's output for them (one CPU forward per config; GroupNorm is per image, so the first B images
    of the batch give the first B outputs)."""
    from humanliff_amd import synthetic as syn
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults
    from oracle import unet_oracle as uo
    g, ks, _, _, _, _, _ = load_unet_case("tiny32")
    heads, size = int(g["arg_num_heads"]), int(g["arg_image_size"])
    a = model_and_diffusion_defaults()
    a.update(dict(in_channels=27, out_channels=27, class_cond=True, num_heads=heads, rescale_timesteps=False, image_size=size, num_channels=channels,
                  num_res_blocks=int(g["arg_num_res_blocks"]), attention_resolutions=str(g["arg_attention_resolutions"])))
    model, _ = create_model_and_diffusion(**a)
    if channels != int(g["arg_num_channels"]):
        ks = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = syn.state_from_shapes(ks, seed=1)
    model.load_state_dict(sd, strict=True)
    gen = torch.Generator().manual_seed(11 + channels)
    x = torch.randn((BMAX, 27, size, size), generator=gen)
    xc = torch.randn((BMAX, 27, size, size), generator=gen).clamp(-1, 1) * 0.7
    t = torch.randint(0, 1000, (BMAX,), generator=gen)
    y = torch.randint(0, 4, (BMAX,), generator=gen)
    with torch.no_grad():
        want = uo.unet_forward(sd, x, t, xc, y, num_heads=heads)
    return model.to(dev).eval(), x, xc, t, y, want


@pytest.mark.parametrize("B", [1, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("channels", [32, 96])
def test_unet_matches_oracle_at_every_batch_variant(channels, B):
    model, x, xc, t, y, want = _case(channels)
    with torch.no_grad():
        out = model(x[:B].to(dev), t[:B].to(dev), xc[:B].to(dev), y=y[:B].to(dev)).cpu()
    err = float((out - want[:B]).abs().max())
    print(f"unet ch{channels} B{B}: max-abs {err:.2e} (outputs up to {float(want.abs().max()):.2f})")
    assert err < 1e-4
