"""The four training cases of tests/golden/gen_golden_train_variants.py (train_loss_variants.npz): their model arguments, inputs and
picked parameters, shared by the generator (reference, CPU) and the tests (tests/test_train_variants_cpu.py, tests/test_unet_train_variants_gpu.py)."""
import torch

AWARE_PICK = ["time_embed.0.weight", "input_blocks.0.0.weight", "input_blocks.1.0.out_layers.0.weight", "input_blocks.1.0.out_layers.3.weight",
              "input_blocks.3.0.emb_layers.1.bias", "middle_block.0.out_layers.0.bias", "middle_block.1.qkv.weight",
              "output_blocks.2.0.out_layers.3.bias", "output_blocks.5.0.out_layers.0.weight", "out.2.weight", "label_emb.weight",
              "input_blocks_cond.1.0.out_layers.3.bias", "input_blocks_proj_cond.2.weight"]
_T = "input_blocks.7.1.transformer_blocks.0."
XATTN_PICK = ["time_embed.0.weight", "input_blocks.0.0.weight", "conv_proj_1.weight", "linear.bias", "input_blocks.7.1.norm.weight",
              "input_blocks.7.1.proj_in.weight", _T + "norm1.weight", _T + "attn1.to_q.weight", _T + "attn1.to_v.weight", _T + "attn1.to_out.0.bias",
              _T + "norm2.weight", _T + "norm2.bias", _T + "attn2.to_q.weight", _T + "attn2.to_k.weight", _T + "attn2.to_v.weight",
              _T + "attn2.to_out.0.weight", _T + "norm3.bias", _T + "ff.net.0.proj.bias", _T + "ff.net.2.weight", "input_blocks.7.1.proj_out.weight",
              "input_blocks.7.0.out_layers.0.weight", "out.2.weight"]


def case_overrides(tag):
    """create_model_and_diffusion arguments of a case on top of model_and_diffusion_defaults() (the reference's and this package's)."""
    a = dict(out_channels=27, class_cond=True, learn_sigma=False, use_scale_shift_norm=True, rescale_timesteps=False, dropout=0.0,
             diffusion_steps=1000, noise_schedule="linear", timestep_respacing="", num_channels=32, num_res_blocks=1)
    if tag == "xattn":
        a.update(dict(in_channels=27, num_heads=2, cond_type="cross_attention", image_size=256, attention_resolutions="32,16,8"))
    else:
        cond = {"aware3d_controlnet": "controlnet", "aware3d_concat": "concat", "aware3d_plain": ""}[tag]
        a.update(dict(in_channels=18 if cond == "concat" else 9, out_channels=9, num_heads=4, cond_type=cond, use_3d_aware=True, image_size=32,
                      attention_resolutions="16,8"))
    return a


def case_inputs(tag):
    """x_start (clamped), x_cond (None for aware3d_plain), timesteps, labels and the q_sample noise of a case."""
    size, seed = (256, 17) if tag == "xattn" else (32, 13)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((2, 27, size, size), generator=g)
    xc = torch.randn((2, 27, size, size), generator=g).clamp(-1, 1) * 0.7
    noise = torch.randn((2, 27, size, size), generator=torch.Generator().manual_seed(seed + 100))
    return x.clamp(-1, 1), (None if tag == "aware3d_plain" else xc), torch.tensor([999, 17]), torch.tensor([3, 0]), noise


CASES = ("aware3d_controlnet", "aware3d_concat", "aware3d_plain", "xattn")
