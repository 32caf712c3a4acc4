"""The training-loop case of tests/golden/gen_golden_train_loop.py (train_loop_tiny32.npz): the tiny32 controlnet net of
gen_golden_train_loss.py, its batches and the q_sample noise stream, shared by the generator (reference TrainLoop, CPU) and the tests."""
import torch

PICK = ["time_embed.0.weight", "time_embed.2.bias", "input_blocks.0.0.weight", "input_blocks.1.0.emb_layers.1.weight",
        "input_blocks.2.1.qkv.weight", "input_blocks_cond.1.0.out_layers.3.weight",
        "input_blocks_proj_cond.2.weight", "output_blocks.2.0.skip_connection.weight", "out.2.weight", "label_emb.weight"]
LOOP = dict(batch_size=4, microbatch=2, lr=1e-4, ema_rate="0.9999,0.99", log_interval=1, save_interval=1000, steps=3)
NP_SEED = 0
NSLICE = 1024                   # elements of each picked parameter the fixture keeps (flattened, from the start)
WDS = (0.0, 0.01)


def model_overrides():
    return dict(in_channels=27, out_channels=27, class_cond=True, learn_sigma=False, num_heads=4, use_scale_shift_norm=True,
                cond_type="controlnet", rescale_timesteps=False, dropout=0.0, diffusion_steps=1000, noise_schedule="linear",
                timestep_respacing="", image_size=32, num_channels=32, num_res_blocks=1, attention_resolutions="16,8")


def batches(steps=LOOP["steps"], B=LOOP["batch_size"], seed=21):
    """(x_start clamped, layer condition, {"y"}) per step, CPU."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        x = torch.randn((B, 27, 32, 32), generator=g).clamp(-1, 1)
        c = torch.randn((B, 27, 32, 32), generator=g).clamp(-1, 1) * 0.7
        y = torch.randint(0, 4, (B,), generator=g)
        out.append((x, c, {"y": y}))
    return out


def noise_stream(seed=11):
    """The q_sample noise of each training_losses call, in call order: a generator the caller draws microbatch shapes from."""
    return torch.Generator().manual_seed(seed)
