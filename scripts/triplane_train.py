"""Train the tri-plane diffusion model on the HIP training path: the reference's human_diffusion/scripts/image_train.py flags that apply
here, feeding humanliff_amd.improved_diffusion.train_util.TrainLoop (fused grad-norm / clip / AdamW / EMA tail).

    python scripts/triplane_train.py --data_dir <dir with human_list.txt>/x --log_dir out --use_cond True --use_amp True \
        --microbatch 2 --batch_size 8 <model flags of triplane_scripts/*_train_*.sh>

Checkpoints (modelNNNNNN.pt, ema_<rate>_NNNNNN.pt, optNNNNNN.pt) go to --log_dir with the reference's names, so the sampler loads them;
--resume_checkpoint <log_dir>/modelNNNNNN.pt continues from one.  One GPU; under torchrun with a RCCL process group the loop wraps the
model in DDP as the reference does."""
import argparse
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from humanliff_amd.improved_diffusion.resample import create_named_schedule_sampler  # noqa: E402
from humanliff_amd.improved_diffusion.script_util import (add_dict_to_argparser, args_to_dict, create_model_and_diffusion,  # noqa: E402
                                                          model_and_diffusion_defaults)
from humanliff_amd.improved_diffusion.train_util import TrainLoop  # noqa: E402
from humanliff_amd.improved_diffusion.triplane_datasets import load_triplane_data  # noqa: E402


def main():
    args = create_argparser().parse_args()
    rank, world = 0, 1
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group(backend="nccl", world_size=world, rank=rank, timeout=datetime.timedelta(seconds=9000))
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.log_dir, exist_ok=True)
    writer = None
    if rank == 0 and args.tensorboard:
        from torch.utils.tensorboard import SummaryWriter
        writer = SummaryWriter(os.path.join(args.log_dir, "runs"))
    print("creating model and diffusion...", flush=True)
    model, diffusion = create_model_and_diffusion(**args_to_dict(args, model_and_diffusion_defaults().keys()))
    model.to(dev)
    sampler = create_named_schedule_sampler(args.schedule_sampler, diffusion)
    print("creating data loader...", flush=True)
    data = load_triplane_data(data_name=args.data_name, data_dir=args.data_dir, batch_size=args.batch_size, image_size=args.image_size,
                              class_cond=args.class_cond, layer_idx=args.layer_idx, num_subjects=args.num_subjects, world_size=world,
                              rank=rank)
    print("training...", flush=True)
    TrainLoop(model=model, diffusion=diffusion, data=data, batch_size=args.batch_size, microbatch=args.microbatch, lr=args.lr,
              ema_rate=args.ema_rate, log_interval=args.log_interval, save_interval=args.save_interval,
              resume_checkpoint=args.resume_checkpoint, use_fp16=args.use_fp16, fp16_scale_growth=args.fp16_scale_growth,
              use_amp=args.use_amp, schedule_sampler=sampler, weight_decay=args.weight_decay, lr_anneal_steps=args.lr_anneal_steps,
              use_cond=args.use_cond, writer=writer, log_dir=args.log_dir).run_loop()
    if writer is not None:
        writer.close()
    if dist.is_initialized():
        dist.destroy_process_group()


def create_argparser():
    defaults = dict(data_name="SynBody", data_dir="", log_dir="", schedule_sampler="uniform", lr=1e-4, weight_decay=0.0,
                    lr_anneal_steps=0, batch_size=1, microbatch=-1, ema_rate="0.9999", log_interval=10, save_interval=10000,
                    resume_checkpoint="", use_fp16=False, fp16_scale_growth=1e-3, use_amp=False, num_subjects=1000, layer_idx=None,
                    use_cond=False, tensorboard=False)
    defaults.update(model_and_diffusion_defaults())
    parser = argparse.ArgumentParser()
    add_dict_to_argparser(parser, defaults)
    return parser


if __name__ == "__main__":
    main()
