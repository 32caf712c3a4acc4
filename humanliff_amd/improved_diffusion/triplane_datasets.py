"""Tri-plane training data (human_diffusion/improved_diffusion/triplane_datasets.py load_triplane_data) without blobfile, cv2 or SMPL.

`data_dir` names a file inside the directory that holds `human_list.txt` (one tri-plane checkpoint per line, relative to that directory:
the `.tar` files the fitting stage saves, torch.save dicts with ['network_fn_state_dict']['tri_planes']).  Item idx is subject idx // 4,
layer idx % 4 (or the fixed layer_idx): (tri_planes[layer], tri_planes[layer - 1] or zeros for layer 0, {"y": layer}), each plane
reshaped from (L, 1, C, H, W)-style checkpoints to (L, C', H, W) as the reference does.  SynBody and TightCap read the same layout.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

LAYERS = 4


def load_triplane_data(*, data_name, data_dir, batch_size, image_size, class_cond=False, num_subjects=1000, layer_idx=None,
                       deterministic=False, world_size=1, rank=0, num_workers=3):
    """Endless generator of (tri-planes, layer condition, {"y": layer}) batches, as the reference's."""
    if not data_dir:
        raise ValueError("unspecified data directory")
    if data_name not in ("SynBody", "tightcap"):
        raise ValueError(f"unknown data_name {data_name!r} (SynBody, tightcap)")
    dataset = TriplaneDataset(image_size, data_dir, num_subjects, layer_idx=layer_idx)
    if deterministic:
        loader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=0, drop_last=True)
    else:
        sampler = DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=True)
        loader = DataLoader(dataset, sampler=sampler, batch_size=batch_size, num_workers=num_workers, drop_last=False, pin_memory=True)
    while True:
        yield from loader


class TriplaneDataset(Dataset):
    def __init__(self, resolution, data_dir, num_subjects, classes=None, layer_idx=None):
        super().__init__()
        self.resolution = resolution
        self.layer_idx = layer_idx
        self.num_subjects = num_subjects
        self.layer_num = LAYERS
        root = os.path.dirname(data_dir)
        with open(os.path.join(root, "human_list.txt")) as f:
            self.tri_plane_lst = [os.path.join(root, line.strip()) for line in f.readlines()[:num_subjects]]

    def __len__(self):
        return self.num_subjects * self.layer_num

    def __getitem__(self, idx):
        subject, layer = idx // self.layer_num, idx % self.layer_num
        if self.layer_idx is not None:
            layer = int(self.layer_idx)
        tp = torch.load(self.tri_plane_lst[subject], map_location="cpu")["network_fn_state_dict"]["tri_planes"].squeeze(0)
        tp = tp.reshape(tp.shape[0], -1, *tp.shape[-2:])
        cond = torch.zeros(tp.shape[1:], dtype=tp.dtype) if layer == 0 else tp[layer - 1]
        return tp[layer], cond, {"y": np.array(layer, dtype=np.int64)}


SynBodyDataset = TightCapDataset = TriplaneDataset
