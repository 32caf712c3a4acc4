"""A TightCap directory tree -> a prepared ViewStore: the dataset half of recon_NeRF/lib/TightCap_dataset.py (TightCapDatasetBatch) of the
reference, for the device-resident fitting path (contract: DESIGN.md 4j).

    index = TightCapIndex(data_root, multi_person=True, num_instance=2, pose_start=0, pose_interval=5, poses_num=1, views_num=382)
    store = load_view_store(index, load_body_model(smpl_path), image_scaling=1.0)
    FitLoop(renderer, RayBatchLoader(store, batch_size=2, n_rays=2048), ...).run_loop()

TightCap ships one photograph per view and no image per cloth layer: the reference builds each layer's image in a DataLoader worker from
the photograph and up to five masks (:233-298) - garment-only pixels zeroed, a fixed skin colour where body and garment overlap, the cut to
the full mask, the layer's body mask derived from what is left - and resizes both with cv2.  Here every file a layer names is decoded once
(PIL, a bounded thread pool), uploaded as uint8, and one launch per batch composes, reduces and derives the mask on the device
(humanliff_amd.view_ingest.ingest_layered_views).  The world bounds pad y by a further 0.1 (:165-168), not SynBody's 0.05.
TightCapIndex is host code and needs neither a GPU nor PIL.  smpl_type 'smplx' is not covered.
"""
import json
import os

import numpy as np
import torch

from ... import view_ingest
from .SynBody_dataset import (fill_view_store, read_image, read_mask, scaled_intrinsics, scaled_size, smpl_params, store_bytes,  # noqa: F401
                              store_test_views)

FULL_DIR = 'person-top-bottom-shoes'                                             # the photograph, the full mask, cameras.json and the SMPL fit
PLANE_DIRS = {'full': FULL_DIR, 'person': 'person', 'top': 'top', 'bottom': 'bottom', 'shoes': 'shoes'}
SMPL_FILE = os.path.join(FULL_DIR, 'outputs_re_fitting', 'refit_smpl_2nd.npz')  # :313
Y_MARGIN = 0.1                                                                   # :167-168
SOURCE_BYTES = 8                                                                 # uint8 source bytes per pixel: 3 of image, 5 planes


class TightCapIndex:
    """The files and camera of every dataset index, with the index arithmetic of TightCapDatasetBatch (:20-53, 218-226, 233-315)."""

    def __init__(self, data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=5, poses_num=1, views_num=382, smpl_type='smpl',
                 layer_idx=None):
        if smpl_type != 'smpl':
            raise NotImplementedError(f"TightCapIndex: smpl_type {smpl_type!r} needs the smplx package's body model, which this project does "
                                      "not have; only 'smpl' is restated")
        if layer_idx is not None and not 0 <= int(layer_idx) <= 3:
            raise ValueError(f"TightCapIndex: cloth layers are 0 .. 3, got layer_idx {layer_idx}")
        self.data_root, self.multi_person, self.num_instance = data_root, multi_person, int(num_instance)
        self.views_num = int(views_num)
        self.cloth_layer_num = 4 if layer_idx is None else 1
        self.i, self.i_intv, self.ni = int(pose_start), int(pose_interval), int(poses_num)
        self.layer_idx = None if layer_idx is None else int(layer_idx)
        parent = os.path.dirname(data_root)                           # TightCap_human_list.txt lies beside the subjects' directories (:41-42)
        self.human_list = os.path.join(parent, 'TightCap_human_list.txt')
        with open(self.human_list) as f:                              # (read even for a single subject, as the reference does)
            names = [line.strip() for line in f.readlines()[:self.num_instance]]
        self.root_list = [os.path.join(parent, n) for n in names] if multi_person else [data_root]
        self.cams_all = []
        for root in self.root_list:
            with open(os.path.join(root, FULL_DIR, 'cameras.json')) as f:
                self.cams_all.append(json.load(f))

    def __len__(self):
        return self.num_instance * self.cloth_layer_num * self.ni * self.views_num

    def indices(self, index):
        """(instance_idx, cloth_layer_index, pose_index, view_index) of a dataset index (:218-226)."""
        nv, per_layer = self.views_num, self.ni * self.views_num
        per_instance = self.cloth_layer_num * per_layer
        instance_idx = index // per_instance if self.multi_person else 0
        cloth_layer_index = (index - instance_idx * per_instance) // per_layer
        pose_index = (index - instance_idx * per_instance - cloth_layer_index * per_layer) // nv * self.i_intv + self.i
        view_index = index % nv
        if self.layer_idx is not None:
            cloth_layer_index = self.layer_idx
        return instance_idx, cloth_layer_index, pose_index, view_index

    def item(self, index):
        """(instance_idx, cloth_layer_index, pose_index, view_index, img_path, mask_paths, K (3,3), R (3,3), T (3,1)) - K unscaled.
        mask_paths: {plane: path} of the masks the layer's rule names and no other (view_ingest.LAYER_PLANES).  The image is `{pppp}.jpg`
        as in the reference, or `{pppp}.png` where only that exists.  ValueError for a cloth layer outside 0 .. 3 (the reference would
        leave `img` undefined there)."""
        instance_idx, cloth_layer_index, pose_index, view_index = self.indices(index)
        if not 0 <= cloth_layer_index <= 3:
            raise ValueError(f"TightCapIndex: dataset index {index} is cloth layer {cloth_layer_index}; the layers are 0 .. 3")
        root = self.root_list[instance_idx]
        camera, frame = f'camera{str(view_index).zfill(4)}', str(pose_index).zfill(4)
        img_path = os.path.join(root, FULL_DIR, 'img', camera, frame + '.jpg')
        if not os.path.exists(img_path) and os.path.exists(img_path[:-4] + '.png'):
            img_path = img_path[:-4] + '.png'
        mask_paths = {n: os.path.join(root, PLANE_DIRS[n], 'mask', camera, frame + '.png') for n in view_ingest.LAYER_PLANES[cloth_layer_index]}
        cam = self.cams_all[instance_idx][camera]
        K, R, T = np.array(cam['K'], dtype=np.float64), np.array(cam['R'], dtype=np.float64), np.array(cam['T'], dtype=np.float64).reshape(-1, 1)
        return instance_idx, cloth_layer_index, pose_index, view_index, img_path, mask_paths, K, R, T

    def smpl_path(self, instance_idx):
        return os.path.join(self.root_list[instance_idx], SMPL_FILE)


def load_view_store(index, body_model, image_scaling=1.0, device=None, items=None, decode_threads=8):
    """Every dataset index in `items` (default: all of `index`) as one view of a prepared ViewStore on `device`, in that order: each
    view's layer image composed from its photograph and masks (:233-298), image and derived mask resized to int(Hs * image_scaling) x
    int(Ws * image_scaling) (:305-308), K[:2] scaled (:309), world bounds from body_model.pose of smpl_params with y padded by 0.15 in all
    (prepare_input :135-171).  The store also carries `dataset_index`, `pose_index` and `view_index` (host int64 arrays, one entry per
    view).  MemoryError before anything is decoded when the store would not fit the free device memory; ValueError for a file of another
    size than the first, for image_scaling > 1 and for a cloth layer outside 0 .. 3."""
    def decode(rec):
        out = {rec[4]: read_image(rec[4])}
        out.update({path: read_mask(path) for path in rec[5].values()})
        return out

    def ingest(recs, decoded, H, W, device):
        layers = [rec[1] for rec in recs]
        img = torch.from_numpy(np.stack([d[rec[4]] for rec, d in zip(recs, decoded)])).to(device)
        blank = np.zeros(img.shape[1:3], dtype=np.uint8)              # for a view that does not read the plane: never looked at
        masks = {n: torch.from_numpy(np.stack([d[rec[5][n]] if n in rec[5] else blank for rec, d in zip(recs, decoded)])).to(device)
                 for n in view_ingest.planes_read(layers)}
        return view_ingest.ingest_layered_views(img, masks, layers, H, W)

    return fill_view_store(index, body_model, image_scaling, device, items, decode_threads, source_bytes=SOURCE_BYTES, y_margin=Y_MARGIN,
                           decode=decode, ingest=ingest)
