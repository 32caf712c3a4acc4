"""A SynBody directory tree -> a prepared ViewStore: the dataset half of recon_NeRF/lib/SynBody_dataset.py (SynBodyDatasetBatch) of the
reference, for the device-resident fitting path (contract: DESIGN.md 4i).

    index = SynBodyIndex(data_root, multi_person=True, num_instance=2, pose_start=0, pose_interval=5, poses_num=1, views_num=185)
    store = load_view_store(index, load_body_model(smpl_path), image_scaling=0.5)           # decoded, resized and prepared on the device
    FitLoop(renderer, RayBatchLoader(store, batch_size=2, n_rays=2048), ...).run_loop()

The reference decodes, masks and resizes one image per __getitem__ call in a DataLoader worker (imageio + cv2, :266-278) and draws its rays
there.  Here every view is decoded once (PIL, a bounded thread pool), uploaded as uint8 and turned into the store's float image and body
mask by one launch per batch (humanliff_amd.view_ingest); rays are drawn on the device afterwards (if_nerf_data_utils.sample_ray_batch).
SynBodyIndex, smpl_params and smplx_params are host code and need neither a GPU nor PIL.  smpl_type 'smplx' (the reference's default,
:44) reads <subject>/smplx.npz and poses a humanliff_amd.body.SmplxModel of the file's gender; the TightCap layout is
TightCap_dataset.py's, which reuses the readers and helpers below.
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import view_ingest
from .if_nerf_data_utils import ViewStore

LAYER_DIRS = ('person', 'person-pants', 'person-pants-shirt', 'person-pants-shirt-shoes')          # cloth_layer_index 0 .. 3 (:253-264)
SMPL_FILE = os.path.join('person-top-bottom-shoes', 'outputs_re_fitting', 'refit_smpl_2nd.npz')    # :283
SMPLX_FILE = 'smplx.npz'                                                                            # :285
MAX_DECODE_THREADS = 16
UPLOAD_BYTES = 256 << 20                 # uint8 source bytes uploaded and ingested per batch


class SynBodyIndex:
    """The file and camera of every dataset index, with the index arithmetic of SynBodyDatasetBatch (:44-77, 238-272, 354-355)."""

    def __init__(self, data_root, multi_person=True, num_instance=1, pose_start=0, pose_interval=5, poses_num=1, views_num=185, layer_idx=None):
        self.data_root, self.multi_person, self.num_instance = data_root, multi_person, int(num_instance)
        self.views_num = int(views_num)
        self.cloth_layer_num = 4 if layer_idx is None else 1
        self.i, self.i_intv, self.ni = int(pose_start), int(pose_interval), int(poses_num)
        self.layer_idx = layer_idx
        parent = os.path.dirname(data_root)                           # human_list.txt lies beside the subjects' directories (:65-66)
        self.human_list = os.path.join(parent, 'human_list.txt')
        with open(self.human_list) as f:                              # (read even for a single subject, as the reference does)
            names = [line.strip() for line in f.readlines()[:self.num_instance]]
        self.root_list = [os.path.join(parent, n) for n in names] if multi_person else [data_root]
        self.cams_all = []
        for root in self.root_list:
            with open(os.path.join(root, 'cameras.json')) as f:
                self.cams_all.append(json.load(f))

    def __len__(self):
        return self.num_instance * self.cloth_layer_num * self.ni * self.views_num

    def indices(self, index):
        """(instance_idx, cloth_layer_index, pose_index, view_index) of a dataset index (:238-246)."""
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
        """(instance_idx, cloth_layer_index, pose_index, view_index, img_path, mask_path, K (3,3), R (3,3), T (3,1)) - K unscaled.  The image
        is `{pppp}.jpg` as in the reference, or `{pppp}.png` where only that exists."""
        instance_idx, cloth_layer_index, pose_index, view_index = self.indices(index)
        root = self.root_list[instance_idx]
        camera, frame = f'camera{str(view_index).zfill(4)}', str(pose_index).zfill(4)
        layer_dir = os.path.join(root, LAYER_DIRS[cloth_layer_index])
        img_path = os.path.join(layer_dir, 'img', camera, frame + '.jpg')
        if not os.path.exists(img_path) and os.path.exists(img_path[:-4] + '.png'):
            img_path = img_path[:-4] + '.png'
        mask_path = os.path.join(layer_dir, 'mask', camera, frame + '.png')
        cam = self.cams_all[instance_idx][camera]
        K, R, T = np.array(cam['K'], dtype=np.float64), np.array(cam['R'], dtype=np.float64), np.array(cam['T'], dtype=np.float64).reshape(-1, 1)
        return instance_idx, cloth_layer_index, pose_index, view_index, img_path, mask_path, K, R, T

    def smpl_path(self, instance_idx):
        return os.path.join(self.root_list[instance_idx], SMPL_FILE)

    def smplx_path(self, instance_idx):
        return os.path.join(self.root_list[instance_idx], SMPLX_FILE)                # :285


def smpl_params(smpl_path, pose_index, smpl_type='smpl'):
    """prepare_smpl_params (:135-144) for smpl_type 'smpl': float32 numpy 'shapes' (betas), 'poses' (1, 72), 'R' = I and 'Th' = transl[0:1] -
    the reference takes the FIRST frame's translation whatever pose_index is, and so does this."""
    if smpl_type != 'smpl':
        raise NotImplementedError(f"smpl_params: smpl_type {smpl_type!r} needs the smplx package's body model, which this project does not "
                                  "have; only 'smpl' is restated")
    with np.load(smpl_path, allow_pickle=True) as z:
        fitted = z['smpl'].item()
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    poses = np.concatenate([f32(fitted['global_orient'][pose_index]).reshape(1, 3), f32(fitted['body_pose'][pose_index]).reshape(1, -1)], axis=1)
    if poses.shape != (1, 72):
        raise ValueError(f"{smpl_path}: global_orient and body_pose of frame {pose_index} hold {poses.shape[1]} values, SMPL has 72")
    return {'shapes': f32(fitted['betas']), 'poses': poses, 'R': np.eye(3, dtype=np.float32), 'Th': f32(fitted['transl'][0:1])}


def smplx_params(smplx_path, pose_index):
    """prepare_smpl_params (:145-155) for smpl_type 'smplx' -> (params, gender): every key of the file's 'smplx' dict as a torch tensor,
    'betas' whole and every other key [pose_index:pose_index + 1]; 'R' = I, 'Th' = zeros (1, 3) (float32 numpy); gender from 'meta'."""
    with np.load(smplx_path, allow_pickle=True) as z:
        fitted, gender = z['smplx'].item(), z['meta'].item()['gender']
    params = {k: torch.from_numpy(np.asarray(v) if k == 'betas' else np.asarray(v)[pose_index:pose_index + 1]) for k, v in fitted.items()}
    params['R'] = np.eye(3).astype(np.float32)
    params['Th'] = np.zeros((1, 3)).astype(np.float32)
    return params, gender


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("reading SynBody images needs Pillow (PIL), the only decoder this loader uses; install it, or decode the files "
                          "yourself and fill a ViewStore through humanliff_amd.view_ingest.ingest_views") from e
    return Image


def read_image(path):
    """(H, W, 3) uint8 RGB, as imageio.imread gives for the dataset's JPEG / PNG files (:266)."""
    with _pil().open(path) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


def read_mask(path):
    """(H, W) uint8, non-zero where the file is (get_mask :130-133 sets those pixels to 255)."""
    with _pil().open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2:
        raise ValueError(f"{path}: the mask has {a.shape[2] if a.ndim == 3 else '?'} channels; a single-channel image is expected")
    return (a != 0).astype(np.uint8) * np.uint8(255)


def store_bytes(V, H, W):
    """Device bytes of a prepared ViewStore of V float32 views: image 12 + body 1 per pixel, the two class bitmaps and the row tables."""
    return V * (H * W * 13 + 2 * H * ((W + 63) // 64) * 8 + 2 * (H + 1) * 4)


def scaled_size(Hs, Ws, image_scaling):
    return int(Hs * image_scaling), int(Ws * image_scaling)          # :276, Python float arithmetic


def scaled_intrinsics(K, image_scaling):
    """K (..., 3, 3) with its first two rows multiplied by image_scaling (:279); a float64 copy."""
    K = np.array(K, dtype=np.float64)
    K[..., :2, :] = K[..., :2, :] * image_scaling
    return K


def store_test_views(store, view_ids=None):
    """The stored views as evaluate_views' tp_input dicts, one per view (ViewStore.test_view: the reference's split != 'train' tuple).
    `view_ids`: the id reported for each view (default: its position in the store)."""
    pose_index = getattr(store, "pose_index", None)
    for v in range(len(store)):
        rgb, ray_o, ray_d, near, far, _, mask_at_box, _ = store.test_view(v)
        yield {"rgb_all": rgb[None, None], "ray_o_all": ray_o[None, None], "ray_d_all": ray_d[None, None], "near_all": near[None, None, :, None],
               "far_all": far[None, None, :, None], "mask_at_box_all": mask_at_box[None, None], "instance_idx": store.instance_idx[v:v + 1],
               "cloth_layer_index": store.cloth_layer_index[v:v + 1], "pose_index": torch.tensor([0 if pose_index is None else int(pose_index[v])]),
               "world_bounds": store.world_bounds[v:v + 1], "view_id": v if view_ids is None else int(view_ids[v]), "H": store.H, "W": store.W}


def load_view_store(index, body_model, image_scaling=1.0, device=None, items=None, decode_threads=8, smpl_type='smpl'):
    """Every dataset index in `items` (default: all of `index`) as one view of a prepared ViewStore on `device`, in that order: image
    and mask resized to int(Hs * image_scaling) x int(Ws * image_scaling) as :266-278 does, K[:2] scaled (:279), world bounds from
    body_model.pose of smpl_params (prepare_input :158-194).  The store also carries `dataset_index`, `pose_index` and `view_index`
    (host int64 arrays, one entry per view).  MemoryError before anything is decoded when the store would not fit the free device
    memory; ValueError for a file of another size than the first, and for image_scaling > 1.
    smpl_type 'smplx': `body_model` is a SmplxModel, or a dict of them keyed 'male' / 'female' / 'neutral' as the reference keeps them
    (:84-99); the bounds come from SmplxModel.pose_dict of smplx_params (index.smplx_path), with the model of the file's gender - KeyError
    naming the gender when the dict lacks it."""
    if smpl_type not in ('smpl', 'smplx'):
        raise ValueError(f"load_view_store: smpl_type {smpl_type!r}; 'smpl' or 'smplx'")

    def smplx_bounds(inst, pose, device):
        params, gender = smplx_params(index.smplx_path(inst), pose)
        if isinstance(body_model, dict):
            if gender not in body_model:
                raise KeyError(f"load_view_store: {index.smplx_path(inst)} is of gender {gender!r}; body_model holds {sorted(body_model)}")
            model = body_model[gender]
        else:
            model = body_model
        return model.pose_dict({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in params.items()}, y_margin=0.05).world_bounds[0]

    def ingest(recs, decoded, H, W, device):
        img = torch.from_numpy(np.stack([d[rec[4]] for rec, d in zip(recs, decoded)])).to(device)
        msk = torch.from_numpy(np.stack([d[rec[5]] for rec, d in zip(recs, decoded)])).to(device)
        return view_ingest.ingest_views(img, msk, H, W)

    return fill_view_store(index, body_model, image_scaling, device, items, decode_threads, source_bytes=4, y_margin=0.05,
                           decode=lambda rec: {rec[4]: read_image(rec[4]), rec[5]: read_mask(rec[5])}, ingest=ingest,
                           pose_bounds=smplx_bounds if smpl_type == 'smplx' else None)


def fill_view_store(index, body_model, image_scaling, device, items, decode_threads, source_bytes, y_margin, decode, ingest, pose_bounds=None):
    """What the loaders of the two dataset layouts share.  `index.item(i)` gives (instance_idx, cloth_layer_index, pose_index, view_index,
    img_path, ..., K, R, T) and `index.smpl_path`; `decode(rec)` -> {path: uint8 array} of the files the view names (called in the thread
    pool); `ingest(recs, decoded, H, W, device)` -> (image (V, H, W, 3) float32, body (V, H, W) uint8) of one batch on the device;
    `source_bytes`: uint8 bytes uploaded per source pixel; `y_margin`: BodyModel.pose's; `pose_bounds(inst, pose, device)` -> (2, 3)
    device tensor: the world bounds of a posed subject where they do not come from body_model.pose of smpl_params."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_view_store needs a HIP device; humanliff_amd has no CPU path")
    items = list(range(len(index))) if items is None else [int(i) for i in items]
    if not items:
        raise ValueError("load_view_store: no items")
    records = [index.item(i) for i in items]
    with _pil().open(records[0][4]) as im:                            # (the header only)
        Ws, Hs = im.size
    H, W = scaled_size(Hs, Ws, image_scaling)
    view_ingest.check_sizes(Hs, Ws, H, W)
    V = len(records)
    per_batch = max(1, min(V, UPLOAD_BYTES // (Hs * Ws * source_bytes)))
    free = torch.cuda.mem_get_info(device)[0]
    staging = per_batch * (Hs * Ws * source_bytes + H * W * 13)       # a batch's uint8 source and its output before torch.cat
    if store_bytes(V, H, W) + staging > free:
        fit = max(0, (free - staging) // store_bytes(1, H, W))
        raise MemoryError(f"load_view_store: {V} views of {H} x {W} need {store_bytes(V, H, W) + staging} bytes on {device}, "
                          f"{free} are free: {fit} views would fit (pass fewer `items`, or a smaller image_scaling)")
    # world bounds: one posed body per (subject, pose)
    bounds = {}
    for inst, _, pose, *_ in records:
        if (inst, pose) in bounds:
            continue
        if pose_bounds is not None:
            bounds[(inst, pose)] = pose_bounds(inst, pose, device)
        else:
            p = smpl_params(index.smpl_path(inst), pose)
            posed = body_model.pose(torch.from_numpy(p['poses']).to(device), torch.from_numpy(p['shapes'].reshape(-1)).to(device), p['R'], p['Th'],
                                    y_margin=y_margin)
            bounds[(inst, pose)] = posed.world_bounds[0]
    bounds = {k: b.double().cpu().numpy() for k, b in bounds.items()}

    def decode_checked(rec):
        out = decode(rec)
        for path, a in out.items():
            if a.shape[:2] != (Hs, Ws):
                raise ValueError(f"{path} is {a.shape[0]} x {a.shape[1]}; the views of a store have one size and the first is {Hs} x {Ws}")
        return out

    store = ViewStore(H, W, device)
    with ThreadPoolExecutor(max_workers=max(1, min(int(decode_threads), MAX_DECODE_THREADS))) as pool:
        for b0 in range(0, V, per_batch):
            recs = records[b0:b0 + per_batch]
            image, body = ingest(recs, list(pool.map(decode_checked, recs)), H, W, device)
            K = scaled_intrinsics(np.stack([r[6] for r in recs]), image_scaling)
            store.add(image, body, K, np.stack([r[7] for r in recs]), np.stack([r[8] for r in recs]),
                      np.stack([bounds[(r[0], r[2])] for r in recs]), [r[0] for r in recs], [r[1] for r in recs])
    store.prepare()
    store.dataset_index = np.asarray(items, dtype=np.int64)
    store.pose_index = np.asarray([r[2] for r in records], dtype=np.int64)
    store.view_index = np.asarray([r[3] for r in records], dtype=np.int64)
    return store
