"""A small SynBody-shaped directory tree written with PIL, for tests/test_synbody_dataset_cpu.py and tests/test_synbody_dataset_gpu.py:
human_list.txt, per subject cameras.json (orbit cameras of humanliff_amd.synthetic) and the SMPL parameter file, per cloth layer
img/camera{vvvv}/{pppp}.jpg|.png and mask/camera{vvvv}/{pppp}.png."""
import json
import os

import numpy as np

from humanliff_amd import synthetic as syn

LAYER_DIRS = ('person', 'person-pants', 'person-pants-shirt', 'person-pants-shirt-shoes')
SMPL_FILE = os.path.join('person-top-bottom-shoes', 'outputs_re_fitting', 'refit_smpl_2nd.npz')


def orbit_cameras(n_views, size):
    cams = {}
    for v in range(n_views):
        K, c2w, cam = syn.orbit_camera(v, n_views, size, size)
        R = c2w.T
        cams[f'camera{v:04d}'] = {'K': K.tolist(), 'R': R.tolist(), 'T': (-R @ cam).tolist()}
    return cams


def smpl_file_content(n_poses, seed):
    rng = np.random.default_rng(seed)
    return {'betas': (rng.standard_normal((1, 10)) * 0.5).astype(np.float32),
            'global_orient': (rng.standard_normal((n_poses, 3)) * 0.1).astype(np.float32),
            'body_pose': (rng.standard_normal((n_poses, 23, 3)) * 0.2).astype(np.float32),
            'transl': (rng.standard_normal((n_poses, 3)) * 0.02).astype(np.float32)}


def view_arrays(size, seed, radius):
    """(image (size, size, 3) uint8: smooth colour ramps plus a little noise; mask (size, size) uint8: a centred disc of 255)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    ramps = np.stack([xx * 255.0 / size, yy * 255.0 / size, (xx + yy) * 127.0 / size], axis=-1)
    img = np.clip(ramps + rng.integers(-20, 21, (size, size, 3)), 0, 255).astype(np.uint8)
    msk = (((yy - size / 2 + 0.5) ** 2 + (xx - size / 2 + 0.5) ** 2) <= radius * radius).astype(np.uint8) * 255
    return img, msk


def write_tree(base, n_subjects=1, layers=(0, 1), poses=(0,), n_views=4, size=64, png_images=((0, 0, 0, 1),), radius=7.0):
    """Writes the tree under `base` and returns (data_root of the first subject, {(subject, layer, pose, view): (img_path, mask_path)}).
    `png_images`: the (subject, layer, pose, view) keys whose image is a PNG; every other image is a JPEG."""
    from PIL import Image
    base = str(base)
    names = [f'human_{s:02d}' for s in range(n_subjects)]
    with open(os.path.join(base, 'human_list.txt'), 'w') as f:
        f.write(''.join(n + '\n' for n in names))
    files = {}
    for s, name in enumerate(names):
        root = os.path.join(base, name)
        os.makedirs(os.path.dirname(os.path.join(root, SMPL_FILE)), exist_ok=True)
        with open(os.path.join(root, 'cameras.json'), 'w') as f:
            json.dump(orbit_cameras(n_views, size), f)
        np.savez(os.path.join(root, SMPL_FILE), smpl=np.array(smpl_file_content(max(poses) + 1, 50 + s), dtype=object))
        for layer in layers:
            for v in range(n_views):
                for pose in poses:
                    key = (s, layer, pose, v)
                    img, msk = view_arrays(size, ((s * 4 + layer) * 100 + pose) * 100 + v, radius + 0.5 * layer)
                    ext = '.png' if key in png_images else '.jpg'
                    ip = os.path.join(root, LAYER_DIRS[layer], 'img', f'camera{v:04d}', f'{pose:04d}{ext}')
                    mp = os.path.join(root, LAYER_DIRS[layer], 'mask', f'camera{v:04d}', f'{pose:04d}.png')
                    os.makedirs(os.path.dirname(ip), exist_ok=True)
                    os.makedirs(os.path.dirname(mp), exist_ok=True)
                    Image.fromarray(img).save(ip, **({} if ext == '.png' else {'quality': 95}))
                    Image.fromarray(msk).save(mp)
                    files[key] = (ip, mp)
    return os.path.join(base, names[0]), files
