"""A small TightCap-shaped directory tree written with PIL, for tests/test_tightcap_dataset_cpu.py and tests/test_tightcap_dataset_gpu.py:
TightCap_human_list.txt, per subject person-top-bottom-shoes/{cameras.json, outputs_re_fitting/refit_smpl_2nd.npz, img/camera{vvvv}/{pppp}.jpg}
and {person-top-bottom-shoes,person,top,bottom,shoes}/mask/camera{vvvv}/{pppp}.png.  One photograph per view: the cloth layers are composed
from it by the reader."""
import json
import os

import numpy as np

from tests import synbody_fixture as sf

FULL_DIR = 'person-top-bottom-shoes'
PLANE_DIRS = {'full': FULL_DIR, 'person': 'person', 'top': 'top', 'bottom': 'bottom', 'shoes': 'shoes'}
SMPL_FILE = os.path.join(FULL_DIR, 'outputs_re_fitting', 'refit_smpl_2nd.npz')


def view_arrays(size, seed, radius):
    """(image (size, size, 3) uint8, {plane: (size, size) uint8}): synbody_fixture's ramps; a centred body disc (person) wearing a top
    (a band above the middle, a little wider than the body; the head stays bare), a bottom (below the middle, overlapping the top by a
    band) and shoes (the lowest rows, partly beside the body), with a few pixels of the top sticking out of `full`."""
    img, person = sf.view_arrays(size, seed, radius)
    yy, xx = np.mgrid[0:size, 0:size]
    c = size / 2 - 0.5
    wide = (((yy - c) ** 2 + (xx - c) ** 2) <= (radius + 1.5) ** 2)
    top = wide & (yy >= c - 0.6 * radius) & (yy < c + 1)                                      # (the head stays bare)
    bottom = wide & (yy > c - 1) & (yy < c + radius - 1)
    shoes = (np.abs(yy - (c + radius)) <= 1.5) & (np.abs(xx - c) <= radius * 0.7)
    full = ((person != 0) | top | bottom | shoes) & ~(top & (xx > c + radius))                # the top's rim on the right is outside `full`
    u8 = lambda m: m.astype(np.uint8) * np.uint8(255)  # noqa: E731
    return img, {'full': u8(full), 'person': person, 'top': u8(top), 'bottom': u8(bottom), 'shoes': u8(shoes)}


def write_tree(base, n_subjects=1, poses=(0,), n_views=4, size=64, radius=7.0, jpeg=True):
    """Writes the tree under `base` and returns (data_root of the first subject, {(subject, pose, view): (img_path, {plane: mask_path})})."""
    from PIL import Image
    base = str(base)
    names = [f'human_{s:02d}' for s in range(n_subjects)]
    with open(os.path.join(base, 'TightCap_human_list.txt'), 'w') as f:
        f.write(''.join(n + '\n' for n in names))
    files = {}
    for s, name in enumerate(names):
        root = os.path.join(base, name)
        os.makedirs(os.path.dirname(os.path.join(root, SMPL_FILE)), exist_ok=True)
        with open(os.path.join(root, FULL_DIR, 'cameras.json'), 'w') as f:
            json.dump(sf.orbit_cameras(n_views, size), f)
        np.savez(os.path.join(root, SMPL_FILE), smpl=np.array(sf.smpl_file_content(max(poses) + 1, 50 + s), dtype=object))
        for v in range(n_views):
            for pose in poses:
                img, planes = view_arrays(size, (s * 100 + pose) * 100 + v, radius)
                ip = os.path.join(root, FULL_DIR, 'img', f'camera{v:04d}', f'{pose:04d}' + ('.jpg' if jpeg else '.png'))
                os.makedirs(os.path.dirname(ip), exist_ok=True)
                Image.fromarray(img).save(ip, **({'quality': 95} if jpeg else {}))
                paths = {}
                for n, a in planes.items():
                    mp = os.path.join(root, PLANE_DIRS[n], 'mask', f'camera{v:04d}', f'{pose:04d}.png')
                    os.makedirs(os.path.dirname(mp), exist_ok=True)
                    Image.fromarray(a).save(mp)
                    paths[n] = mp
                files[(s, pose, v)] = (ip, paths)
    return os.path.join(base, names[0]), files
