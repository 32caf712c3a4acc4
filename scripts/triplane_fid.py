"""Frechet Inception Distance between two image sets on the device (humanliff_amd.fid).

    python scripts/triplane_fid.py A B --inception-weights PATH [--batch 64] [--save-stats OUT.npz [OUT_B.npz]]

A and B are each a directory of images (decoded with PIL, uploaded as uint8, scaled to [0, 1] on the device) or an .npz of statistics
in pytorch-fid's --save-stats layout (`mu`, `sigma`).  PATH is a saved state dict of pytorch-fid's InceptionV3 (INTEGRATION.md says how
to write one on a machine that has the package); it is only needed when a directory is given.  --save-stats writes the statistics of
A (and of B, with a second name) so that a set is pushed through the network once.  Prints the FID and the image counts.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

EXTENSIONS = (".bmp", ".jpg", ".jpeg", ".pgm", ".png", ".ppm", ".tif", ".tiff", ".webp")       # pytorch-fid's list


def image_files(path):
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(EXTENSIONS))
    if len(files) < 2:
        raise SystemExit(f"{path}: {len(files)} images; a covariance needs at least 2")
    return files


def directory_statistics(path, model, batch, dev):
    """Every image of the directory, in sorted order, through the network into the running moments; images of one size share a call."""
    from PIL import Image
    from humanliff_amd.fid import FidStatistics
    stats, pending = FidStatistics(dev), []

    def flush():
        if pending:
            x = torch.from_numpy(np.stack(pending)).to(dev).permute(0, 3, 1, 2).float() / 255.0
            stats.update(model(x))
            pending.clear()

    for f in image_files(path):
        with Image.open(f) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if pending and (a.shape != pending[0].shape or len(pending) == batch):
            flush()
        pending.append(a)
    flush()
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sets", nargs=2, metavar=("A", "B"), help="a directory of images or an .npz of statistics, each")
    ap.add_argument("--inception-weights", help="a saved state dict of pytorch-fid's InceptionV3")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--save-stats", nargs="+", metavar="OUT.npz", help="write the statistics of A (and B) here")
    a = ap.parse_args()
    from humanliff_amd.fid import InceptionFID, frechet_distance, load_statistics, save_statistics
    if a.save_stats and len(a.save_stats) > 2:
        ap.error("--save-stats: one name (A) or two (A and B)")
    dev, model, results = torch.device("cuda:0"), None, []
    for i, path in enumerate(a.sets):
        if os.path.isdir(path):
            if model is None:
                if not a.inception_weights:
                    ap.error("--inception-weights is needed to score a directory of images")
                model = InceptionFID.from_state_dict(torch.load(a.inception_weights, map_location="cpu"), dev)
            stats = directory_statistics(path, model, a.batch, dev)
            mu, sigma = stats.finalize()
            results.append((mu, sigma, f"{stats.count} images"))
        else:
            mu, sigma = load_statistics(path)
            results.append((mu, sigma, "saved statistics"))
        if a.save_stats and i < len(a.save_stats):
            save_statistics(a.save_stats[i], mu, sigma)
    (mu1, s1, n1), (mu2, s2, n2) = results
    print(f"FID {frechet_distance(mu1, s1, mu2, s2):.6f}  ({a.sets[0]}: {n1}; {a.sets[1]}: {n2})")


if __name__ == "__main__":
    main()
