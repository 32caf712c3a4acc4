"""Frechet Inception Distance between two image sets on the device (humanliff_amd.fid), and with --kid / --prc the Kernel
Inception Distance and precision / recall / density / coverage of their features (humanliff_amd.feature_metrics).

    python scripts/triplane_fid.py A B --inception-weights PATH [--batch 64] [--save-stats OUT.npz [OUT_B.npz]]
                                   [--save-features OUT.npy [OUT_B.npy]] [--kid [--kid-subsets 100 --kid-subset-size 1000]] [--prc [--prc-k 3]]

A and B are each a directory of images (decoded with PIL, uploaded as uint8, scaled to [0, 1] on the device), an .npy of pool3 features
(n, 2048) float32 as --save-features writes it, or an .npz of statistics in pytorch-fid's --save-stats layout (`mu`, `sigma`).  PATH is
a saved state dict of pytorch-fid's InceptionV3 (INTEGRATION.md says how to write one on a machine that has the package); it is only
needed when a directory is given.  --save-stats / --save-features write the statistics / the features of A (and of B, with a second
name) so that a set is pushed through the network once.  Prints the FID and the image counts, then the KID line, then the
precision / recall line.  KID and precision / recall need the features: a set given as statistics only is an error.
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


def directory_collector(path, model, batch, dev, keep):
    """Every image of the directory, in sorted order, through the network into the running moments (and the kept features); images of
    one size share a call."""
    from PIL import Image
    from humanliff_amd.feature_metrics import FeatureCollector
    from humanliff_amd.fid import FidStatistics
    col = FeatureCollector(model, batch, stats=FidStatistics(dev), keep=keep)
    for f in image_files(path):
        with Image.open(f) as im:
            a = np.array(im.convert("RGB"), dtype=np.uint8)
        col.add(torch.from_numpy(a).to(dev).permute(2, 0, 1).float() / 255.0)
    return col.flush()


def directory_statistics(path, model, batch, dev):
    return directory_collector(path, model, batch, dev, keep=False).stats


def load_features(path, dev):
    f = np.load(path)
    if f.ndim != 2 or f.shape[1] != 2048 or f.shape[0] < 2 or f.dtype != np.float32:
        raise SystemExit(f"{path}: features must be (n >= 2, 2048) float32, got {f.shape} {f.dtype}")
    return torch.from_numpy(f).to(dev)


def kid_line(mean, std, subsets, subset_size):
    return f"KID {mean:.8f} +- {std:.8f}  ({subsets} subsets of {subset_size})"


def prc_line(p, k):
    return f"precision {p['precision']:.6f}  recall {p['recall']:.6f}  density {p['density']:.6f}  coverage {p['coverage']:.6f}  (k = {k})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("sets", nargs=2, metavar=("A", "B"), help="a directory of images, an .npy of features or an .npz of statistics, each")
    ap.add_argument("--inception-weights", help="a saved state dict of pytorch-fid's InceptionV3")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--save-stats", nargs="+", metavar="OUT.npz", help="write the statistics of A (and B) here")
    ap.add_argument("--save-features", nargs="+", metavar="OUT.npy", help="write the pool3 features of A (and B) here")
    ap.add_argument("--kid", action="store_true", help="also print the Kernel Inception Distance (mean and std over the subsets)")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--prc", action="store_true", help="also print precision / recall / density / coverage")
    ap.add_argument("--prc-k", type=int, default=3)
    a = ap.parse_args(argv)
    from humanliff_amd.fid import FidStatistics, InceptionFID, frechet_distance, load_statistics, save_statistics
    if a.save_stats and len(a.save_stats) > 2:
        ap.error("--save-stats: one name (A) or two (A and B)")
    if a.save_features and len(a.save_features) > 2:
        ap.error("--save-features: one name (A) or two (A and B)")
    dev, model, results, feats = torch.device("cuda:0"), None, [], []
    for i, path in enumerate(a.sets):
        wanted = a.kid or a.prc or bool(a.save_features and i < len(a.save_features))
        if os.path.isdir(path):
            if model is None:
                if not a.inception_weights:
                    ap.error("--inception-weights is needed to score a directory of images")
                model = InceptionFID.from_state_dict(torch.load(a.inception_weights, map_location="cpu"), dev)
            col = directory_collector(path, model, a.batch, dev, keep=wanted)
            mu, sigma = col.stats.finalize()
            results.append((mu, sigma, f"{col.stats.count} images"))
            feats.append(col.features() if wanted else None)
        elif path.lower().endswith(".npy"):
            f = load_features(path, dev)
            mu, sigma = FidStatistics(dev).update(f).finalize()
            results.append((mu, sigma, f"{f.shape[0]} saved features"))
            feats.append(f)
        else:
            if wanted:
                raise SystemExit(f"{path} holds statistics only: --kid, --prc and --save-features need the features of both sets "
                                 "(a directory of images or an .npy written by --save-features)")
            mu, sigma = load_statistics(path)
            results.append((mu, sigma, "saved statistics"))
            feats.append(None)
        if a.save_stats and i < len(a.save_stats):
            save_statistics(a.save_stats[i], mu, sigma)
        if a.save_features and i < len(a.save_features):
            with open(a.save_features[i], "wb") as fh:
                np.save(fh, feats[i].cpu().numpy())
    (mu1, s1, n1), (mu2, s2, n2) = results
    print(f"FID {frechet_distance(mu1, s1, mu2, s2):.6f}  ({a.sets[0]}: {n1}; {a.sets[1]}: {n2})")
    if a.kid or a.prc:
        from humanliff_amd.feature_metrics import kernel_inception_distance, precision_recall
        if a.kid:
            try:
                mean, std, _ = kernel_inception_distance(feats[0], feats[1], a.kid_subsets, a.kid_subset_size)
            except ValueError as e:
                raise SystemExit(f"--kid: {e}")
            print(kid_line(mean, std, a.kid_subsets, a.kid_subset_size))
        if a.prc:
            try:
                p = precision_recall(feats[0], feats[1], a.prc_k)
            except ValueError as e:
                raise SystemExit(f"--prc: {e}")
            print(prc_line(p, a.prc_k))


if __name__ == "__main__":
    main()
