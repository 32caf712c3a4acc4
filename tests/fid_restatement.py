"""A restatement of pytorch-fid's InceptionV3 (the FID variant of torchvision's Inception3, eval mode, up to pool3) from plain
F.conv2d / F.batch_norm / F.avg_pool2d / F.max_pool2d / F.interpolate, in the dtype of its input (float64 is the tests' reference,
float32 is what the package computes).  Neither `pytorch_fid` nor `torchvision` is imported: the network is written out here, from the
description in DESIGN.md 4l, and like that description it has not been checked against pytorch-fid's own weights.

Every BasicConv2d is a convolution without bias, BatchNorm with eps = 1e-3 in eval mode, ReLU.  The forward asks a parameter source for
each layer by name and shape, so the forward itself is the list of the network's layers: Seeded (below) generates a layer's parameters
the first time it is asked, and `layers()` is the list a forward leaves behind.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
PARTS = ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")


class Seeded:
    """Seeded parameters: convolution weights N(0, 2 / fan_in), gamma and running_var U(0.75, 1.25), beta and running_mean 0.1 N(0, 1);
    float32 values (a float64 run uses the same values, widened)."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.rows, self.p, self.cast = [], {}, {}

    def get(self, name, cin, cout, kh, kw, dtype):
        if name not in self.p:
            w = torch.randn((cout, cin, kh, kw), generator=self.g) * float(np.sqrt(2.0 / (cin * kh * kw)))
            gamma, var = (0.75 + 0.5 * torch.rand((cout,), generator=self.g) for _ in range(2))
            beta, mean = (0.1 * torch.randn((cout,), generator=self.g) for _ in range(2))
            self.p[name] = (w, gamma, beta, mean, var)
            self.rows.append((name, (cin, cout, kh, kw)))
        if (name, dtype) not in self.cast:
            self.cast[name, dtype] = tuple(t.to(dtype) for t in self.p[name])
        return self.cast[name, dtype]

    def state_dict(self, rename=lambda name: name):
        """<layer>.conv.weight and <layer>.bn.{weight, bias, running_mean, running_var} of every layer asked for so far."""
        sd = {}
        for name, _ in self.rows:
            w, gamma, beta, mean, var = self.p[name]
            for part, t in zip(PARTS, (w, gamma, beta, mean, var)):
                sd[f"{rename(name)}.{part}"] = t
        return sd


def bconv(P, name, x, cout, k, s=1, p=0):
    kh, kw = k if isinstance(k, tuple) else (k, k)
    w, gamma, beta, mean, var = P.get(name, x.shape[1], cout, kh, kw, x.dtype)
    x = F.conv2d(x, w, None, stride=s, padding=p)
    return F.relu(F.batch_norm(x, mean, var, gamma, beta, False, 0.0, BN_EPS))


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def mixed_a(P, b, x, pf):
    b1 = bconv(P, f"{b}.branch1x1", x, 64, 1)
    b5 = bconv(P, f"{b}.branch5x5_2", bconv(P, f"{b}.branch5x5_1", x, 48, 1), 64, 5, p=2)
    b3 = bconv(P, f"{b}.branch3x3dbl_1", x, 64, 1)
    b3 = bconv(P, f"{b}.branch3x3dbl_3", bconv(P, f"{b}.branch3x3dbl_2", b3, 96, 3, p=1), 96, 3, p=1)
    bp = bconv(P, f"{b}.branch_pool", _avg(x), pf, 1)
    return torch.cat([b1, b5, b3, bp], 1)


def mixed_b(P, b, x):
    b3 = bconv(P, f"{b}.branch3x3", x, 384, 3, s=2)
    bd = bconv(P, f"{b}.branch3x3dbl_2", bconv(P, f"{b}.branch3x3dbl_1", x, 64, 1), 96, 3, p=1)
    bd = bconv(P, f"{b}.branch3x3dbl_3", bd, 96, 3, s=2)
    return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)


def mixed_c(P, b, x, c7):
    b1 = bconv(P, f"{b}.branch1x1", x, 192, 1)
    b7 = bconv(P, f"{b}.branch7x7_1", x, c7, 1)
    b7 = bconv(P, f"{b}.branch7x7_2", b7, c7, (1, 7), p=(0, 3))
    b7 = bconv(P, f"{b}.branch7x7_3", b7, 192, (7, 1), p=(3, 0))
    bd = bconv(P, f"{b}.branch7x7dbl_1", x, c7, 1)
    bd = bconv(P, f"{b}.branch7x7dbl_2", bd, c7, (7, 1), p=(3, 0))
    bd = bconv(P, f"{b}.branch7x7dbl_3", bd, c7, (1, 7), p=(0, 3))
    bd = bconv(P, f"{b}.branch7x7dbl_4", bd, c7, (7, 1), p=(3, 0))
    bd = bconv(P, f"{b}.branch7x7dbl_5", bd, 192, (1, 7), p=(0, 3))
    bp = bconv(P, f"{b}.branch_pool", _avg(x), 192, 1)
    return torch.cat([b1, b7, bd, bp], 1)


def mixed_d(P, b, x):
    b3 = bconv(P, f"{b}.branch3x3_2", bconv(P, f"{b}.branch3x3_1", x, 192, 1), 320, 3, s=2)
    b7 = bconv(P, f"{b}.branch7x7x3_1", x, 192, 1)
    b7 = bconv(P, f"{b}.branch7x7x3_2", b7, 192, (1, 7), p=(0, 3))
    b7 = bconv(P, f"{b}.branch7x7x3_3", b7, 192, (7, 1), p=(3, 0))
    b7 = bconv(P, f"{b}.branch7x7x3_4", b7, 192, 3, s=2)
    return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)


def mixed_e(P, b, x, max_pool):
    b1 = bconv(P, f"{b}.branch1x1", x, 320, 1)
    b3 = bconv(P, f"{b}.branch3x3_1", x, 384, 1)
    b3 = torch.cat([bconv(P, f"{b}.branch3x3_2a", b3, 384, (1, 3), p=(0, 1)), bconv(P, f"{b}.branch3x3_2b", b3, 384, (3, 1), p=(1, 0))], 1)
    bd = bconv(P, f"{b}.branch3x3dbl_2", bconv(P, f"{b}.branch3x3dbl_1", x, 448, 1), 384, 3, p=1)
    bd = torch.cat([bconv(P, f"{b}.branch3x3dbl_3a", bd, 384, (1, 3), p=(0, 1)), bconv(P, f"{b}.branch3x3dbl_3b", bd, 384, (3, 1), p=(1, 0))], 1)
    pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else _avg(x)          # the FID variant's Mixed_7c pools with a maximum
    bp = bconv(P, f"{b}.branch_pool", pooled, 192, 1)
    return torch.cat([b1, b3, bd, bp], 1)


def blocks(P, x, resize_input=True, normalize_input=True):
    """The four block outputs of x (N, 3, h, w) in [0, 1]: (N, 64, ., .), (N, 192, ., .), (N, 768, ., .), (N, 2048, 1, 1)."""
    if resize_input:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    out = []
    x = bconv(P, "Conv2d_1a_3x3", x, 32, 3, s=2)
    x = bconv(P, "Conv2d_2a_3x3", x, 32, 3)
    x = bconv(P, "Conv2d_2b_3x3", x, 64, 3, p=1)
    x = F.max_pool2d(x, 3, 2)
    out.append(x)
    x = bconv(P, "Conv2d_3b_1x1", x, 80, 1)
    x = bconv(P, "Conv2d_4a_3x3", x, 192, 3)
    x = F.max_pool2d(x, 3, 2)
    out.append(x)
    x = mixed_a(P, "Mixed_5b", x, 32)
    x = mixed_a(P, "Mixed_5c", x, 64)
    x = mixed_a(P, "Mixed_5d", x, 64)
    x = mixed_b(P, "Mixed_6a", x)
    x = mixed_c(P, "Mixed_6b", x, 128)
    x = mixed_c(P, "Mixed_6c", x, 160)
    x = mixed_c(P, "Mixed_6d", x, 160)
    x = mixed_c(P, "Mixed_6e", x, 192)
    out.append(x)
    x = mixed_d(P, "Mixed_7a", x)
    x = mixed_e(P, "Mixed_7b", x, False)
    x = mixed_e(P, "Mixed_7c", x, True)
    out.append(x.mean([2, 3], keepdim=True))
    return out


# the wrapper's names: blocks.B.I.<rest>
_WRAPPER = ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"], ["Conv2d_3b_1x1", "Conv2d_4a_3x3"], \
    ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"], ["Mixed_7a", "Mixed_7b", "Mixed_7c"]


def wrapper_name(name):
    top, _, rest = name.partition(".")
    for b, members in enumerate(_WRAPPER):
        if top in members:
            return f"blocks.{b}.{members.index(top)}" + ("." + rest if rest else "")
    raise KeyError(name)


# ---- the moment rule and the distance, restated with numpy / scipy ----
def moments(x):
    """(mu, sigma) of fp32 feature rows x (n, D) by the library's rule: rows widened to float64 and taken strictly in order,
    s += x, S += outer(x, x) (numpy rounds the product and the sum separately); mu = s / n; sigma[i][j] = (S[i][j] - (n mu[i]) mu[j]) / (n - 1)
    for i <= j, mirrored below the diagonal."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, d = x.shape
    s, S = np.zeros(d), np.zeros((d, d))
    for row in x:
        s = s + row
        S = S + np.outer(row, row)
    mu = s / float(n)
    full = (S - np.outer(float(n) * mu, mu)) / (float(n) - 1.0)
    return mu, np.triu(full) + np.triu(full, 1).T


def frechet_sqrtm(mu1, sigma1, mu2, sigma2):
    """pytorch-fid's calculate_frechet_distance, where the square root is well defined: |d mu|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2)."""
    from scipy import linalg
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        assert np.abs(covmean.imag).max() <= 1e-3 * np.abs(covmean.real).max()
        covmean = covmean.real
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))
