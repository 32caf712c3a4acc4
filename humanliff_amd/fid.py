"""Frechet Inception Distance on the device: the pool3 features of pytorch-fid's InceptionV3 (block 3, 2048-d), their float64 mean and
covariance, and the distance between two such statistics - hl_fid (csrc/hl_fid.hip; contract: DESIGN.md 4l "FID").  The weights come
from a state dict the user supplies; nothing is downloaded and neither `pytorch_fid` nor `torchvision` is imported.  There is no CPU
path for the network or the moments; the distance itself is two symmetric eigen-decompositions in float64 on the host, once per
evaluation.

The architecture was written down from the published description of the network and has not been checked against pytorch-fid's own
weights."""
import ctypes as C

import numpy as np
import torch

from . import _lib

DIMS = 2048
BN_EPS = 1e-3
SIDE = 299
MIN_SIDE = 75                       # without resize: every stride-2 stage must leave at least one pixel
CHUNK = 16                          # input channels per K step of k_fid_conv
BLOCK_CHANNELS = (64, 192, 768, 2048)


def _layers():
    """The 94 BasicConv2d in the order the forward runs them: (name, (Cin, Cout, kH, kW, sH, sW, pH, pW)).  The library holds the same
    table (hl_fid_layer); tests/test_fid_cpu.py compares the two."""
    rows = []

    def add(block, name, cin, cout, kh, kw, s=1, ph=0, pw=0):
        rows.append((f"{block}.{name}" if block else name, (cin, cout, kh, kw, s, s, ph, pw)))

    add("", "Conv2d_1a_3x3", 3, 32, 3, 3, 2)
    add("", "Conv2d_2a_3x3", 32, 32, 3, 3)
    add("", "Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1)
    add("", "Conv2d_3b_1x1", 64, 80, 1, 1)
    add("", "Conv2d_4a_3x3", 80, 192, 3, 3)
    for b, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(b, "branch1x1", cin, 64, 1, 1)
        add(b, "branch5x5_1", cin, 48, 1, 1)
        add(b, "branch5x5_2", 48, 64, 5, 5, 1, 2, 2)
        add(b, "branch3x3dbl_1", cin, 64, 1, 1)
        add(b, "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1)
        add(b, "branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1)
        add(b, "branch_pool", cin, pf, 1, 1)
    add("Mixed_6a", "branch3x3", 288, 384, 3, 3, 2)
    add("Mixed_6a", "branch3x3dbl_1", 288, 64, 1, 1)
    add("Mixed_6a", "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1)
    add("Mixed_6a", "branch3x3dbl_3", 96, 96, 3, 3, 2)
    for b, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(b, "branch1x1", 768, 192, 1, 1)
        add(b, "branch7x7_1", 768, c7, 1, 1)
        add(b, "branch7x7_2", c7, c7, 1, 7, 1, 0, 3)
        add(b, "branch7x7_3", c7, 192, 7, 1, 1, 3, 0)
        add(b, "branch7x7dbl_1", 768, c7, 1, 1)
        add(b, "branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0)
        add(b, "branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3)
        add(b, "branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0)
        add(b, "branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3)
        add(b, "branch_pool", 768, 192, 1, 1)
    add("Mixed_7a", "branch3x3_1", 768, 192, 1, 1)
    add("Mixed_7a", "branch3x3_2", 192, 320, 3, 3, 2)
    add("Mixed_7a", "branch7x7x3_1", 768, 192, 1, 1)
    add("Mixed_7a", "branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3)
    add("Mixed_7a", "branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0)
    add("Mixed_7a", "branch7x7x3_4", 192, 192, 3, 3, 2)
    for b, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(b, "branch1x1", cin, 320, 1, 1)
        add(b, "branch3x3_1", cin, 384, 1, 1)
        add(b, "branch3x3_2a", 384, 384, 1, 3, 1, 0, 1)
        add(b, "branch3x3_2b", 384, 384, 3, 1, 1, 1, 0)
        add(b, "branch3x3dbl_1", cin, 448, 1, 1)
        add(b, "branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1)
        add(b, "branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1)
        add(b, "branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0)
        add(b, "branch_pool", cin, 192, 1, 1)
    return tuple(rows)


LAYERS = _layers()
# the top-level module of a layer -> its place in the wrapper's `blocks` (blocks.B.I.<rest of the name>)
WRAPPER = {"Conv2d_1a_3x3": "blocks.0.0", "Conv2d_2a_3x3": "blocks.0.1", "Conv2d_2b_3x3": "blocks.0.2", "Conv2d_3b_1x1": "blocks.1.0",
           "Conv2d_4a_3x3": "blocks.1.1", "Mixed_5b": "blocks.2.0", "Mixed_5c": "blocks.2.1", "Mixed_5d": "blocks.2.2", "Mixed_6a": "blocks.2.3",
           "Mixed_6b": "blocks.2.4", "Mixed_6c": "blocks.2.5", "Mixed_6d": "blocks.2.6", "Mixed_6e": "blocks.2.7", "Mixed_7a": "blocks.3.0",
           "Mixed_7b": "blocks.3.1", "Mixed_7c": "blocks.3.2"}


def library_layers():
    """The library's layer table, row by row, in the form of LAYERS."""
    L = _lib.lib()
    rows = []
    for i in range(_lib.HL_FID_LAYERS):
        name, desc = C.create_string_buffer(64), (C.c_int * 8)()
        _lib.check(L.hl_fid_layer(i, name, 64, desc), "hl_fid_layer")
        rows.append((name.value.decode(), tuple(desc)))
    return tuple(rows)


def wrapper_name(name):
    top, _, rest = name.partition(".")
    return WRAPPER[top] + ("." + rest if rest else "")


def _take(sd, name, suffix, shape):
    keys = (f"{name}.{suffix}", f"{wrapper_name(name)}.{suffix}")
    key = next((k for k in keys if k in sd), None)
    if key is None:
        raise KeyError(f"InceptionFID: the state dict has neither '{keys[0]}' nor '{keys[1]}'")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"InceptionFID: '{key}' must be a tensor of shape {tuple(shape)}, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    return t.detach()


def fold_batchnorm(w, gamma, beta, mean, var, eps=BN_EPS):
    """Convolution without bias + eval-mode BatchNorm -> (weight, bias) of one convolution, in float64."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * scale.view(-1, 1, 1, 1), beta.double() - mean.double() * scale


def _pack_conv(w, device):
    """(Cout, Cin, kH, kW) -> (kH kW, ceil(Cin / 16), CoutP, 16), CoutP = Cout rounded up to 32: tap, channel chunk, output channel,
    channel within the chunk; zeros in all padding."""
    cout, cin, kh, kw = w.shape
    nch, coutp = (cin + CHUNK - 1) // CHUNK, (cout + 31) // 32 * 32
    full = torch.zeros((coutp, nch * CHUNK, kh * kw), dtype=torch.float32)
    full[:cout, :cin] = w.reshape(cout, cin, kh * kw)
    return full.reshape(coutp, nch, CHUNK, kh * kw).permute(3, 1, 0, 2).contiguous().to(device)


class InceptionFID:
    """pytorch-fid's InceptionV3 up to pool3 in eval mode: `model(x)` -> (N, 2048) float32 on the device; x (N, 3, h, w) float32 in [0, 1]."""

    def __init__(self, convs, device="cuda", resize_input=True, normalize_input=True):
        """convs: 94 (weight (Cout, Cin, kH, kW), bias (Cout,)) with BatchNorm folded in, in the order of LAYERS."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("InceptionFID needs a HIP device; humanliff_amd has no CPU path")
        if len(convs) != len(LAYERS):
            raise ValueError(f"InceptionFID: {len(convs)} convolutions, the network has {len(LAYERS)}")
        self.device = device
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self._host = [(w.detach().float(), b.detach().float()) for w, b in convs]
        for (name, d), (w, b) in zip(LAYERS, self._host):
            if tuple(w.shape) != (d[1], d[0], d[2], d[3]) or tuple(b.shape) != (d[1],):
                raise ValueError(f"InceptionFID: '{name}' must have a weight of shape {(d[1], d[0], d[2], d[3])}, got {tuple(w.shape)}")
        self._params = None
        self._ws = None

    @classmethod
    def from_state_dict(cls, sd, device="cuda", resize_input=True, normalize_input=True):
        """From the FID weights file (a torchvision-style Inception3 state dict: <layer>.conv.weight, <layer>.bn.weight / bias /
        running_mean / running_var) or the wrapper's own state dict (blocks.B.I.<...>).  fc.*, AuxLogits.* and num_batches_tracked are
        not looked at.  BatchNorm (eps 1e-3) is folded in float64, once, then rounded to float32.  KeyError / ValueError name the key."""
        convs = []
        for name, (cin, cout, kh, kw, *_) in LAYERS:
            w = _take(sd, name, "conv.weight", (cout, cin, kh, kw))
            bn = [_take(sd, name, f"bn.{k}", (cout,)) for k in ("weight", "bias", "running_mean", "running_var")]
            w64, b64 = fold_batchnorm(w, *bn)
            convs.append((w64.float(), b64.float()))
        return cls(convs, device, resize_input, normalize_input)

    def _upload(self):
        """Pack the weights to the kernel's layout on the device, once, at the first call."""
        if self._params is not None:
            return
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._w = [_pack_conv(w, self.device) for w, _ in self._host]
        self._b = [b.to(self.device).contiguous() for _, b in self._host]
        p = _lib.FidParams()
        for i in range(len(LAYERS)):
            p.conv_w[i], p.conv_b[i] = self._w[i].data_ptr(), self._b[i].data_ptr()
        self._params, self._host = p, None

    def _images(self, x):
        if not torch.is_tensor(x):
            raise RuntimeError(f"InceptionFID: x must be a HIP tensor, got {type(x).__name__}")
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or x.shape[0] < 1:
            raise RuntimeError(f"InceptionFID: x must be (3, h, w) or (N, 3, h, w) float32, got {tuple(x.shape)} {x.dtype}")
        if not self.resize_input and (x.shape[2] < MIN_SIDE or x.shape[3] < MIN_SIDE):
            raise ValueError(f"InceptionFID: x is {x.shape[2]} x {x.shape[3]}; without resize_input the network needs h, w >= {MIN_SIDE}")
        if not x.is_cuda:
            raise RuntimeError("InceptionFID: x must be a HIP tensor; humanliff_amd has no CPU path")
        self._upload()
        if x.device != self.device:
            raise RuntimeError(f"InceptionFID: x is on {x.device}, the weights on {self.device}")
        return x.contiguous()

    def _workspace(self, n, h, w, keep):
        """__call__ reuses one grow-only buffer (`keep`); blocks() returns views into its workspace: a buffer of its own."""
        nbytes = _lib.lib().hl_fid_workspace_bytes(n, h, w, int(self.resize_input))
        if nbytes == 0:
            raise ValueError(f"InceptionFID: {n} images of {h} x {w} are outside what hl_fid_features serves")
        if not keep:
            return torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = None                         # (released before the larger one is taken)
            self._ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        return self._ws

    def _run(self, x, ws, out):
        n, _, h, w = x.shape
        with _lib.on(self.device):
            _lib.check(_lib.lib().hl_fid_features(C.byref(self._params), _lib.ptr(x), n, h, w, int(self.resize_input), int(self.normalize_input),
                                                  _lib.ptr(out), C.c_void_p(ws.data_ptr()), ws.numel() * 4, _lib.stream_ptr(self.device)),
                       "hl_fid_features")

    def blocks(self, x):
        """The four block outputs of pytorch-fid's wrapper: (N, 64, ., .), (N, 192, ., .), (N, 768, ., .) (channels-last in memory) and the
        pool3 features (N, 2048, 1, 1)."""
        x = self._images(x)
        n, _, h, w = x.shape
        ws = self._workspace(n, h, w, keep=False)
        self._run(x, ws, None)
        L, out = _lib.lib(), []
        for k in range(4):
            off, hk, wk, ck = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
            _lib.check(L.hl_fid_block_shape(n, h, w, int(self.resize_input), k, C.byref(off), C.byref(hk), C.byref(wk), C.byref(ck)), "hl_fid_block_shape")
            numel = n * hk.value * wk.value * ck.value
            out.append(ws[off.value // 4: off.value // 4 + numel].view(n, hk.value, wk.value, ck.value).permute(0, 3, 1, 2))
        return out

    def __call__(self, x):
        x = self._images(x)
        n, _, h, w = x.shape
        ws = self._workspace(n, h, w, keep=True)
        out = torch.empty((n, DIMS), dtype=torch.float32, device=self.device)
        self._run(x, ws, out)
        return out


class FidStatistics:
    """Running float64 moments of pool3 features on the device: update(features) per batch, finalize() -> (mu (2048,), sigma (2048, 2048)).
    The images are taken strictly in order with separately rounded products and sums, so the result does not depend on the batching."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("FidStatistics needs a HIP device; humanliff_amd has no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.count = 0
        self._state = torch.zeros(_lib.HL_FID_STATE_BYTES // 8, dtype=torch.float64, device=device)

    def update(self, features):
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != DIMS or features.dtype != torch.float32:
            raise RuntimeError(f"FidStatistics: features must be (n, {DIMS}) float32, got "
                               f"{(tuple(features.shape), features.dtype) if torch.is_tensor(features) else type(features).__name__}")
        if not features.is_cuda or features.device != self.device:
            raise RuntimeError(f"FidStatistics: features must be on {self.device}; humanliff_amd has no CPU path")
        n = features.shape[0]
        if n == 0:
            return self
        features = features.contiguous()
        with _lib.on(self.device):
            _lib.check(_lib.lib().hl_fid_moments_update(C.c_void_p(self._state.data_ptr()), _lib.ptr(features), n, _lib.stream_ptr(self.device)),
                       "hl_fid_moments_update")
        self.count += n
        return self

    def finalize(self):
        if self.count < 2:
            raise ValueError(f"FidStatistics: a covariance needs at least 2 images, got {self.count}")
        mu = torch.empty(DIMS, dtype=torch.float64, device=self.device)
        sigma = torch.empty((DIMS, DIMS), dtype=torch.float64, device=self.device)
        with _lib.on(self.device):
            _lib.check(_lib.lib().hl_fid_moments_finalize(C.c_void_p(self._state.data_ptr()), self.count, C.c_void_p(mu.data_ptr()),
                                                          C.c_void_p(sigma.data_ptr()), _lib.stream_ptr(self.device)), "hl_fid_moments_finalize")
        return mu, sigma

    def save(self, path):
        """pytorch-fid's --save-stats layout: an .npz with `mu` and `sigma`."""
        mu, sigma = self.finalize()
        save_statistics(path, mu, sigma)


def save_statistics(path, mu, sigma):
    with open(path, "wb") as f:                     # (an open file: np.savez would append .npz to a bare name)
        np.savez(f, mu=_host64(mu).numpy(), sigma=_host64(sigma).numpy())


def load_statistics(path):
    """(mu, sigma) as float64 host tensors from an .npz in pytorch-fid's layout."""
    with np.load(path) as z:
        for k in ("mu", "sigma"):
            if k not in z:
                raise KeyError(f"{path} has no '{k}'")
        mu, sigma = torch.from_numpy(np.asarray(z["mu"], dtype=np.float64)), torch.from_numpy(np.asarray(z["sigma"], dtype=np.float64))
    if mu.dim() != 1 or tuple(sigma.shape) != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"{path}: mu {tuple(mu.shape)} and sigma {tuple(sigma.shape)} do not belong together")
    return mu, sigma


FidStatistics.load = staticmethod(load_statistics)


def _host64(t):
    t = torch.as_tensor(t) if not torch.is_tensor(t) else t
    return t.detach().to(device="cpu", dtype=torch.float64)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum_k sqrt(max(lambda_k, 0)), lambda_k the eigenvalues of R S2 R, R = S1^(1/2) from eigh with its
    eigenvalues clamped at 0.  R S2 R is similar to S1 S2 where S1 is regular, so the sum is pytorch-fid's tr sqrtm(S1 S2) where that is
    well defined, and stays real where sqrtm goes complex (fewer images than dimensions).  Float64 on the host, any D.

    The sqrt(lambda_k) are taken as the singular values of A = L2^(1/2) Q2' Q1 L1^(1/2) (S_i = Q_i L_i Q_i' from eigh, clamped at 0):
    R S2 R = (S2^(1/2) R)' (S2^(1/2) R), and S2^(1/2) R is A between two orthogonal matrices.  Calling eigh on R S2 R itself returns the
    same numbers with an absolute error of eps |R S2 R| each, which the root turns into sqrt(eps) for every eigenvalue that is truly 0 - with
    6 images and D = 2048 there are 2043 of them, and the distance of a set from itself came out as -1.1e-6 tr S instead of 0; a
    singular value carries eps |A|."""
    mu1, sigma1, mu2, sigma2 = (_host64(t) for t in (mu1, sigma1, mu2, sigma2))
    d = mu1.shape[0]
    if mu1.dim() != 1 or mu2.shape != mu1.shape or tuple(sigma1.shape) != (d, d) or tuple(sigma2.shape) != (d, d):
        raise ValueError(f"frechet_distance: shapes {tuple(mu1.shape)}, {tuple(sigma1.shape)}, {tuple(mu2.shape)}, {tuple(sigma2.shape)}")
    lam1, q1 = torch.linalg.eigh((sigma1 + sigma1.T) / 2)
    lam2, q2 = torch.linalg.eigh((sigma2 + sigma2.T) / 2)
    a = torch.sqrt(lam2.clamp_min(0.0))[:, None] * (q2.T @ q1) * torch.sqrt(lam1.clamp_min(0.0))[None, :]
    cross = torch.linalg.svdvals(a).sum()
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * cross)
