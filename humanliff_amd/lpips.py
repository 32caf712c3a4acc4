"""LPIPS(net='vgg', version='0.1') on the device: the perceptual score the reference's test mode reports (recon_NeRF/lib/all_test.py,
loss_fn_vgg) - hl_lpips (csrc/hl_lpips.hip; contract: DESIGN.md 4f "LPIPS").  The weights come from a state dict the user supplies;
nothing is downloaded and neither `lpips` nor `torchvision` is imported.  There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib

SHIFT = (-.030, -.088, -.188)       # the package's ScalingLayer
SCALE = (.458, .448, .450)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
# torchvision's features indices of the 13 convolutions, by the package's slice1..slice5
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIDE = 16                       # four 2 x 2 pools must leave 1 x 1
CHUNK = 16                          # input channels per K chunk of k_lpips_conv


def _take(sd, key, shape):
    if key not in sd:
        raise KeyError(f"LpipsVGG: the state dict has no '{key}'")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"LpipsVGG: '{key}' must be a tensor of shape {tuple(shape)}, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    return t.detach()


def _pack_conv(w, device):
    """(Cout, Cin, 3, 3) -> (ceil(Cin / 16), Cout, 9, 16): channel chunk, output channel, tap, channel within the chunk (zero-padded)."""
    w = w.to(device=device, dtype=torch.float32)
    cout, cin = w.shape[:2]
    nch = (cin + CHUNK - 1) // CHUNK
    full = torch.zeros((cout, nch * CHUNK, 9), dtype=torch.float32, device=device)
    full[:, :cin] = w.reshape(cout, cin, 9)
    return full.reshape(cout, nch, CHUNK, 9).permute(1, 0, 3, 2).contiguous()


class LpipsVGG:
    """lpips.LPIPS(net='vgg', version='0.1') in eval mode: `model(in0, in1)` -> (B, 1, 1, 1) float32 on the device."""

    def __init__(self, convs, lins, shift=SHIFT, scale=SCALE, device="cuda"):
        """convs: 13 (weight (Cout, Cin, 3, 3), bias (Cout,)) in network order; lins: 5 weights (1, C, 1, 1)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("LpipsVGG needs a HIP device; humanliff_amd has no CPU path")
        self.device = device
        self._host = ([(w.detach().float(), b.detach().float()) for w, b in convs], [l.detach().float().reshape(-1) for l in lins])
        self.shift, self.scale = tuple(float(v) for v in shift), tuple(float(v) for v in scale)
        self._params = None
        self._ws = None

    def _upload(self):
        """Pack the weights to the kernels' layout on the device, once, at the first call."""
        if self._params is not None:
            return
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        convs, lins = self._host
        self._w = [_pack_conv(w, self.device) for w, _ in convs]
        self._b = [b.to(self.device).contiguous() for _, b in convs]
        self._lin = [l.to(self.device).contiguous() for l in lins]
        p = _lib.LpipsParams()
        for i in range(13):
            p.conv_w[i], p.conv_b[i] = self._w[i].data_ptr(), self._b[i].data_ptr()
        for k in range(5):
            p.lin[k] = self._lin[k].data_ptr()
        p.shift[:], p.scale[:] = self.shift, self.scale
        self._params, self._host = p, None

    # ---- loaders ----
    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        """From lpips.LPIPS(net='vgg').state_dict(): net.slice{1..5}.{i}.weight / bias (torchvision's indices), lin{k}.model.1.weight or
        lins.{k}.model.1.weight (1, C, 1, 1), optional scaling_layer.shift / scale.  KeyError / ValueError name the offending key."""
        convs, cin = [], 3
        widths = iter(WIDTHS)
        for s, idx in enumerate(SLICES, 1):
            for i in idx:
                cout = next(widths)
                convs.append((_take(sd, f"net.slice{s}.{i}.weight", (cout, cin, 3, 3)), _take(sd, f"net.slice{s}.{i}.bias", (cout,))))
                cin = cout
        lins = []
        for k, c in enumerate(TAP_CHANNELS):
            names = (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight")
            key = next((n for n in names if n in sd), None)
            if key is None:
                raise KeyError(f"LpipsVGG: the state dict has neither '{names[0]}' nor '{names[1]}'")
            lins.append(_take(sd, key, (1, c, 1, 1)))
        shift, scale = SHIFT, SCALE
        if "scaling_layer.shift" in sd or "scaling_layer.scale" in sd:
            shift = _take(sd, "scaling_layer.shift", (1, 3, 1, 1)).reshape(-1).tolist()
            scale = _take(sd, "scaling_layer.scale", (1, 3, 1, 1)).reshape(-1).tolist()
        return cls(convs, lins, shift, scale, device)

    @classmethod
    def from_files(cls, vgg16_path, lin_path, device="cuda"):
        """From torchvision's VGG-16 checkpoint (features.{i}.weight / bias) and the package's weights/v0.1/vgg.pth."""
        vgg = torch.load(vgg16_path, map_location="cpu")
        lin = torch.load(lin_path, map_location="cpu")
        sd = {}
        for s, idx in enumerate(SLICES, 1):
            for i in idx:
                for what in ("weight", "bias"):
                    if f"features.{i}.{what}" not in vgg:
                        raise KeyError(f"LpipsVGG: {vgg16_path} has no 'features.{i}.{what}'")
                    sd[f"net.slice{s}.{i}.{what}"] = vgg[f"features.{i}.{what}"]
        sd.update({k: v for k, v in lin.items() if k.startswith(("lin", "scaling_layer"))})
        return cls.from_state_dict(sd, device)

    # ---- forward ----
    def _images(self, name, x):
        if not torch.is_tensor(x):
            raise RuntimeError(f"LpipsVGG: {name} must be a HIP tensor, got {type(x).__name__}")
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise RuntimeError(f"LpipsVGG: {name} must be (3, h, w) or (B, 3, h, w) float32, got {tuple(x.shape)} {x.dtype}")
        if x.shape[2] < MIN_SIDE or x.shape[3] < MIN_SIDE:
            raise ValueError(f"LpipsVGG: {name} is {x.shape[2]} x {x.shape[3]}; four 2 x 2 pools need h, w >= {MIN_SIDE}")
        if not x.is_cuda:
            raise RuntimeError(f"LpipsVGG: {name} must be a HIP tensor; humanliff_amd has no CPU path")
        self._upload()
        if x.device != self.device:
            raise RuntimeError(f"LpipsVGG: {name} is on {x.device}, the weights on {self.device}")
        return x.contiguous()

    def _workspace(self, n, h, w, keep=False):
        """The call's workspace.  __call__ reuses one grow-only buffer (`keep`): held-out crops all differ in size, and a fresh block per
        size would pile up in torch's caching allocator next to the renderer's memory.  Calls on one stream are ordered, so the
        buffer is free again when the next call's kernels start.  features() returns views into its workspace: a buffer of its own."""
        nbytes = _lib.lib().hl_lpips_workspace_bytes(n, h, w)
        if nbytes == 0:
            raise ValueError(f"LpipsVGG: {n} images of {h} x {w} are outside what hl_lpips serves")
        if not keep:
            return torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = None                         # (released before the larger one is taken)
            self._ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        return self._ws

    def _taps(self, ws, n, h, w):
        L = _lib.lib()
        out = []
        for k in range(5):
            off, hk, wk, ck = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
            _lib.check(L.hl_lpips_tap_shape(n, h, w, k, C.byref(off), C.byref(hk), C.byref(wk), C.byref(ck)), "hl_lpips_tap_shape")
            numel = n * hk.value * wk.value * ck.value
            out.append(ws[off.value // 4: off.value // 4 + numel].view(n, hk.value, wk.value, ck.value).permute(0, 3, 1, 2))
        return out

    def features(self, x):
        """The five taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of x as (B, C_k, h_k, w_k) tensors (channels-last in memory)."""
        x = self._images("x", x)
        n, _, h, w = x.shape
        ws = self._workspace(n, h, w)
        with _lib.on(self.device):
            _lib.check(_lib.lib().hl_lpips_features(C.byref(self._params), _lib.ptr(x), None, n, h, w, C.c_void_p(ws.data_ptr()), ws.numel() * 4,
                                                    _lib.stream_ptr(self.device)), "hl_lpips_features")
        return self._taps(ws, n, h, w)

    def __call__(self, in0, in1, retPerLayer=False):
        in0, in1 = self._images("in0", in0), self._images("in1", in1)
        if in0.shape != in1.shape:
            raise RuntimeError(f"LpipsVGG: in0 and in1 differ in shape: {tuple(in0.shape)}, {tuple(in1.shape)}")
        b, _, h, w = in0.shape
        ws = self._workspace(2 * b, h, w, keep=True)
        out = torch.empty((b, 6), dtype=torch.float64, device=self.device)
        with _lib.on(self.device):
            _lib.check(_lib.lib().hl_lpips(C.byref(self._params), _lib.ptr(in0), _lib.ptr(in1), b, h, w, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(ws.data_ptr()), ws.numel() * 4, _lib.stream_ptr(self.device)), "hl_lpips")
        out = out.float()
        val = out[:, 5].reshape(b, 1, 1, 1)
        if retPerLayer:
            return val, [out[:, k].reshape(b, 1, 1, 1) for k in range(5)]
        return val
