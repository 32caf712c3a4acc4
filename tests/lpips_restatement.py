"""A restatement of lpips.LPIPS(net='vgg', version='0.1') in eval mode from plain F.conv2d / F.max_pool2d, in the dtype of its
weights (float64 is the tests' reference, float32 is what the package computes), and a small nn.Module twin whose submodule names
reproduce the package's state-dict keys.  Neither `lpips` nor `torchvision` is imported: the network is written out here.

    x = (in - shift) / scale
    torchvision VGG-16 features[0:30]: 3 x 3 / pad 1 convolutions + ReLU, widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512,
    MaxPool2d(2, 2) (floor mode) at each |; taps = the ReLU outputs at features indices 3, 8, 15, 22, 29
    n(f) = f / (sqrt(sum_c f^2) + 1e-10);  d_k = mean_{y,x} sum_c lin_k[c] (n(f0) - n(f1))^2;  result = sum_k d_k
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))
# torchvision's features indices of the convolutions of each block (the package's slice1..slice5 keep those indices as names)
CONV_INDEX = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
TAP_CHANNELS = tuple(b[-1] for b in BLOCKS)


def taps(convs, x, shift=SHIFT, scale=SCALE):
    """The five tap tensors of x (B, 3, h, w); convs: 13 (weight, bias) in network order, of x's dtype."""
    # (the package keeps shift and scale as float32 buffers: those values, widened when x is float64)
    x = (x - torch.tensor(shift, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)) / torch.tensor(scale, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    out, it = [], iter(convs)
    for k, block in enumerate(BLOCKS):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for _ in block:
            w, b = next(it)
            x = F.relu(F.conv2d(x, w, b, padding=1))
        out.append(x)
    return out


def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def head(lins, f0, f1):
    """([d_1 .. d_5], their sum), each (B, 1, 1, 1); lins: 5 weights (1, C, 1, 1)."""
    terms = []
    for k in range(5):
        diff = (normalize_tensor(f0[k]) - normalize_tensor(f1[k])) ** 2
        terms.append(F.conv2d(diff, lins[k]).mean([2, 3], keepdim=True))
    val = terms[0]
    for k in range(1, 5):
        val = val + terms[k]
    return terms, val


def lpips(convs, lins, in0, in1):
    return head(lins, taps(convs, in0), taps(convs, in1))


def cast(convs, lins, dtype):
    return [(w.to(dtype), b.to(dtype)) for w, b in convs], [l.to(dtype) for l in lins]


# ---- the twin: the package's module tree, as far as its state-dict keys go ----
class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.Tensor(SHIFT)[None, :, None, None])
        self.register_buffer('scale', torch.Tensor(SCALE)[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class _NetLinLayer(nn.Module):
    def __init__(self, chn_in):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))

    def forward(self, x):
        return self.model(x)


class _Vgg16(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for k, block in enumerate(BLOCKS):
            if k:
                layers.append(nn.MaxPool2d(2, 2))
            for cout in block:
                layers += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(inplace=False)]
                cin = cout
        bounds = (0, 4, 9, 16, 23, 30)
        for s in range(5):
            seq = nn.Sequential()
            for i in range(bounds[s], bounds[s + 1]):
                seq.add_module(str(i), layers[i])
            setattr(self, f"slice{s + 1}", seq)

    def forward(self, x):
        out = []
        for s in range(5):
            x = getattr(self, f"slice{s + 1}")(x)
            out.append(x)
        return out


class Twin(nn.Module):
    """Same submodule names as lpips.LPIPS(net='vgg'): net.slice{1..5}.{i}, scaling_layer, lin0..lin4 and the lins ModuleList over them."""

    def __init__(self, convs, lins):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _Vgg16()
        for k, c in enumerate(TAP_CHANNELS):
            setattr(self, f"lin{k}", _NetLinLayer(c))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(5)])
        it = iter(convs)
        with torch.no_grad():
            for s, idx in enumerate(CONV_INDEX, 1):
                for i in idx:
                    w, b = next(it)
                    conv = getattr(self.net, f"slice{s}")[i - (0, 4, 9, 16, 23)[s - 1]]
                    conv.weight.copy_(w)
                    conv.bias.copy_(b)
            for k in range(5):
                self.lins[k].model[1].weight.copy_(lins[k])
        self.eval()

    def forward(self, in0, in1, retPerLayer=False):
        f0, f1 = self.net(self.scaling_layer(in0)), self.net(self.scaling_layer(in1))
        res = [self.lins[k]((normalize_tensor(f0[k]) - normalize_tensor(f1[k])) ** 2).mean([2, 3], keepdim=True) for k in range(5)]
        val = res[0]
        for k in range(1, 5):
            val = val + res[k]
        return (val, res) if retPerLayer else val
