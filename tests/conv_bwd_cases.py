"""Backward-data convolutions (hl_conv2d_nhwc_bwd_data) by the kernel they reach, with their float64 and fp32-CPU references, and ragged
geometries for the weight-gradient kernels.

Plain functions, seeded torch.Generators, no GPU.  The backward-data of a convolution is the forward convolution of the output gradient
with the weights read flipped and channel-transposed (tf = 1) by the packer of whichever kernel family plan_conv picks, so every family
and its split-K variant has a transposed packing of its own.  CASES holds one case per (mode, kernel size, kernel, split or not) that
hl_conv2d_bwd_data_plan can answer on GRID - tests/test_conv_bwd_cpu.py proves that, and that every case is FAIR (fp32 CPU autograd on
the same operands within E_REF_MAX of float64) - and tests/test_conv_bwd_gpu.py holds the kernels to the project's standing bounds on
the identical tensors.  Every function returns the same bits on every call; cached results are shared and must not be written to.

What a case is compared with: float64 autograd of F.conv2d (on the nearest-x2 image where `ups`, with the given stride) on the operands
AS THE KERNEL ROUNDS THEM, read from the kernels:
  * the fp32 kernels (k_conv, k_conv_dma, k_conv_wino, k_conv_wino4, k_conv_wino4w), under whatever mode they were reached: unrounded;
  * k_conv_h16 / k_conv1_h16: dy and w rounded to nearest-even to the 16-bit type of the MODE THE CALL NAMES - bf16 under HL_CONV_BF16,
    fp16 under HL_CONV_FP16 (conv2d_single packs with f16 = (mode == HL_CONV_FP16) and conv2d launches the kernel with the same flag,
    also when tf = 1).  The training path itself never names HL_CONV_FP16 in a backward-data call: _Conv.backward turns the fp16 mode
    into HL_CONV_BF16 (gradients need fp32's exponent range), i.e. it makes the calls of the bf16 cases here.  The fp16 cases pin what the
    C ABI does when asked directly;
  * k_conv_bf3 under HL_CONV_BF16 (NPL = 1): dy rounded to bf16 to nearest-even (split3: u + 0x7fff + lsb), w cut to its two leading
    TRUNCATED bf16 planes - hi = the upper 16 bits of w, mid = the upper 16 bits of (w - hi), as k_pack_conv_bf3 splits it - the
    products ah*bm and ah*bh are exact in fp32 and accumulated in fp32.
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

E_REF_MAX = 5e-6          # the fairness condition, relative to max|dx|: a case whose fp32 reference misses it is redrawn or dropped, on the CPU

Case = collections.namedtuple("Case", "mode N Ho Wo Cy Cout Cin ks stride ups Cx kernel split")

# hl_conv2d_plan's kernel numbers (include/humanliff_hip.h); k_conv1_h16 shares k_conv_h16's
KERNELS = {0: "k_conv", 1: "k_conv_dma", 2: "k_conv_bf3", 3: "k_conv_wino", 4: "k_conv_wino4", 5: "k_conv_wino4w", 6: "k_conv_h16"}
WINOGRAD = ("k_conv_wino", "k_conv_wino4", "k_conv_wino4w")
MODES = ("fp32", "bf16", "fp16")


def _c(mode, N, Ho, Wo, Cy, Cin, ks, kernel, split, stride=1, ups=0, Cout=None, Cx=None):
    return Case(mode, N, Ho, Wo, Cy, Cy if Cout is None else Cout, Cin, ks, stride, ups, Cin if Cx is None else Cx, kernel, split)


# name -> (mode, N, Ho, Wo, Cy of dy -> Cin of dx, ks), the kernel the case is there for and whether it splits K.  Each shape is near the
# smallest of GRID that reaches its kernel; the 16-bit modes reach the fp32 kernels too (layers k_conv_h16 / k_conv_bf3 do not cover), with
# the fp32 shapes where those carry over so that the float64 reference is shared.
CASES = {
    # HL_CONV_FP32: Fp32, Wino2 and Wino4 forms
    "fp32_conv3": _c("fp32", 4, 64, 96, 32, 96, 3, "k_conv", False),
    "fp32_conv1": _c("fp32", 1, 32, 32, 96, 384, 1, "k_conv", False),
    "fp32_conv3_split": _c("fp32", 2, 32, 32, 64, 64, 3, "k_conv", True),
    "fp32_conv1_split": _c("fp32", 1, 8, 8, 384, 32, 1, "k_conv", True),
    "fp32_dma3_split": _c("fp32", 2, 24, 48, 96, 192, 3, "k_conv_dma", True),
    "fp32_dma1": _c("fp32", 1, 64, 96, 32, 384, 1, "k_conv_dma", False),
    "fp32_dma1_split": _c("fp32", 1, 16, 32, 768, 768, 1, "k_conv_dma", True),
    "fp32_wino_split": _c("fp32", 4, 32, 64, 96, 192, 3, "k_conv_wino", True),
    "fp32_wino": _c("fp32", 1, 64, 96, 32, 768, 3, "k_conv_wino", False),
    "fp32_wino4": _c("fp32", 2, 64, 96, 32, 768, 3, "k_conv_wino4", False),
    "fp32_wino4w": _c("fp32", 4, 64, 128, 32, 192, 3, "k_conv_wino4w", False),
    "fp32_wino4w_split": _c("fp32", 2, 64, 64, 192, 192, 3, "k_conv_wino4w", True),
    # geometry in front of / behind the convolution, off k_conv: stride 2 convolves the zero-stuffed 24 x 48 grid (and stores 192 real
    # channels in a pitch of 208), the upsample case sums 2x2 blocks of the 24 x 48 result
    "fp32_dma3_stride2_pitch": _c("fp32", 2, 12, 24, 96, 192, 3, "k_conv_dma", True, stride=2, Cx=208),
    "fp32_dma3_upsample": _c("fp32", 2, 24, 48, 96, 192, 3, "k_conv_dma", True, ups=1),
    # 27 real channels in a pitch of 32 (the input convolution; no other family takes 27 output channels), and 27 of the gradient's 32
    # channels covered by the weight (the output convolution)
    "fp32_conv3_cin27": _c("fp32", 1, 32, 32, 32, 27, 3, "k_conv", True, Cx=32),
    "fp32_conv3_cout27": _c("fp32", 1, 32, 32, 32, 32, 3, "k_conv", True, Cout=27),
    # both at once behind an upsample: the convolution stores into a zeroed (N, Ho, Wo, Cx) image, whose 2x2 sums fill all Cx channels of dx
    "fp32_conv3_upsample_cin27": _c("fp32", 1, 32, 32, 32, 27, 3, "k_conv", True, ups=1, Cx=32),
    # HL_CONV_BF16: Fp32, Bf16x3 and the 16-bit form in bf16
    "bf16_h16": _c("bf16", 1, 64, 96, 32, 384, 3, "k_conv_h16", False),
    "bf16_h16_split": _c("bf16", 1, 16, 16, 768, 768, 3, "k_conv_h16", True),
    "bf16_h16_1x1": _c("bf16", 1, 64, 96, 96, 384, 1, "k_conv_h16", False),
    "bf16_bf3_split": _c("bf16", 1, 16, 16, 192, 768, 3, "k_conv_bf3", True),
    "bf16_bf3_1x1": _c("bf16", 1, 64, 96, 32, 384, 1, "k_conv_bf3", False),
    "bf16_bf3_1x1_split": _c("bf16", 1, 16, 32, 768, 768, 1, "k_conv_bf3", True),
    "bf16_conv3": _c("bf16", 4, 64, 96, 32, 96, 3, "k_conv", False),
    "bf16_conv1": _c("bf16", 1, 32, 32, 96, 384, 1, "k_conv", False),
    "bf16_conv3_split": _c("bf16", 2, 32, 32, 64, 64, 3, "k_conv", True),
    "bf16_conv1_split": _c("bf16", 1, 8, 8, 384, 32, 1, "k_conv", True),
    # HL_CONV_FP16: Fp32, Wino2, Wino4 and the 16-bit form in fp16
    "fp16_h16": _c("fp16", 1, 64, 96, 32, 384, 3, "k_conv_h16", False),
    "fp16_h16_split": _c("fp16", 1, 16, 16, 768, 768, 3, "k_conv_h16", True),
    "fp16_h16_1x1": _c("fp16", 1, 64, 96, 96, 384, 1, "k_conv_h16", False),
    "fp16_dma3_split": _c("fp16", 2, 24, 48, 96, 192, 3, "k_conv_dma", True),
    "fp16_dma1": _c("fp16", 1, 64, 96, 32, 384, 1, "k_conv_dma", False),
    "fp16_dma1_split": _c("fp16", 1, 16, 32, 768, 768, 1, "k_conv_dma", True),
    "fp16_wino_split": _c("fp16", 4, 32, 64, 96, 192, 3, "k_conv_wino", True),
    "fp16_conv3": _c("fp16", 4, 64, 96, 32, 96, 3, "k_conv", False),
    "fp16_conv1": _c("fp16", 1, 32, 32, 96, 384, 1, "k_conv", False),
    "fp16_conv3_split": _c("fp16", 2, 32, 32, 64, 64, 3, "k_conv", True),
    "fp16_conv1_split": _c("fp16", 1, 8, 8, 384, 32, 1, "k_conv", True),
}

# the grid the coverage test scans with hl_conv2d_bwd_data_plan: stride 1, no upsample, Cout = Cy, Cx = Cin
GRID = dict(N=(1, 2, 4),
            sizes=((8, 8), (16, 16), (16, 32), (24, 48), (32, 32), (32, 64), (64, 64), (64, 96), (64, 128), (96, 96), (128, 128)),
            channels=(32, 64, 96, 192, 384, 768), ks=(3, 1), modes=MODES)
# the kernels a mode's weight forms (conv_forms(mode, true, true)) and a kernel size admit; the Winograd kernels are 3x3 only
MODE_KERNELS = {"fp32": ("k_conv", "k_conv_dma", "k_conv_wino", "k_conv_wino4", "k_conv_wino4w"),
                "bf16": ("k_conv", "k_conv_bf3", "k_conv_h16"),
                "fp16": ("k_conv", "k_conv_dma", "k_conv_wino", "k_conv_wino4", "k_conv_wino4w", "k_conv_h16")}
# (mode, ks, kernel, split) of that universe which GRID cannot reach at all, each with the line of plan_conv that keeps it out
UNREACHABLE = {
    ("fp32", 3, "k_conv_dma", False): "a 3x3 layer that fills the DMA tile unsplit has whole 8x16 tiles and 64-multiple channels here: Winograd takes it first",
    ("fp32", 3, "k_conv_wino4", True): "k_conv_wino4 is only taken with one slab (the split goes to k_conv_wino4w)",
    ("bf16", 3, "k_conv_bf3", False): "a 3x3 layer that fills the DMA tile unsplit has 192-multiple channels on whole 16x16 tiles here: k_conv_h16 takes it first",
    ("bf16", 1, "k_conv_h16", True): "k_conv1_h16 never splits K (want = 0 unless ks == 3)",
    ("fp16", 3, "k_conv_dma", False): "as under fp32",
    ("fp16", 3, "k_conv_wino", False): "an F(2x2) layer that fills the chip unsplit has 192-multiple channels on whole 16x16 tiles here: k_conv_h16 takes it first",
    ("fp16", 3, "k_conv_wino4", False): "as k_conv_wino: k_conv_h16 takes every layer the F(4x4) kernels would fill",
    ("fp16", 3, "k_conv_wino4", True): "as under fp32",
    ("fp16", 3, "k_conv_wino4w", False): "as k_conv_wino4",
    ("fp16", 3, "k_conv_wino4w", True): "its split needs 64-multiple channels on the DMA tile (so 192-multiples) and 16x32 tiles: k_conv_h16 splits those first",
    ("fp16", 1, "k_conv_h16", True): "as under bf16",
}


def x_hw(c):
    """H, W of dx."""
    return (2 * c.Ho, 2 * c.Wo) if c.stride == 2 else (c.Ho // 2, c.Wo // 2) if c.ups else (c.Ho, c.Wo)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _shape_key(c):
    return (c.N, c.Ho, c.Wo, c.Cout, c.Cin, c.ks, c.stride, c.ups)


@functools.lru_cache(maxsize=None)
def _operands(key):
    """dy ~ randn (N, Cout, Ho, Wo), w ~ randn / sqrt(Cout ks^2) (Cout, Cin, ks, ks): dx is O(1).  Drawn per geometry, so that the cases
    of different modes on one shape share tensors (and references)."""
    N, Ho, Wo, Cout, Cin, ks, _, _ = key
    g = _gen("conv_bwd", key)
    return torch.randn((N, Cout, Ho, Wo), generator=g), torch.randn((Cout, Cin, ks, ks), generator=g) / (Cout * ks * ks) ** 0.5


def operands(c):
    return _operands(_shape_key(c))


def bf16_planes2(w):
    """w cut to its two leading truncated bf16 planes, as k_pack_conv_bf3 splits it (fp32 in, fp32 out: 16 significand bits at most)."""
    hi = (w.view(torch.int32) & -65536).view(torch.float32)
    r1 = w - hi                                                     # exact
    mid = (r1.view(torch.int32) & -65536).view(torch.float32)
    return hi + mid                                                 # exact: the planes do not overlap


def _rounding(kernel, mode):
    if kernel == "k_conv_h16":
        dt = torch.bfloat16 if mode == "bf16" else torch.float16
        r = lambda t: t.to(dt).float()  # noqa: E731
        return r, r
    if kernel == "k_conv_bf3":
        return (lambda t: t.to(torch.bfloat16).float()), bf16_planes2
    return None


def rounding(c):
    """What the case's kernel does to (dy, w) before it multiplies: None (fp32 kernels) or a pair of functions fp32 -> fp32."""
    return _rounding(c.kernel, c.mode)


def _grad(dy, w, c):
    """d input of F.conv2d by autograd, in the dtype of the operands -> (N, Cin, H, W)."""
    H, W = x_hw(c)
    x = torch.zeros((c.N, c.Cin, H, W), dtype=dy.dtype, requires_grad=True)
    xi = F.interpolate(x, scale_factor=2, mode="nearest") if c.ups else x
    y = F.conv2d(xi, w, None, stride=c.stride, padding=c.ks // 2)
    assert y.shape == dy.shape, (tuple(y.shape), tuple(dy.shape))
    return torch.autograd.grad(y, x, dy)[0]


@functools.lru_cache(maxsize=None)
def _reference(key, rnd, c):
    dy, w = _operands(key)
    if rnd is not None:
        fy, fw = _rounding(*rnd)
        dy, w = fy(dy), fw(w)
    want = _grad(dy.double(), w.double(), c)
    ref32 = _grad(dy, w, c)
    scale = float(want.abs().max())
    return dict(want=want, ref32=ref32, scale=scale, e_ref=float((ref32.double() - want).abs().max()))


def reference(c):
    """want: float64 dx (N, Cin, H, W) of the operands as the case's kernel rounds them; ref32: fp32 CPU autograd on the same operands;
    e_ref = max|ref32 - want|; scale = max|want|; exact: float64 dx of the unrounded operands (= want for the fp32 kernels)."""
    rnd = None if rounding(c) is None else (c.kernel, c.mode)
    geom = c._replace(mode="", kernel="", split=False, Cy=0, Cx=0)          # what _grad reads
    r = dict(_reference(_shape_key(c), rnd, geom))
    r["exact"] = r["want"] if rnd is None else _reference(_shape_key(c), None, geom)["want"]
    return r


def abi_args(c):
    """The arguments of hl_conv2d_bwd_data_plan / _scratch_bytes after the mode."""
    return (c.N, c.Ho, c.Wo, c.Cy, c.Cout, c.Cin, c.ks, c.stride, c.ups, c.Cx)


# ---- ragged geometries for the weight-gradient kernels, through _Conv.apply --------------------------------------------------------------
Wgrad = collections.namedtuple("Wgrad", "N Cin Cout H W ks stride ups")
WGRAD_CASES = {
    "stride2_ragged": Wgrad(3, 96, 160, 20, 24, 3, 2, 0),     # k_conv_wgrad_t<2>: 10 x 12 outputs = ragged 4x8 tiles, slabs that cross images
    "upsample_odd": Wgrad(2, 64, 96, 5, 7, 3, 1, 1),          # k_conv_wgrad_t<1> / k_conv_wgrad_h16 behind the nearest-x2 of an odd source
    "1x1_ragged": Wgrad(3, 80, 100, 5, 7, 1, 1, 0),           # k_conv_wgrad_1x1: Cout below one 192-block, 105 pixels (not a multiple of 64)
}


@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """x (N,Cin,H,W), w, b, cot (the output gradient) and the float64 results of the unrounded operands: y, dx, dw, db; dw16 = the float64
    weight gradient of x and cot rounded to bf16 (what k_conv_wgrad_h16 computes in the 16-bit modes: 3x3 / stride-1 layers only -
    hl_conv2d_wgrad_nhwc_ws_mode - the others stay fp32, dw16 is None)."""
    g = WGRAD_CASES[name]
    gen = _gen("wgrad", name)
    x = torch.randn((g.N, g.Cin, g.H, g.W), generator=gen)
    w = torch.randn((g.Cout, g.Cin, g.ks, g.ks), generator=gen) / (g.Cin * g.ks * g.ks) ** 0.5
    b = torch.randn((g.Cout,), generator=gen)

    def fwd(xx, ww, bb):
        xi = F.interpolate(xx, scale_factor=2, mode="nearest") if g.ups else xx
        return F.conv2d(xi, ww, bb, stride=g.stride, padding=g.ks // 2)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = fwd(xr, wr, br)
    cot = torch.randn(yr.shape, generator=gen)
    (yr * cot.double()).sum().backward()
    dw16 = None
    if g.ks == 3 and g.stride == 1:
        w2 = w.double().requires_grad_(True)
        (fwd(x.to(torch.bfloat16).double(), w2, None) * cot.to(torch.bfloat16).double()).sum().backward()
        dw16 = w2.grad
    return dict(geom=g, x=x, w=w, b=b, cot=cot, y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad, dw16=dw16)
