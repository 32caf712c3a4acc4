"""Forward convolutions (hl_conv2d_nhwc_mode / hl_conv2d_nhwc_gn) by the kernel INSTANTIATION they launch, with their float64 and fp32-CPU
references.

Plain functions, seeded torch.Generators, no GPU; the helpers of tests/conv_bwd_cases.py are reused.  A case is one instantiation, keyed by
    (kernel, tile, ks, stride, ups, GroupNorm handling, split-K or not, operand arithmetic)
  * tile: k_conv's cfg (0 = 128x96, 1 = 128x32, 2 = 64x64), the waves of k_conv_dma / k_conv_bf3 (4 or 8), None for the other kernels;
  * GroupNorm handling: "none"; "affine" / "affine_silu" - applied by the convolution kernel while it stages (k_conv's template mode, the
    fp16x2 kernels' staging); or the pre-pass that materialises it: "dense" (k_gn_apply, fp32), "blocked" (k_gn_apply_blk, fp32 [C/8][pixel][8]:
    k_conv_wino4<., true>, the blk form of k_conv_wino4w), "half" (k_gn_apply_h16, the 16-bit image of k_conv_h16), "twoplane" (two fp16 planes,
    k_conv_h2s).  A pre-pass takes SiLU as an argument, so it is no part of the key there; the table runs both (but see DROPPED);
  * arithmetic: "fp32", "fp16x2" (two fp16 planes per operand), "bf16x3" (three bf16 planes, HL_CONV_BF16X3), "bf16w2" (k_conv_bf3 under
    HL_CONV_BF16: activations rounded to bf16, two truncated weight planes), "fp16" / "bf16" (k_conv_h16 / k_conv1_h16).
and names the one HL_CONV_* mode it is run under.  ALL_CASES holds one case per key that any of the seven modes reaches on GRID (Cin 16 and 48
included: with every Cin a multiple of 32 the default mode never leaves k_conv_h2s for the Winograd kernels on a plain 3x3 layer), at the smallest
N H W Cin Cout of the grid that reaches it (ties: the default mode first), and below them the edges the kernels accept (ragged pixel
tiles and tiles that straddle images, Cout 27 and Cout off the 64-multiples, Cin 16, 1x1 with stride 2 / behind the upsample, the smallest
legal image of the tile-exact kernels).  tests/test_conv_fwd_cpu.py proves with hl_conv2d_plan_ex (host arithmetic) that every case
launches its key, that no key the grid reaches lacks a case, that the keys of UNIVERSE the grid cannot reach are exactly UNREACHABLE, and that
every case of CASES (= ALL_CASES without DROPPED, at the end of this file) is FAIR; tests/test_conv_fwd_gpu.py holds the kernels to the suite's
standing bounds on the identical tensors.

Operands (tests/test_conv_h2s_tiles_gpu.py's): x = 1.5 randn, w = randn / sqrt(ks^2 Cin) times a per-output-channel power of two in
[2^-6, 1], bias = 0.1 randn, GroupNorm coefficients A in [0.5, 1.5), B = 0.1 randn, residual = randn; drawn per geometry, so the cases of
different modes on one shape share tensors and references.

What a case is compared with: float64 F.conv2d of the operands AS THE KERNEL ROUNDS THEM - on the nearest-x2 image where ups, after float64
x*A + B (then SiLU) where a GroupNorm is in front, plus the residual.  Read from the kernels (see also conv_bwd_cases.py):
  * fp32 kernels, the fp16x2 kernels and the bf16x3 emulation: unrounded (their bounds are relative to the direct fp32 kernel);
  * k_conv_h16 / k_conv1_h16: activations and weights rounded to nearest-even to the type the mode names;
  * k_conv_bf3 under HL_CONV_BF16: activations rounded to bf16 to nearest-even, the weights' two leading truncated bf16 planes;
  * behind a "half" pre-pass, or a "dense" one in front of k_conv_bf3 under HL_CONV_BF16, the rounding applies to the float64 GroupNorm
    output.  The kernel forms it in fp32, so some activations round the other way; the fp32 restatement (ref32) meets the same flips, which is
    why such cases are held to norm_cases.bar(E_ref) and why those whose E_ref misses the fairness condition are DROPPED below, not loosened.
"""
import collections
import functools
import itertools

import torch
import torch.nn.functional as F

from tests.conv_bwd_cases import E_REF_MAX, _gen, bf16_planes2  # noqa: F401  (E_REF_MAX: the fairness condition, relative to max|y|)

Case = collections.namedtuple("Case", "mode N H W Cin Cout ks stride ups kernel tile gn split arith silu res bias stats")

MODES = ("fp32", "bf16x3", "direct", "f23", "bf16", "fp16", "mfma")      # -> _lib.HL_CONV_*: mode_number()
# hl_conv2d_plan_ex's numbers (include/humanliff_hip.h)
KERNELS = {0: "k_conv", 1: "k_conv_dma", 2: "k_conv_bf3", 3: "k_conv_wino", 4: "k_conv_wino4", 5: "k_conv_wino4w", 6: "k_conv_h16", 7: "k_conv_h2s",
           8: "k_conv1_h2s", 9: "k_conv_h2d", 10: "k_conv_h2s_ph"}
PRE = {0: None, 1: "dense", 2: "blocked", 3: "half", 4: "twoplane"}
STATS_BY = {0: "none", 1: "epilogue", 2: "finish"}
PLAN_FIELDS = ("kernel", "splits", "cfg", "tile8", "gn_mode", "pre", "stats_by", "stat_slots", "kt_per")
FP16X2 = ("k_conv_h2s", "k_conv1_h2s", "k_conv_h2d", "k_conv_h2s_ph")
KINDS = {"3x3": (3, 1, 0), "3x3s2": (3, 2, 0), "3x3up": (3, 1, 1), "1x1": (1, 1, 0), "1x1s2": (1, 2, 0), "1x1up": (1, 1, 1)}

# name  mode  N H W Cin Cout  kind  kernel  tile  GroupNorm  split-K  arithmetic  flags (res: a residual, nobias: a null bias, silu: SiLU in a
# pre-pass, stats:<who>: run through hl_conv2d_nhwc_gn, and who adds the output statistics)
_TABLE = """
conv1_1x1_affine fp32 1 8 8 16 27 1x1 k_conv 1 affine whole fp32 res
conv1_1x1_affine_split fp32 1 8 8 384 27 1x1 k_conv 1 affine split fp32 -
conv1_1x1_affine_silu fp32 1 8 8 16 27 1x1 k_conv 1 affine_silu whole fp32 res,nobias
conv1_1x1_affine_silu_split fp32 1 8 8 384 27 1x1 k_conv 1 affine_silu split fp32 -
conv1_1x1 fp32 1 8 8 16 27 1x1 k_conv 1 none whole fp32 res
conv1_1x1_split fp32 1 8 8 384 27 1x1 k_conv 1 none split fp32 nobias
conv1_3x3_affine fp32 1 8 8 16 27 3x3 k_conv 1 affine whole fp32 res
conv1_3x3_affine_split fp32 1 8 8 32 27 3x3 k_conv 1 affine split fp32 -
conv1_3x3_affine_silu fp32 1 8 8 16 27 3x3 k_conv 1 affine_silu whole fp32 res,nobias
conv1_3x3_affine_silu_split fp32 1 8 8 32 27 3x3 k_conv 1 affine_silu split fp32 -
conv1_3x3 fp32 1 8 8 16 27 3x3 k_conv 1 none whole fp32 res
conv1_3x3_split fp32 1 8 8 32 27 3x3 k_conv 1 none split fp32 nobias
conv1_3x3up fp32 1 8 8 16 27 3x3up k_conv 1 none whole fp32 res
conv1_3x3up_split fp32 1 8 8 32 27 3x3up k_conv 1 none split fp32 -
conv1_3x3s2_affine fp32 1 8 8 16 27 3x3s2 k_conv 1 affine whole fp32 res,nobias
conv1_3x3s2_affine_split fp32 1 8 8 32 27 3x3s2 k_conv 1 affine split fp32 -
conv1_3x3s2_affine_silu fp32 1 8 8 16 27 3x3s2 k_conv 1 affine_silu whole fp32 res
conv1_3x3s2_affine_silu_split fp32 1 8 8 32 27 3x3s2 k_conv 1 affine_silu split fp32 nobias
conv1_3x3s2 fp32 1 8 8 16 27 3x3s2 k_conv 1 none whole fp32 res
conv1_3x3s2_split fp32 1 8 8 32 27 3x3s2 k_conv 1 none split fp32 -
conv2_1x1_affine fp32 1 8 8 16 64 1x1 k_conv 2 affine whole fp32 res,nobias
conv2_1x1_affine_split fp32 1 8 8 384 64 1x1 k_conv 2 affine split fp32 -
conv2_1x1_affine_silu fp32 1 8 8 16 64 1x1 k_conv 2 affine_silu whole fp32 res
conv2_1x1_affine_silu_split fp32 1 8 8 384 64 1x1 k_conv 2 affine_silu split fp32 nobias
conv2_1x1 fp32 1 8 8 16 64 1x1 k_conv 2 none whole fp32 res
conv2_1x1_split fp32 1 8 8 384 64 1x1 k_conv 2 none split fp32 -
conv2_3x3_affine fp32 1 8 8 16 64 3x3 k_conv 2 affine whole fp32 res,nobias
conv2_3x3_affine_split fp32 1 8 8 32 64 3x3 k_conv 2 affine split fp32 -
conv2_3x3_affine_silu fp32 1 8 8 16 64 3x3 k_conv 2 affine_silu whole fp32 res
conv2_3x3_affine_silu_split fp32 1 8 8 32 64 3x3 k_conv 2 affine_silu split fp32 nobias
conv2_3x3 fp32 1 8 8 16 64 3x3 k_conv 2 none whole fp32 res,stats:none
conv2_3x3_split fp32 1 8 8 32 64 3x3 k_conv 2 none split fp32 stats:finish
conv2_3x3up fp32 1 8 8 16 64 3x3up k_conv 2 none whole fp32 res,nobias
conv2_3x3up_split fp32 1 8 8 32 64 3x3up k_conv 2 none split fp32 -
conv2_3x3s2_affine fp32 1 8 8 16 64 3x3s2 k_conv 2 affine whole fp32 res
conv2_3x3s2_affine_split fp32 1 8 8 32 64 3x3s2 k_conv 2 affine split fp32 nobias
conv2_3x3s2_affine_silu fp32 1 8 8 16 64 3x3s2 k_conv 2 affine_silu whole fp32 res
conv2_3x3s2_affine_silu_split fp32 1 8 8 32 64 3x3s2 k_conv 2 affine_silu split fp32 -
conv2_3x3s2 fp32 1 8 8 16 64 3x3s2 k_conv 2 none whole fp32 res,nobias
conv2_3x3s2_split fp32 1 8 8 32 64 3x3s2 k_conv 2 none split fp32 -
dma4_1x1_dense fp32 1 64 96 16 384 1x1 k_conv_dma 4 dense whole fp32 res,silu
dma4_1x1_dense_split fp32 1 16 32 768 768 1x1 k_conv_dma 4 dense split fp32 nobias
dma4_1x1 fp32 1 64 96 16 384 1x1 k_conv_dma 4 none whole fp32 res
dma4_1x1_split fp32 1 16 32 768 768 1x1 k_conv_dma 4 none split fp32 -
dma4_3x3_dense fp32 1 64 96 16 384 3x3 k_conv_dma 4 dense whole fp32 res,nobias,silu
dma4_3x3_dense_split fp32 1 16 16 192 768 3x3 k_conv_dma 4 dense split fp32 -
dma4_3x3 fp32 1 64 96 16 384 3x3 k_conv_dma 4 none whole fp32 res,stats:epilogue
dma4_3x3_split fp32 1 16 16 192 768 3x3 k_conv_dma 4 none split fp32 nobias,stats:finish
dma4_3x3up fp32 1 32 32 16 768 3x3up k_conv_dma 4 none whole fp32 res
dma4_3x3up_split fp32 1 8 8 192 768 3x3up k_conv_dma 4 none split fp32 -
dma4_3x3s2_dense fp32 2 64 96 16 768 3x3s2 k_conv_dma 4 dense whole fp32 res,nobias,silu
dma4_3x3s2_dense_split fp32 1 32 32 192 768 3x3s2 k_conv_dma 4 dense split fp32 -
dma4_3x3s2 fp32 2 64 96 16 768 3x3s2 k_conv_dma 4 none whole fp32 res
dma4_3x3s2_split fp32 1 32 32 192 768 3x3s2 k_conv_dma 4 none split fp32 nobias
dma8_1x1_dense fp32 1 64 128 16 768 1x1 k_conv_dma 8 dense whole fp32 res,silu
dma8_1x1_dense_split mfma 1 64 128 384 768 1x1 k_conv_dma 8 dense split fp32 -
dma8_1x1 fp32 1 64 128 16 768 1x1 k_conv_dma 8 none whole fp32 res,nobias,stats:epilogue
dma8_1x1_split mfma 1 64 128 384 768 1x1 k_conv_dma 8 none split fp32 -
dma8_3x3_dense direct 1 64 128 16 768 3x3 k_conv_dma 8 dense whole fp32 res,silu
dma8_3x3_dense_split direct 1 64 128 32 768 3x3 k_conv_dma 8 dense split fp32 nobias
dma8_3x3 direct 1 64 128 16 768 3x3 k_conv_dma 8 none whole fp32 res
dma8_3x3_split direct 1 64 128 32 768 3x3 k_conv_dma 8 none split fp32 -
dma8_3x3up direct 1 32 64 16 768 3x3up k_conv_dma 8 none whole fp32 res,nobias
dma8_3x3up_split direct 1 32 64 32 768 3x3up k_conv_dma 8 none split fp32 -
dma8_3x3s2_dense fp32 2 128 128 16 768 3x3s2 k_conv_dma 8 dense whole fp32 res,silu
dma8_3x3s2_dense_split fp32 2 128 128 32 768 3x3s2 k_conv_dma 8 dense split fp32 nobias
dma8_3x3s2 fp32 2 128 128 16 768 3x3s2 k_conv_dma 8 none whole fp32 res
dma8_3x3s2_split mfma 2 128 128 32 768 3x3s2 k_conv_dma 8 none split fp32 -
bf34_bf16w2_1x1_dense bf16 1 64 96 16 384 1x1 k_conv_bf3 4 dense whole bf16w2 res,nobias
bf34_bf16w2_1x1_dense_split bf16 1 16 32 768 768 1x1 k_conv_bf3 4 dense split bf16w2 -
bf34_bf16w2_1x1 bf16 1 64 96 16 384 1x1 k_conv_bf3 4 none whole bf16w2 res
bf34_bf16w2_1x1_split bf16 1 16 32 768 768 1x1 k_conv_bf3 4 none split bf16w2 nobias
bf34_bf16w2_3x3_dense bf16 1 64 96 16 384 3x3 k_conv_bf3 4 dense whole bf16w2 res
bf34_bf16w2_3x3_dense_split bf16 1 16 16 192 768 3x3 k_conv_bf3 4 dense split bf16w2 -
bf34_bf16w2_3x3 bf16 1 64 96 16 384 3x3 k_conv_bf3 4 none whole bf16w2 res,nobias
bf34_bf16w2_3x3_split bf16 1 16 16 192 768 3x3 k_conv_bf3 4 none split bf16w2 -
bf34_bf16w2_3x3up bf16 1 32 32 16 768 3x3up k_conv_bf3 4 none whole bf16w2 res
bf34_bf16w2_3x3up_split bf16 1 8 8 192 768 3x3up k_conv_bf3 4 none split bf16w2 nobias
bf34_bf16w2_3x3s2_dense bf16 2 64 96 16 768 3x3s2 k_conv_bf3 4 dense whole bf16w2 res
bf34_bf16w2_3x3s2_dense_split bf16 1 32 32 192 768 3x3s2 k_conv_bf3 4 dense split bf16w2 -
bf34_bf16w2_3x3s2 bf16 2 64 96 16 768 3x3s2 k_conv_bf3 4 none whole bf16w2 res,nobias
bf34_bf16w2_3x3s2_split bf16 1 32 32 192 768 3x3s2 k_conv_bf3 4 none split bf16w2 -
bf38_bf16w2_1x1_dense bf16 1 64 128 16 768 1x1 k_conv_bf3 8 dense whole bf16w2 res
bf38_bf16w2_1x1 bf16 1 64 128 16 768 1x1 k_conv_bf3 8 none whole bf16w2 nobias
bf38_bf16w2_3x3_dense bf16 1 64 128 16 768 3x3 k_conv_bf3 8 dense whole bf16w2 res
bf38_bf16w2_3x3_dense_split bf16 1 64 128 48 768 3x3 k_conv_bf3 8 dense split bf16w2 -
bf38_bf16w2_3x3 bf16 1 64 128 16 768 3x3 k_conv_bf3 8 none whole bf16w2 res,nobias
bf38_bf16w2_3x3_split bf16 1 64 128 48 768 3x3 k_conv_bf3 8 none split bf16w2 -
bf38_bf16w2_3x3up bf16 1 32 64 16 768 3x3up k_conv_bf3 8 none whole bf16w2 res
bf38_bf16w2_3x3up_split bf16 1 32 64 48 768 3x3up k_conv_bf3 8 none split bf16w2 nobias
bf38_bf16w2_3x3s2_dense bf16 2 128 128 16 768 3x3s2 k_conv_bf3 8 dense whole bf16w2 res
bf38_bf16w2_3x3s2_dense_split bf16 2 128 128 32 768 3x3s2 k_conv_bf3 8 dense split bf16w2 -
bf38_bf16w2_3x3s2 bf16 2 128 128 16 768 3x3s2 k_conv_bf3 8 none whole bf16w2 res,nobias
bf38_bf16w2_3x3s2_split bf16 2 128 128 32 768 3x3s2 k_conv_bf3 8 none split bf16w2 -
bf34_bf16x3_1x1_dense bf16x3 1 64 96 16 384 1x1 k_conv_bf3 4 dense whole bf16x3 res,silu
bf34_bf16x3_1x1_dense_split bf16x3 1 16 32 768 768 1x1 k_conv_bf3 4 dense split bf16x3 nobias
bf34_bf16x3_1x1 bf16x3 1 64 96 16 384 1x1 k_conv_bf3 4 none whole bf16x3 res,stats:none
bf34_bf16x3_1x1_split bf16x3 1 16 32 768 768 1x1 k_conv_bf3 4 none split bf16x3 -
bf34_bf16x3_3x3_dense bf16x3 1 64 96 16 384 3x3 k_conv_bf3 4 dense whole bf16x3 res,nobias,silu
bf34_bf16x3_3x3_dense_split bf16x3 1 16 16 192 768 3x3 k_conv_bf3 4 dense split bf16x3 -
bf34_bf16x3_3x3 bf16x3 1 64 96 16 384 3x3 k_conv_bf3 4 none whole bf16x3 res
bf34_bf16x3_3x3_split bf16x3 1 16 16 192 768 3x3 k_conv_bf3 4 none split bf16x3 nobias
bf34_bf16x3_3x3up bf16x3 1 32 32 16 768 3x3up k_conv_bf3 4 none whole bf16x3 res
bf34_bf16x3_3x3up_split bf16x3 1 8 8 192 768 3x3up k_conv_bf3 4 none split bf16x3 -
bf34_bf16x3_3x3s2_dense bf16x3 2 64 96 16 768 3x3s2 k_conv_bf3 4 dense whole bf16x3 res,nobias,silu
bf34_bf16x3_3x3s2_dense_split bf16x3 1 32 32 192 768 3x3s2 k_conv_bf3 4 dense split bf16x3 -
bf34_bf16x3_3x3s2 bf16x3 2 64 96 16 768 3x3s2 k_conv_bf3 4 none whole bf16x3 res
bf34_bf16x3_3x3s2_split bf16x3 1 32 32 192 768 3x3s2 k_conv_bf3 4 none split bf16x3 nobias
bf38_bf16x3_1x1_dense bf16x3 1 64 128 16 768 1x1 k_conv_bf3 8 dense whole bf16x3 res,silu
bf38_bf16x3_1x1_dense_split bf16x3 1 64 128 384 768 1x1 k_conv_bf3 8 dense split bf16x3 -
bf38_bf16x3_1x1 bf16x3 1 64 128 16 768 1x1 k_conv_bf3 8 none whole bf16x3 res,nobias
bf38_bf16x3_1x1_split bf16x3 1 64 128 384 768 1x1 k_conv_bf3 8 none split bf16x3 -
bf38_bf16x3_3x3_dense bf16x3 1 64 128 16 768 3x3 k_conv_bf3 8 dense whole bf16x3 res,silu
bf38_bf16x3_3x3_dense_split bf16x3 1 64 128 32 768 3x3 k_conv_bf3 8 dense split bf16x3 nobias
bf38_bf16x3_3x3 bf16x3 1 64 128 16 768 3x3 k_conv_bf3 8 none whole bf16x3 res
bf38_bf16x3_3x3_split bf16x3 1 64 128 32 768 3x3 k_conv_bf3 8 none split bf16x3 -
bf38_bf16x3_3x3up bf16x3 1 32 64 16 768 3x3up k_conv_bf3 8 none whole bf16x3 res,nobias
bf38_bf16x3_3x3up_split bf16x3 1 32 64 32 768 3x3up k_conv_bf3 8 none split bf16x3 -
bf38_bf16x3_3x3s2_dense bf16x3 2 128 128 16 768 3x3s2 k_conv_bf3 8 dense whole bf16x3 res,silu
bf38_bf16x3_3x3s2_dense_split bf16x3 2 128 128 32 768 3x3s2 k_conv_bf3 8 dense split bf16x3 nobias
bf38_bf16x3_3x3s2 bf16x3 2 128 128 16 768 3x3s2 k_conv_bf3 8 none whole bf16x3 res
bf38_bf16x3_3x3s2_split bf16x3 2 128 128 32 768 3x3s2 k_conv_bf3 8 none split bf16x3 -
wino_3x3_dense fp32 1 64 96 16 768 3x3 k_conv_wino - dense whole fp32 res,nobias,silu
wino_3x3_dense_split fp32 1 16 16 768 768 3x3 k_conv_wino - dense split fp32 stats:finish
wino_3x3 fp32 1 64 96 16 768 3x3 k_conv_wino - none whole fp32 res,stats:epilogue
wino_3x3_split fp32 1 16 16 768 768 3x3 k_conv_wino - none split fp32 nobias
wino_3x3up fp32 1 64 96 16 192 3x3up k_conv_wino - none whole fp32 res
wino_3x3up_split fp32 1 8 8 768 768 3x3up k_conv_wino - none split fp32 -
wino4_3x3_blocked fp32 2 64 96 16 768 3x3 k_conv_wino4 - blocked whole fp32 res,nobias,silu,stats:epilogue
wino4_3x3 fp32 2 64 96 16 768 3x3 k_conv_wino4 - none whole fp32 -
wino4_3x3up fp32 1 64 96 16 384 3x3up k_conv_wino4 - none whole fp32 res
wino4w_3x3_blocked fp32 1 64 128 16 768 3x3 k_conv_wino4w - blocked whole fp32 nobias
wino4w_3x3_blocked_split mfma 1 16 32 768 768 3x3 k_conv_wino4w - blocked split fp32 res,silu
wino4w_3x3 fp32 1 64 128 16 768 3x3 k_conv_wino4w - none whole fp32 stats:epilogue
wino4w_3x3_split mfma 1 16 32 768 768 3x3 k_conv_wino4w - none split fp32 res,nobias,stats:finish
wino4w_3x3up fp32 1 32 64 16 768 3x3up k_conv_wino4w - none whole fp32 -
wino4w_3x3up_split mfma 1 16 16 384 768 3x3up k_conv_wino4w - none split fp32 res
h16_bf16_1x1_half bf16 1 64 96 96 384 1x1 k_conv_h16 - half whole bf16 nobias
h16_bf16_1x1 bf16 1 64 96 96 384 1x1 k_conv_h16 - none whole bf16 res,stats:epilogue
h16_bf16_3x3_half bf16 1 64 96 32 384 3x3 k_conv_h16 - half whole bf16 -
h16_bf16_3x3_half_split bf16 1 16 16 768 768 3x3 k_conv_h16 - half split bf16 res,nobias
h16_bf16_3x3 bf16 1 64 96 32 384 3x3 k_conv_h16 - none whole bf16 -
h16_bf16_3x3_split bf16 1 16 16 768 768 3x3 k_conv_h16 - none split bf16 res
h16_bf16_3x3up bf16 1 32 32 32 768 3x3up k_conv_h16 - none whole bf16 nobias
h16_bf16_3x3up_split bf16 1 8 8 768 768 3x3up k_conv_h16 - none split bf16 res
h16_fp16_1x1_half fp16 1 64 96 96 384 1x1 k_conv_h16 - half whole fp16 -
h16_fp16_1x1 fp16 1 64 96 96 384 1x1 k_conv_h16 - none whole fp16 res,nobias
h16_fp16_3x3_half fp16 1 64 96 32 384 3x3 k_conv_h16 - half whole fp16 -
h16_fp16_3x3_half_split fp16 1 16 16 768 768 3x3 k_conv_h16 - half split fp16 res
h16_fp16_3x3 fp16 1 64 96 32 384 3x3 k_conv_h16 - none whole fp16 nobias,stats:epilogue
h16_fp16_3x3_split fp16 1 16 16 768 768 3x3 k_conv_h16 - none split fp16 res,stats:finish
h16_fp16_3x3up fp16 1 32 32 32 768 3x3up k_conv_h16 - none whole fp16 -
h16_fp16_3x3up_split fp16 1 8 8 768 768 3x3up k_conv_h16 - none split fp16 res,nobias
h2s_3x3_affine fp32 1 64 128 32 768 3x3 k_conv_h2s - affine whole fp16x2 -
h2s_3x3_affine_split fp32 1 16 32 192 768 3x3 k_conv_h2s - affine split fp16x2 res
h2s_3x3_affine_silu fp32 1 64 128 32 768 3x3 k_conv_h2s - affine_silu whole fp16x2 nobias,stats:epilogue
h2s_3x3_affine_silu_split fp32 1 16 32 192 768 3x3 k_conv_h2s - affine_silu split fp16x2 res
h2s_3x3 fp32 1 64 128 32 768 3x3 k_conv_h2s - none whole fp16x2 -
h2s_3x3_split fp32 1 16 32 192 768 3x3 k_conv_h2s - none split fp16x2 res,nobias,stats:finish
h2s_3x3up_split fp32 2 8 8 192 768 3x3up k_conv_h2s - none split fp16x2 -
h2s1_1x1_affine fp32 1 32 32 48 768 1x1 k_conv1_h2s - affine whole fp16x2 res
h2s1_1x1_affine_split fp32 1 32 32 384 768 1x1 k_conv1_h2s - affine split fp16x2 nobias
h2s1_1x1_affine_silu fp32 1 32 32 48 768 1x1 k_conv1_h2s - affine_silu whole fp16x2 res
h2s1_1x1_affine_silu_split fp32 1 32 32 384 768 1x1 k_conv1_h2s - affine_silu split fp16x2 -
h2s1_1x1 fp32 1 32 32 48 768 1x1 k_conv1_h2s - none whole fp16x2 res,nobias,stats:epilogue
h2s1_1x1_split fp32 1 32 32 384 768 1x1 k_conv1_h2s - none split fp16x2 stats:finish
h2d_3x3s2 fp32 1 64 128 32 768 3x3s2 k_conv_h2d - none whole fp16x2 res,stats:epilogue
h2sph_3x3up fp32 1 32 64 32 768 3x3up k_conv_h2s_ph - none whole fp16x2 nobias,stats:epilogue
h2sph_3x3up_split fp32 1 16 16 192 384 3x3up k_conv_h2s_ph - none split fp16x2 res,stats:finish
edge_conv1_ragged_cout27 direct 3 12 20 16 27 3x3 k_conv 1 none whole fp32 res
edge_conv1_s2_ragged_affine direct 3 24 40 48 27 3x3s2 k_conv 1 affine split fp32 -
edge_conv1_1x1up direct 3 12 20 16 27 1x1up k_conv 1 none whole fp32 nobias
edge_conv2_ragged_cout80_silu direct 3 12 20 16 80 3x3 k_conv 2 affine_silu whole fp32 res
edge_conv2_1x1_ragged_cout80 direct 3 24 40 48 80 1x1 k_conv 2 none whole fp32 -
edge_conv2_up_ragged_cout80 direct 3 12 20 48 80 3x3up k_conv 2 none split fp32 res,nobias
edge_conv2_1x1s2 direct 3 12 20 16 80 1x1s2 k_conv 2 none whole fp32 -
edge_dma4_ragged_cout160_split direct 3 24 40 192 160 3x3 k_conv_dma 4 none split fp32 res
edge_dma4_ragged_cin16_cout352 direct 3 52 54 16 352 3x3 k_conv_dma 4 none whole fp32 -
edge_dma4_1x1_ragged_dense direct 3 52 54 48 352 1x1 k_conv_dma 4 dense whole fp32 res,nobias,silu
edge_dma4_1x1s2_ragged direct 3 104 108 16 352 1x1s2 k_conv_dma 4 none whole fp32 -
edge_dma4_1x1up_ragged direct 3 24 40 16 352 1x1up k_conv_dma 4 none whole fp32 res
edge_dma8_ragged_cin16_cout160 direct 3 104 108 16 160 3x3 k_conv_dma 8 none whole fp32 res
edge_dma8_up_ragged direct 3 52 54 16 160 3x3up k_conv_dma 8 none whole fp32 nobias
edge_bf3x3_4_ragged_cout160_split bf16x3 3 24 40 192 160 3x3 k_conv_bf3 4 none split bf16x3 res
edge_bf3x3_4_ragged_cin16_cout352 bf16x3 3 52 54 16 352 3x3 k_conv_bf3 4 none whole bf16x3 -
edge_bf3x3_8_ragged_cin16_cout160 bf16x3 3 104 108 16 160 3x3 k_conv_bf3 8 none whole bf16x3 res
edge_bf3x3_8_up_ragged bf16x3 3 52 54 16 160 3x3up k_conv_bf3 8 none whole bf16x3 nobias
edge_bf3w2_4_ragged_cout160_split bf16 3 24 40 192 160 3x3 k_conv_bf3 4 none split bf16w2 res
edge_bf3w2_8_ragged_cin16_cout160 bf16 3 104 108 16 160 3x3 k_conv_bf3 8 none whole bf16w2 res
edge_wino_smallest_image f23 2 8 16 768 768 3x3 k_conv_wino - none split fp32 res,nobias
edge_h2s_smallest_image_res fp32 2 16 16 192 768 3x3 k_conv_h2s - none split fp16x2 res,nobias
edge_h2s1_smallest_image_res fp32 3 16 16 48 768 1x1 k_conv1_h2s - none whole fp16x2 res,nobias
edge_h2d_nonsquare_res fp32 1 128 64 32 768 3x3s2 k_conv_h2d - none whole fp16x2 res,nobias
edge_h2sph_nonsquare_res fp32 1 64 32 32 768 3x3up k_conv_h2s_ph - none whole fp16x2 res,nobias
"""


def _parse(table):
    cases = {}
    for line in table.strip().splitlines():
        name, mode, N, H, W, Cin, Cout, kind, kernel, tile, gn, split, arith, flags = line.split()
        ks, stride, ups = KINDS[kind]
        fl = set() if flags == "-" else set(flags.split(","))
        stats = [f[6:] for f in fl if f.startswith("stats:")]
        assert name not in cases and mode in MODES and split in ("whole", "split") and fl <= {"res", "nobias", "silu"} | {"stats:" + s for s in STATS_BY.values()}, line
        cases[name] = Case(mode, int(N), int(H), int(W), int(Cin), int(Cout), ks, stride, ups, kernel, None if tile == "-" else int(tile), gn, split == "split", arith,
                           int(gn == "affine_silu" or "silu" in fl), "res" in fl, "nobias" not in fl, stats[0] if stats else None)
    return cases


ALL_CASES = _parse(_TABLE)

def key(c):
    return (c.kernel, c.tile, c.ks, c.stride, c.ups, c.gn, c.split, c.arith)


def mode_number(mode):
    from humanliff_amd import _lib
    return {"fp32": _lib.HL_CONV_FP32, "bf16x3": _lib.HL_CONV_BF16X3, "direct": _lib.HL_CONV_FP32_DIRECT, "f23": _lib.HL_CONV_FP32_F23,
            "bf16": _lib.HL_CONV_BF16, "fp16": _lib.HL_CONV_FP16, "mfma": _lib.HL_CONV_FP32_MFMA}[mode]


def plan_key(mode, ks, stride, ups, with_gn, silu, plan):
    """The key of what hl_conv2d_plan_ex answered (plan: its ints as a dict over PLAN_FIELDS) for a call under `mode`."""
    k = KERNELS[plan["kernel"]]
    tile = plan["cfg"] if k == "k_conv" else (8 if plan["tile8"] else 4) if k in ("k_conv_dma", "k_conv_bf3") else None
    gn = "none" if not with_gn else (PRE[plan["pre"]] or ("affine_silu" if silu else "affine"))
    if with_gn and PRE[plan["pre"]] is None:
        assert plan["gn_mode"] == (2 if silu else 1), plan
    arith = ("fp16x2" if k in FP16X2 else ("bf16x3" if mode == "bf16x3" else "bf16w2") if k == "k_conv_bf3" else
             ("fp16" if mode == "fp16" else "bf16") if k == "k_conv_h16" else "fp32")
    return (k, tile, ks, stride, ups, gn, plan["splits"] > 1, arith)


def with_gn(c):
    return c.gn != "none"


def plan_ex(mode, N, H, W, Cin, Cout, ks, stride, ups, gn, silu, want_stats=0):
    """hl_conv2d_plan_ex (host arithmetic) -> its fields by name, or None where it refuses."""
    import ctypes
    from humanliff_amd import _lib
    buf = (ctypes.c_int * len(PLAN_FIELDS))(*([-1] * len(PLAN_FIELDS)))
    rc = _lib.lib().hl_conv2d_plan_ex(mode_number(mode), N, H, W, Cin, Cout, ks, stride, ups, gn, silu, want_stats, buf)
    return dict(zip(PLAN_FIELDS, buf)) if rc == 0 else None


def case_plan(c):
    return plan_ex(c.mode, c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.ups, int(with_gn(c)), c.silu, int(c.stats is not None))


def abi_args(c):
    """The arguments of hl_conv2d_scratch_bytes / hl_conv2d_plan after the mode."""
    return (c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.ups, int(with_gn(c)))


def out_hw(c):
    Hv, Wv = (2 * c.H, 2 * c.W) if c.ups else (c.H, c.W)
    p = c.ks // 2
    return (Hv + 2 * p - c.ks) // c.stride + 1, (Wv + 2 * p - c.ks) // c.stride + 1


# the grid the coverage test scans with hl_conv2d_plan_ex: sizes are the input's; every layer kind with no GroupNorm, the affine, and the affine + SiLU
# in front (none in front of an upsample: the call refuses it)
GRID = dict(N=(1, 2, 4),
            sizes=((8, 8), (16, 16), (16, 32), (24, 48), (32, 32), (32, 64), (64, 64), (64, 96), (64, 128), (96, 96), (128, 128)),
            cin=(16, 32, 48, 64, 96, 192, 384, 768), cout=(27, 32, 64, 96, 192, 384, 768), kinds=("3x3", "3x3s2", "3x3up", "1x1"),
            gn=((0, 0), (1, 0), (1, 1)), modes=MODES)


def _keys(kernel, tiles, kinds, gns, ariths, splits=(False, True)):
    return {(kernel, t) + KINDS[kd] + (g, sp, ar) for t, kd, g, sp, ar in itertools.product(tiles, kinds, gns, splits, ariths) if not (KINDS[kd][2] and g != "none")}


_ALL, _S1 = ("3x3", "3x3s2", "3x3up", "1x1"), ("3x3", "3x3up")
# every instantiation launch_conv / gn_prepass can be asked for on the four layer kinds of GRID
UNIVERSE = (_keys("k_conv", (0, 1, 2), _ALL, ("none", "affine", "affine_silu"), ("fp32",)) |
            _keys("k_conv_dma", (4, 8), _ALL, ("none", "dense"), ("fp32",)) |
            _keys("k_conv_bf3", (4, 8), _ALL, ("none", "dense"), ("bf16x3", "bf16w2")) |
            _keys("k_conv_wino", (None,), _S1, ("none", "dense"), ("fp32",)) |
            _keys("k_conv_wino4", (None,), _S1, ("none", "dense", "blocked"), ("fp32",)) |
            _keys("k_conv_wino4w", (None,), _S1, ("none", "dense", "blocked"), ("fp32",)) |
            _keys("k_conv_h16", (None,), _S1 + ("1x1",), ("none", "half"), ("fp16", "bf16")) |
            _keys("k_conv_h2s", (None,), _S1, ("none", "affine", "affine_silu", "twoplane"), ("fp16x2",)) |
            _keys("k_conv1_h2s", (None,), ("1x1",), ("none", "affine", "affine_silu", "dense"), ("fp16x2",)) |
            _keys("k_conv_h2d", (None,), ("3x3s2",), ("none",), ("fp16x2",)) |
            _keys("k_conv_h2s_ph", (None,), ("3x3up",), ("none",), ("fp16x2",)))

# keys of UNIVERSE that GRID cannot reach under any mode, each with the line of plan_conv that keeps it out
UNREACHABLE = {}
for _why, _ks in (
        ("`dma = pl.cfg == 0 && (!gn_on || a.act_ws) && in_31 && weights below 2 GiB`: a single-op call always brings the GroupNorm room, so a layer on the main "
         "128x96 tile goes to k_conv_dma (or a Winograd / 16-bit kernel); k_conv keeps cfg 0 only past 2^31 bytes of input or weights",
         _keys("k_conv", (0,), _ALL, ("none", "affine", "affine_silu"), ("fp32",))),
        ("`fuse1 = a.in.C <= 4096`: k_conv1_h2s applies the GroupNorm while staging up to 4096 input channels, the grid ends at 768",
         _keys("k_conv1_h2s", (None,), ("1x1",), ("dense",), ("fp16x2",))),
        ("`fuse = !a.ups && a.in.C <= 4096`: k_conv_h2s applies the GroupNorm while staging up to 4096 input channels, the grid ends at 768",
         _keys("k_conv_h2s", (None,), ("3x3",), ("twoplane",), ("fp16x2",))),
        ("`pl.tile8 = dma && blocks8 >= dma_thr` with `blocks <= target / 2` for a split leaves blocks8 == 256 and `nk >= 16` Cin >= 256: on the grid that is 8192 pixels, "
         "Cin 384 / 768, Cout 768, which k_conv1_h16 takes first under HL_CONV_BF16 (`fills`)",
         _keys("k_conv_bf3", (8,), ("1x1",), ("none", "dense"), ("bf16w2",), (True,))),
        ("`want = a.ks == 3 && ... : 0`: k_conv1_h16 never splits K", _keys("k_conv_h16", (None,), ("1x1",), ("none", "half"), ("fp16", "bf16"), (True,))),
        ("`take(ConvPath::Fp16x2, ConvKernel::H2d, {1, direct_sk.kt_per})`: k_conv_h2d is one launch over the whole K",
         _keys("k_conv_h2d", (None,), ("3x3s2",), ("none",), ("fp16x2",), (True,))),
        ("`phases = ... conv3_h2s_ph_applies(...)`: an upsample layer with 32-pixel output rows goes to k_conv_h2s_ph; on the grid only the 8x8 source has none, and its "
         "at most 16 blocks stay below `h3_min_blocks`, so it always splits",
         _keys("k_conv_h2s", (None,), ("3x3up",), ("none",), ("fp16x2",), (False,))),
        ("`else if (wino4_blocks >= wino4_thr) take(ConvPath::Wino4, ConvKernel::Wino4, w4w_sk)` is reached only when `w4w_sk.splits > 1` is false: a split goes to "
         "k_conv_wino4w", _keys("k_conv_wino4", (None,), _S1, ("none", "dense", "blocked"), ("fp32",), (True,))),
        ("`blk = a.in.pixels() % 64 == 0 && (a.coefA || ...)`: whole 16x32 output tiles of a stride-1 layer make the pixels a multiple of 512, and a single-op call "
         "gives the coefficients as arrays, so the pre-pass is always the blocked one",
         _keys("k_conv_wino4", (None,), ("3x3",), ("dense",), ("fp32",), (False,)) | _keys("k_conv_wino4w", (None,), ("3x3",), ("dense",), ("fp32",)))):
    for _k in _ks:
        UNREACHABLE.setdefault(_k, _why)


def _shape_key(c):
    return (c.N, c.H, c.W, c.Cin, c.Cout, c.ks)


@functools.lru_cache(maxsize=None)
def _operands(key_):
    N, H, W, Cin, Cout, ks = key_
    g = _gen("conv_fwd", key_)
    x = torch.randn((N, Cin, H, W), generator=g) * 1.5
    w = torch.randn((Cout, Cin, ks, ks), generator=g) / (ks * ks * Cin) ** 0.5
    w = w * torch.exp2(torch.randint(-6, 1, (Cout, 1, 1, 1), generator=g).float())
    b = torch.randn(Cout, generator=g) * 0.1
    A, B = torch.rand((N, Cin), generator=g) + 0.5, torch.randn((N, Cin), generator=g) * 0.1
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    return dict(x=x, w=w, b=b, A=A, B=B, gamma=gamma, beta=beta)


@functools.lru_cache(maxsize=None)
def _residual(shape):
    return torch.randn(shape, generator=_gen("conv_fwd_res", shape))


def operands(c):
    """x (N,Cin,H,W), w (Cout,Cin,ks,ks), b (Cout) or None, A / B (N,Cin) or None, res (N,Cout,Ho,Wo) or None, and gamma / beta (Cout): the next
    layer's GroupNorm, for the cases that return statistics."""
    o = dict(_operands(_shape_key(c)))
    if not c.bias:
        o["b"] = None
    if not with_gn(c):
        o["A"] = o["B"] = None
    o["res"] = _residual((c.N, c.Cout) + out_hw(c)) if c.res else None
    return o


def _round_to(dt):
    return lambda t: t.to(dt).to(t.dtype)


def _rounding(kernel, arith):
    """What the kernel does to (activations, weights) before it multiplies: None, or a pair of functions that keep the dtype."""
    if kernel == "k_conv_h16":
        r = _round_to(torch.float16 if arith == "fp16" else torch.bfloat16)
        return r, r
    if arith == "bf16w2":
        return _round_to(torch.bfloat16), lambda w: bf16_planes2(w.float()).to(w.dtype)      # (w holds fp32 values: the planes are cut from those)
    return None


def rounding(c):
    return _rounding(c.kernel, c.arith)


def _forward(x, w, b, A, B, res, c, rnd):
    """The case's steps in the dtype of x."""
    if A is not None:
        x = x * A[:, :, None, None] + B[:, :, None, None]
        if c.silu:
            x = x * torch.sigmoid(x)
    if rnd is not None:
        x, w = rnd[0](x), rnd[1](w)
    if c.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w, b, stride=c.stride, padding=c.ks // 2)
    return y if res is None else y + res


@functools.lru_cache(maxsize=None)
def _reference(geom, rounded):
    o = operands(geom)
    rnd = _rounding(geom.kernel, geom.arith) if rounded else None
    d = lambda t: None if t is None else t.double()  # noqa: E731
    want = _forward(d(o["x"]), d(o["w"]), d(o["b"]), d(o["A"]), d(o["B"]), d(o["res"]), geom, rnd)
    ref32 = _forward(o["x"], o["w"], o["b"], o["A"], o["B"], o["res"], geom, rnd)
    return dict(want=want, ref32=ref32, scale=float(want.abs().max()), e_ref=float((ref32.double() - want).abs().max()))


def reference(c):
    """want: float64 y (N, Cout, Ho, Wo) of the operands as the case's kernel rounds them; ref32: the same steps in fp32 on the CPU; e_ref =
    max|ref32 - want|; scale = max|want|; exact: float64 y of the unrounded operands (= want unless the kernel rounds to 16 bits)."""
    rounded = rounding(c) is not None
    geom = c._replace(mode="", tile=None, split=False, stats=None, kernel=c.kernel if rounded else "", arith=c.arith if rounded else "")   # what _forward reads
    r = dict(_reference(geom, rounded))
    r["exact"] = _reference(geom._replace(kernel="", arith=""), False)["want"] if rounded else r["want"]
    return r


def is_fair(c):
    r = reference(c)
    return r["e_ref"] <= E_REF_MAX * r["scale"]


def flips(c):
    """The case rounds a GroupNorm output to 16 bits: the only cases that may be DROPPED."""
    return rounding(c) is not None and with_gn(c)


# Cases whose fp32 CPU restatement misses the fairness condition E_ref <= E_REF_MAX max|y| (tests/test_conv_fwd_cpu.py asserts that each one
# still does, and that nothing else is here): a 16-bit rounding of the GroupNorm output that falls the other way in fp32 than in float64 moves an
# activation by half a unit of the 16-bit type, far above fp32 summation noise, and a new seed only moves the flips (about one activation in
# 2^13 for fp16, 2^16 for bf16, of 10^5 ... 10^6).  They stay pinned to their instantiation and counted by the coverage test, and are not run on
# the GPU by this table.  The three cases of this kind that are fair (bf34_bf16w2_3x3s2_dense_split, bf38_bf16w2_1x1_dense, h16_bf16_3x3_half)
# are: every case of the kind runs its pre-pass WITHOUT SiLU, where the pre-pass kernels (k_gn_apply, k_gn_apply_h16: `v * a + b`, built without
# contraction) and ref32 make the same two IEEE roundings, so a case without flips on the CPU has none on the GPU; a SiLU differs in its last bits.
DROPPED = ("bf34_bf16w2_1x1_dense", "bf34_bf16w2_1x1_dense_split", "bf34_bf16w2_3x3_dense", "bf34_bf16w2_3x3_dense_split", "bf34_bf16w2_3x3s2_dense",
           "bf38_bf16w2_3x3_dense", "bf38_bf16w2_3x3_dense_split", "bf38_bf16w2_3x3s2_dense", "bf38_bf16w2_3x3s2_dense_split",
           "h16_bf16_1x1_half", "h16_bf16_3x3_half_split", "h16_fp16_1x1_half", "h16_fp16_3x3_half", "h16_fp16_3x3_half_split")
# the cases the GPU test runs
CASES = {n: c for n, c in ALL_CASES.items() if n not in DROPPED}
