"""Every staging-mode instantiation of the fp16x2 stride-1 kernels (k_conv_h2s: raw, affine, affine + SiLU, two-plane image; k_conv_h2s_ph: raw;
k_conv1_h2s: raw, affine, affine + SiLU) through hl_conv2d_nhwc_mode, at the smallest shapes that still turn the chunk loop over and touch every
image border:
    3x3, whole K     1 x 64x128, 96 -> 768: three chunks (both patch stages, the weight ring wraps), 768 output channels so that the plan keeps K whole
    3x3, split K     1 x 16x32, 192 -> 768, with a residual
    upsample phases  1 x 32x64 SOURCE (64x128 output), 96 -> 768: at a 32x64 output the plan takes k_conv_wino for this layer, and the 16x32
                     source reaches the phase kernel only from N = 4 on - the same pixel count as the other whole-K cases
    1x1              1 x 64x128, 96 -> 192
    two-plane        1 x 16x32, 4128 -> 768: the smallest Cin above 4096 (a multiple of the 32-channel chunk) - the plan materialises the GroupNorm
                     output as two fp16 planes and k_conv_h2s stages them as they are
The GroupNorm comes as coefficient arrays: the single-operation call has no other form.  Producer totals (ConvK::gn) exist only inside
hl_unet_forward, whose tests and the benchmark's dumped outputs run that prologue; arrays and totals differ in the prologue alone, not in the chunk
loop the instantiations differ in.

Each case is pinned to its kernel and mode with hl_conv2d_plan_ex (the plan's kernel, split, GroupNorm mode and pre-pass are what the launcher picks
the instantiation from) and then handed, under its own name, to tests/test_conv_fwd_gpu.py's test body: float64 reference on the CPU, the standing
bound of the fp16x2 kernels against the direct kernel's error on the same tensors, the call repeated on the same inputs with bit-equal results,
sentinels around the output, and the 2^-10 scale that must pass through bit for bit."""
import pytest

from tests import conv_fwd_cases as cf
from tests import test_conv_fwd_gpu as fwd

pytestmark = pytest.mark.gpu

# name  mode  N H W Cin Cout  kind  kernel  tile  GroupNorm  split-K  arithmetic  flags      (the columns of conv_fwd_cases._TABLE)
_TABLE = """
modes_h2s_whole_raw fp32 1 64 128 96 768 3x3 k_conv_h2s - none whole fp16x2 -
modes_h2s_whole_affine fp32 1 64 128 96 768 3x3 k_conv_h2s - affine whole fp16x2 -
modes_h2s_whole_affine_silu fp32 1 64 128 96 768 3x3 k_conv_h2s - affine_silu whole fp16x2 -
modes_h2s_split_raw fp32 1 16 32 192 768 3x3 k_conv_h2s - none split fp16x2 res
modes_h2s_split_affine fp32 1 16 32 192 768 3x3 k_conv_h2s - affine split fp16x2 res
modes_h2s_split_affine_silu fp32 1 16 32 192 768 3x3 k_conv_h2s - affine_silu split fp16x2 res
modes_h2s_twoplane fp32 1 16 32 4128 768 3x3 k_conv_h2s - twoplane split fp16x2 silu
modes_h2sph_whole_raw fp32 1 32 64 96 768 3x3up k_conv_h2s_ph - none whole fp16x2 -
modes_h2s1_raw fp32 1 64 128 96 192 1x1 k_conv1_h2s - none whole fp16x2 -
modes_h2s1_affine fp32 1 64 128 96 192 1x1 k_conv1_h2s - affine whole fp16x2 -
modes_h2s1_affine_silu fp32 1 64 128 96 192 1x1 k_conv1_h2s - affine_silu whole fp16x2 -
"""
CASES = cf._parse(_TABLE)


def test_two_plane_case_is_the_smallest_the_plan_accepts():
    """4128 = 4096 + one chunk: below it (any multiple of 32 up to 4096) the kernel applies the GroupNorm itself."""
    c = CASES["modes_h2s_twoplane"]
    assert c.Cin == 4096 + 32
    below = cf.case_plan(c._replace(Cin=4096))
    assert cf.KERNELS[below["kernel"]] == "k_conv_h2s" and cf.PRE[below["pre"]] is None and below["gn_mode"] == 2, below


@pytest.mark.parametrize("name", sorted(CASES))
def test_mode_instantiation_matches_float64(name, monkeypatch):
    c = CASES[name]
    plan = cf.case_plan(c)
    assert plan is not None, "the plan refuses the case"
    assert cf.plan_key(c.mode, c.ks, c.stride, c.ups, int(cf.with_gn(c)), c.silu, plan) == cf.key(c), (name, plan)
    assert name not in cf.CASES
    monkeypatch.setitem(cf.CASES, name, c)
    fwd.test_forward_matches_float64_on_its_kernel(name)
