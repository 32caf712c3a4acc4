// Launchers of the UNet / sampler device kernels (hl_unet_kernels.hip). Internal header.
// The packed weight forms of a convolution are one table: WeightForm names them in buffer order, conv_form_bytes / conv_pack_form size and
// pack one, ConvWeights holds the pointers, conv_forms says which of them an HL_CONV_* mode may use and form_of which one a ConvPath reads.
#pragma once
#include "hl_common.h"

namespace hl {

// NHWC fp32 tensor view with a channel pitch (so two producers can write into one "concat" buffer).
struct View {
    float *p = nullptr;
    int N = 0, H = 0, W = 0, C = 0;
    long pitch = 0;  // floats between consecutive pixels
    long pixels() const { return (long)N * H * W; }
};

// Where a kernel that normalises its input gets the per-(image, channel) affine y = x*A + B of GroupNorm32 [+ scale/shift] from: the
// arrays cA / cB (groupnorm_coef / groupnorm_coef_stats wrote them), or - gt set - the fixed-point group totals its producer(s) left
// (ConvArgs::stats) plus the norm's own parameters: every consumer workgroup then forms the coefficients of its image itself
// (coef_to_lds, hl_stats.h) and no coefficient launch sits between producer and consumer.  C = channels of the normalised view, HW =
// pixels per image (it also fixes the number of shards of the totals).
struct GnSrc {
    const float *gt;
    int C, HW;
    const float *gamma, *beta, *emb;   // emb (N, emb_pitch) holds [scale(C) | shift(C)] or null
    long emb_pitch;
    float eps;
};

// The kernel family a convolution runs on.  The values reach Python (hl_unet_dispatch_census, hl_unet_profile_dominant) and keep their numbers.
enum class ConvPath : int {
    Direct = 0,   // implicit GEMM on the fp32 matrix pipe: k_conv, k_conv_dma
    Wino2 = 1,    // Winograd F(2x2,3x3): k_conv_wino
    Bf16x3 = 2,   // fp32 emulated on the bf16 matrix pipe (or HL_CONV_BF16): k_conv_bf3
    Wino4 = 3,    // Winograd F(4x4,3x3): k_conv_wino4, k_conv_wino4w
    H16 = 5,      // 16-bit operands: k_conv_h16
    Fp16x2 = 6,   // fp16x2 products: k_conv1_h2s, k_conv_h2s, k_conv_h2d
};
// row of hl_unet_dispatch_census: 0 direct, 1 F(2x2), 2 the 16-bit matrix pipe (bf16x3 and k_conv_h16), 3 F(4x4), 4 fp16x2
constexpr int conv_census_row(ConvPath p) {
    return p == ConvPath::Fp16x2 ? 4 : (p == ConvPath::H16 ? 2 : (int)p);
}
// FLOPs a family issues per algorithmic FLOP: Winograd F(2x2,3x3) 16 multiplies per 2x2 outputs instead of 36, F(4x4,3x3) a quarter,
// bf16x3 six bf16 MFMA products per fp32 product
constexpr double conv_issued_factor(ConvPath p) {
    return p == ConvPath::Wino2 ? 16.0 / 36.0 : (p == ConvPath::Wino4 ? 0.25 : (p == ConvPath::Bf16x3 ? 6.0 : 1.0));
}

// The packed forms of one convolution's weights, in the order they lie in the network's packed buffer.
enum class WeightForm : int {
    Fp32,     // [Cout_pad][Ktot] floats, K order = kt_decode() in hl_unet_kernels.hip (groups of two 16-channel chunks, taps inside): k_conv, k_conv_dma; every layer has it
    Bf16x3,   // three bf16 planes, [Cout_pad][K/16][plane*2 + k-half][8 bf16], 6 bytes per weight (layers that take the DMA tile: Cout_pad a multiple of 96): k_conv_bf3
    Wino2,    // Winograd F(2x2,3x3) U = G g G^T, [Cout/64][Cin_pad/8][16][2][2][32][4] floats: k_conv_wino
    Wino4,    // Winograd F(4x4,3x3) (points 0, +-3/4, +-3/2, inf), [Cout/32][Cin_pad/8][36][2][32][4] floats, a ragged Cout < 32 padded with zero rows: k_conv_wino4[w]
    Fp16x2,   // two fp16 planes in MFMA-fragment order + the [Cout] inverse power-of-two scales behind them (conv_h2_wscale): k_conv1_h2s, k_conv_h2s, k_conv_h2d
    H16,      // 16-bit weights (fp16, or bf16 on request) in MFMA-fragment order: k_conv_h16, k_conv1_h16
    Fp16x2Up, // the Upsample convolutions only (conv_form_bytes(.., ups = true)): nearest-x2 + 3x3 as four 2x2-tap phase convolutions, the summed taps as
              // Fp16x2 planes [phase 4][..][tap 4].. + the [4][Cout] inverse scales (conv_h2p_wscale): k_conv_h2s_ph
    kCount
};
constexpr int kWeightForms = (int)WeightForm::kCount;
constexpr unsigned form_bit(WeightForm f) { return 1u << (int)f; }
// the form the kernels of a family read
constexpr WeightForm form_of(ConvPath p) {
    return p == ConvPath::Wino2 ? WeightForm::Wino2 : p == ConvPath::Bf16x3 ? WeightForm::Bf16x3 : p == ConvPath::Wino4 ? WeightForm::Wino4 :
           p == ConvPath::H16 ? WeightForm::H16 : p == ConvPath::Fp16x2 ? WeightForm::Fp16x2 : WeightForm::Fp32;
}
// Bytes of one form; 0: the layer has no such form.  cap_wino4: F(4x4,3x3) weights are 4x the direct ones - the network keeps them only up to 64 MB a
// layer (the single-op entry points, which pack one form per call, pass false).  ups: the layer reads its input through the nearest-x2 upsample
// (only such a layer has WeightForm::Fp16x2Up).
size_t conv_form_bytes(WeightForm f, int Cout, int Cin_pad, int ks, bool cap_wino4 = true, bool ups = false);
// packs w (Cout, Cin, ks, ks) into dst (conv_form_bytes of room).  tf = 1: the source is laid out (Cin, Cout, ks, ks) and is read flipped and
// channel-transposed (backward-data weights).  f16 (WeightForm::H16 only): 1 fp16, 0 bf16.
int conv_pack_form(WeightForm f, const float *w, int Cout, int Cin, int Cin_pad, int ks, void *dst, hipStream_t st, int tf = 0, int f16 = 1);
const float *conv_h2_wscale(const void *packed, int Cout, int Cin_pad, int ks);   // the [Cout] inverse scales behind the Fp16x2 planes (ConvK::wsc)
const float *conv_h2p_wscale(const void *packed, int Cout, int Cin_pad);          // the [4 phases][Cout] inverse scales behind the Fp16x2Up planes

struct ConvWeights {
    const void *p[kWeightForms] = {};
    bool has(WeightForm f) const { return p[(int)f] != nullptr; }
    const float *fp32() const { return static_cast<const float *>(p[(int)WeightForm::Fp32]); }
    ConvWeights only(unsigned mask) const {   // the forms of `mask` (bits form_bit)
        ConvWeights r;
        for (int f = 0; f < kWeightForms; ++f) if (mask >> f & 1u) r.p[f] = p[f];
        return r;
    }
};

constexpr bool conv_mode_known(int mode) {
    return mode == HL_CONV_FP32 || mode == HL_CONV_FP32_MFMA || mode == HL_CONV_BF16X3 || mode == HL_CONV_FP32_DIRECT || mode == HL_CONV_FP32_F23 ||
           mode == HL_CONV_BF16 || mode == HL_CONV_FP16;
}
constexpr bool conv_mode_bf16(int mode) { return mode == HL_CONV_BF16X3 || mode == HL_CONV_BF16; }   // the modes of k_conv_bf3
// The forms (bits form_bit) a convolution may use under the HL_CONV_* `mode`.  bf16_h16: the caller can pack the 16-bit form in bf16 - the network
// packs it in fp16 only, so its HL_CONV_BF16 never reaches k_conv_h16.  bwd_data: a backward-data call (tf = 1), which never takes the fp16x2 form
// (measured with the scale-invariant planes - the training step at microbatch 2 went from 102.6 to 110.1 ms as a HIP graph: per call the gradient's
// abs-max pass, the weights' scale + pack, and kernels that at two rounds of workgroups are no faster than F(4x4,3x3) on the fp32 pipe).
constexpr unsigned conv_forms(int mode, bool bf16_h16, bool bwd_data) {
    const bool f32 = mode == HL_CONV_FP32 || mode == HL_CONV_FP32_MFMA || mode == HL_CONV_FP16;   // (HL_CONV_FP16: the other layers as HL_CONV_FP32)
    return form_bit(WeightForm::Fp32) | (conv_mode_bf16(mode) ? form_bit(WeightForm::Bf16x3) : 0u) |
           (f32 || mode == HL_CONV_FP32_F23 ? form_bit(WeightForm::Wino2) : 0u) | (f32 ? form_bit(WeightForm::Wino4) : 0u) |
           (mode == HL_CONV_FP32 && !bwd_data ? form_bit(WeightForm::Fp16x2) | form_bit(WeightForm::Fp16x2Up) : 0u) |
           (mode == HL_CONV_FP16 || (bf16_h16 && mode == HL_CONV_BF16) ? form_bit(WeightForm::H16) : 0u);
}

struct ConvArgs {
    View in;             // C must be a multiple of 16 (pad channels are zero and have zero weights)
    ConvWeights w;       // the forms plan_conv may choose from (Fp32 always; the others masked by conv_forms(mode, ...))
    int mode;            // HL_CONV_*: says which kernel reads a form two modes share - HL_CONV_BF16 (activations rounded to bf16 x the weights' two leading bf16 planes)
                         // against the bf16x3 emulation on Bf16x3; fp16 (HL_CONV_FP16) against bf16 operands on H16
    const float *in_absmax; // optional, instead of in_stats: [N] the largest |x| of every image of `in` (tensor_absmax)
    const float *in_stats; // optional: the group totals the producer(s) of `in` left for ANY view that covers it (conv_stats_floats(N, in.H * in.W) floats, complete
                         // when this launch starts): the fp16x2 kernels derive the power-of-two scale of the raw input from sum x^2 (ConvK::xs_gt); null: scale 1
    const float *bias;   // [Cout] or null
    int Cout;            // real output channels
    int ks;              // 1 or 3 (pad = ks/2)
    int stride;          // 1 or 2
    int ups;             // 1: input is read through a nearest x2 upsample (unet.py:77)
    const float *coefA;  // per-(n, cin) affine applied before the conv (GroupNorm [+scale/shift]) or null
    const float *coefB;
    GnSrc gn;            // alternative to coefA / coefB (gn.t0 != null): the affine formed in the kernels from the producers' totals
    int act;             // 1: SiLU after the affine
    View out;            // NHWC (pitch honoured) unless out_nchw
    const float *res;    // residual added to out (may alias out.p), pitch res_pitch; or null
    long res_pitch;
    float *out2;         // optional second output out2 = out + res2
    long out2_pitch;
    const float *res2;
    long res2_pitch;
    int out_nchw;        // write (N, Cout, H, W) instead of NHWC
    float *act_ws;       // optional scratch (pixels*Cin floats) for the materialised GroupNorm(+SiLU) input of k_conv_dma
    size_t act_ws_bytes;
    float *splitk_ws;    // optional scratch for split-K partial sums (small-M layers); null disables split-K
    size_t splitk_ws_bytes;
    // GroupNorm statistics of the OUTPUT for the layer that will normalise it, emitted by the epilogue of whichever kernel stores
    // the tensor: per image and GROUP of the normalised view the totals (sum x, sum x^2), as 64-bit FIXED-POINT integers [shard][N][32][2]
    // that the workgroups add to with integer atomics (hl_stats.h) - integer addition is associative, so the totals are bit-identical
    // from run to run.  `stats` (and `stats2` for out2) need conv_stats_floats(N, pixels per image) floats each, ZEROED before the first
    // producer of the view runs; null = not wanted.  st_cg = channels per group of the view (0: Cout / 32), st_c0 = channel of the view
    // that output channel 0 is (a decoder "concat" has two producers adding into one block).  ConvPlan::stat_slots says whether the
    // launch adds its totals (> 0) or this path emits none (register-staged / bf16x3 / NCHW / odd sizes): the consumer then computes the
    // statistics from the tensor (groupnorm_coef).
    float *stats, *stats2;
    int st_cg, st_c0, st2_cg, st2_c0;
    hipEvent_t ev_mid;   // optional (profiling): recorded between the GroupNorm pre-pass and the convolution kernel, when there is a pre-pass
};
// kernel-side argument block of the convolution kernels (filled by conv2d)
struct ConvK {
    const float *in; long in_pitch; int N, Hin, Win, Cin;
    int Hout, Wout, ks, stride, ups, taps;
    const float *w;    // WeightForm::Fp32 (the direct kernels)
    const void *wf;    // the form the planned kernel reads, ConvPlan::form: what every other kernel reads
    long Ktot; const float *bias; int Cout;
    const float *cA; const float *cB; int act;
    GnSrc gn;          // (cA null and gn.t0 set: the coefficients are formed in the kernel, coef_to_lds)
    float *out; long out_pitch; const float *res; long res_pitch;
    float *out2; long out2_pitch; const float *res2; long res2_pitch;
    int out_nchw; long M; int wrows;
    int kt_per;        // k-tiles per split (blockIdx.z); gridDim.z == 1 -> whole K
    int n_mtiles, n_nblocks;
    float *partial;    // split-K: raw accumulators [z][M][Cout]
    // GroupNorm statistics of the OUTPUT, emitted by the epilogue for the layer that will normalise it (nn.py:17-19): fixed-point totals
    // (sum, sum of squares) of the stored value (after bias / residual) per image and group of the normalised view, [shard][N][32][2]
    // 64-bit integers the epilogues add to atomically (hl_stats.h); null = not wanted.  st2: the same for out2.  cg / c0: channels per
    // group of the view, the view channel of output channel 0.  Deterministic (integer adds commute).
    int st1_cg, st1_c0, st2_cg, st2_c0;
    float *st1, *st2;
    int in16;          // k_conv_h16 / k_conv1_h16: `in` holds 16-bit values (the GroupNorm pass wrote them), in_pitch counts them
    // fp16x2 kernels (round 6: the split products are scale-invariant).  wsc: [Cout] inverse power-of-two scales of the weight planes (conv_h2_wscale) - the
    // epilogue multiplies the accumulators by them.  xs_gt: group totals of the raw INPUT tensor (the block its producer(s) left, ConvArgs::in_stats) or null:
    // the staging multiplies the input by the power of two sx with |x| sx <= sqrt(sum x^2) sx <= 32752 (no overflow of the fp16 planes, and the low plane stays
    // normal for values down to 2^-11 of the image's largest possible), the epilogue by 1 / sx; a fused GroupNorm takes its sx from the coefficient bound instead.
    const float *wsc;
    const float *xs_gt;
    int xs_hw;         // pixels per image of the tensor the totals belong to (fixes the number of shards)
    const float *xs_max;   // alternative to xs_gt: [N] the largest |x| of every image (tensor_absmax) - exact at any magnitude (the single-op entry points: gradients are 1e-4 ... 1e-9)
};

// k_conv_wino4w (hl_conv_wino4w.hip): Winograd F(4x4,3x3) with 64 output channels per workgroup, one wave per SIMD, 18 accumulator
// tiles per wave in the accumulator registers; reads ConvK::wf = WeightForm::Wino4.  LDS: conv_wino4w_lds_bytes().
size_t conv_wino4w_lds_bytes();
int conv_wino4w_launch(const ConvK &p, int ups, int blk, int splits, hipStream_t st);

// k_conv_h16 (hl_conv_h16.hip): 3x3 / stride-1 convolution with 16-bit operands (fp16 / bf16) and fp32 accumulation, 16x16 pixels x 192
// channels per workgroup; reads ConvK::wf = WeightForm::H16 (ConvK::n_mtiles = N (H/16)(W/16), n_nblocks = Cout/192).
bool conv_h16_applies(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int ups);
int conv_h16_launch(const ConvK &p, int f16, hipStream_t st, int splits = 1);
// k_conv1_h2s (hl_conv_h16.hip): the 1x1 / stride-1 convolutions of the default fp32 mode with fp16x2 products (two fp16 planes per operand, three partial
// products, fp32 accumulation) on 128-pixel tiles, two workgroups per CU; reads ConvK::wf = WeightForm::Fp16x2, ConvK::n_mtiles = pixels / 128,
// n_nblocks = Cout / 192.
bool conv1_h2_applies(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int ups);
int conv1_h2s_launch(const ConvK &p, hipStream_t st, int splits = 1);
bool conv3_h2d_applies(int Hout, int Wout, int Cin, int Cout);        // 3x3 / stride 2 with fp16x2 products (k_conv_h2d)
int conv3_h2d_launch(const ConvK &p, hipStream_t st);                 // p.n_mtiles = output pixels / 128
int conv3_h2s_launch(const ConvK &p, hipStream_t st, int splits = 1);  // 3x3 / stride 1 on 8x16-pixel tiles, two workgroups per CU (p.n_mtiles = pixels / 128;
                                                                       // ConvK::in16 = 2: a two-plane image from the GroupNorm pass)
// k_conv_h2s_ph: nearest-x2 + 3x3 as four 2x2-tap phase convolutions of the source (reads WeightForm::Fp16x2Up); output a multiple of 16 x 32 pixels
bool conv3_h2s_ph_applies(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int ups);
int conv3_h2s_ph_launch(const ConvK &p, hipStream_t st, int splits = 1);   // p.n_mtiles = output pixels / 128 (phase = tile & 3)
void set_h16_min_blocks(long v);   // developer / test switch: workgroups from which the dispatch takes k_conv_h16 (< 0: the default, 48)

// Statistics block of one normalised VIEW (ConvArgs::stats): [shard][N][32 groups][2] 64-bit fixed-point totals.  Levels with many
// workgroups per image keep stat_shards(HW) = 8 copies (a workgroup adds to copy blockIdx.x % 8: atomics on one word serialise), the low
// levels one.
constexpr int stat_shards(long HW) { return HW >= 4096 ? 8 : 1; }
constexpr size_t conv_stats_floats(int N, long HW) { return (size_t)stat_shards(HW) * N * 32 * 4; }
size_t conv_splitk_ws_bytes();
// totals (conv_stats_floats(x.N, x.H * x.W) floats, zeroed here) of a tensor nobody left totals for: what ConvArgs::in_stats wants (the single-op entry points)
int tensor_totals(const View &x, float *totals, hipStream_t st);
// [N] floats: the largest |x| of every image (zeroed here; non-negative floats order like their bit patterns: one integer atomicMax per workgroup)
int tensor_absmax(const View &x, float *amax, hipStream_t st);

// the kernel within the family
// (the numbers reach Python through hl_conv2d_plan and stay)
enum class ConvKernel : int { Conv = 0, Dma = 1, Bf3 = 2, Wino = 3, Wino4 = 4, Wino4w = 5, H16 = 6, H2s = 7, H2s1 = 8, H2d = 9, H2sUp = 10 };
// GroupNorm(+SiLU) materialised into ConvArgs::act_ws before the convolution, and its format: dense fp32, fp32 channel-blocked [C/8][pixel][8]
// (k_conv_wino4 / k_conv_wino4w read it), the 16-bit image (k_conv_h16) or the two-plane fp16 image (k_conv_h2s)
// (the numbers reach Python through hl_conv2d_plan_ex and stay: HL_PRE_* in humanliff_hip.h)
enum class ConvPrePass : int { None = 0, Dense = 1, Blocked = 2, Half = 3, TwoPlane = 4 };
// which kernel adds the output statistics (ConvArgs::stats): the convolution's epilogue, or the split-K finish (HL_STATS_BY_*)
enum class ConvStatsBy : int { None = 0, Epilogue = 1, Finish = 2 };

// Everything a convolution launch decides, made by plan_conv without any HIP call.
struct ConvPlan {
    ConvPath path = ConvPath::Direct;
    ConvKernel kernel = ConvKernel::Conv;
    WeightForm form = WeightForm::Fp32;   // the form the kernel reads: form_of(path), except k_conv_h2s_ph's Fp16x2Up
    int cfg = 0;             // k_conv tile config: 0 = 128x96, 1 = 128x32 (Cout <= 32), 2 = 64x64
    bool tile8 = false;      // k_conv_dma / k_conv_bf3: the 8-wave 256x96 tile (else 4 waves x 128x96)
    int gn_mode = 0;         // GroupNorm in front of the convolution: 0 none, 1 the affine, 2 the affine + SiLU
    ConvPrePass pre = ConvPrePass::None;
    int splits = 1, kt_per = 0;   // split-K slabs (k_splitk_finish[_st] sums them when > 1) and k-tiles per slab
    ConvStatsBy stats_by = ConvStatsBy::None;
    int stat_slots = 0;      // > 0: the launch adds the output statistics (ConvArgs::stats); 0: the consumer computes them from the tensor
};
ConvPlan plan_conv(const ConvArgs &a);
// runs `pl` = plan_conv(a); a caller may drop forms from a.w in between, all but the one the plan reads (conv2d_single)
int conv2d(const ConvArgs &a, const ConvPlan &pl, hipStream_t st);

// GroupNorm(32 groups, eps 1e-5) statistics -> per-(n,c) affine  y = x*A + B   (nn.py:17-19,100)
// optional scale/shift (ResBlock use_scale_shift_norm, unet.py:203-206): y = GN(x)*(1+scale)+shift,
// where emb (N, emb_pitch) holds [scale(C) | shift(C)] starting at emb + n*emb_pitch.
size_t gn_scratch_floats(int N);
// the same affine (as arrays) from the group totals the producer(s) of the view left (ConvArgs::stats)
int groupnorm_coef_stats(const View &x, const float *group_totals, const float *gamma, const float *beta, const float *emb,
                         long emb_pitch, float *coefA, float *coefB, hipStream_t st, float eps = 1e-5f);
// gstat (optional): (N, 32, 2) = (mean, rstd) of every group, for the backward pass of the training path
int groupnorm_coef(const View &x, const float *gamma, const float *beta, const float *emb, long emb_pitch, float *coefA,
                   float *coefB, float *scratch, hipStream_t st, float *gstat = nullptr, float eps = 1e-5f);

// y (dense NHWC) = act ? silu(x*A + B) : x*A + B with the per-(n,c) affine of groupnorm_coef (the pre-pass of the DMA convs; the
// GroupNorm forward of the training path)
int gn_apply(const View &x, const float *coefA, const float *coefB, int act, float *y, hipStream_t st);

// out[b][o] = bias[o] + sum_k act(in[b][k]) * W[o][k] (+ addrow[idx[b]][o]);  B <= 16; act is applied once per workgroup (inputs staged in LDS), weights streamed 16 bytes per lane
int linear_small(const float *in, long in_pitch, int B, int K, const float *W, const float *bias, int O, int silu_in,
                 const float *addrow, const int64_t *idx, float *out, long out_pitch, hipStream_t st);
// sinusoidal timestep embedding (nn.py:103-121); t is int64 (B,)
int timestep_embedding(const int64_t *t, const float *t_float, int B, int dim, float *out, hipStream_t st);

// QKV attention (unet.py:255-274): qkv (N, T, 3C) with channel = head*3ch + {q|k|v}*ch + c ; out (N, T, C)
// h2: fp16x2 products where a kernel has them (the default conv mode's attention).  out_totals: optional zeroed conv_stats_floats(N, T) floats - the key-split kernels add the
// sum x^2 of the output they store (the projection convolution's activation scale); *totals_emitted says whether the kernel that ran did
int attention(const float *qkv, int N, int T, int C, int heads, float *out, hipStream_t st, int h2 = 0, float *out_totals = nullptr, int *totals_emitted = nullptr);
int debug_set_attention_tiling(int query_tiles, int placement);                                // hl_debug_set_attention_tiling (test switch; 0 = the dispatch rule)
size_t attention_backward_scratch_bytes(int N, int T, int C, int heads);                       // hl_attention_bwd.hip
int attention_backward(const float *qkv, const float *out, const float *dout, int N, int T, int C, int heads, float *dqkv, void *scratch,
                       size_t scratch_bytes, hipStream_t st);

// (B,C,H,W) x, x_cond -> NHWC padded to Cpad: x_nhwc and (x + x_cond)_nhwc   (unet.py:588,596)
// x_tot / xsum_tot: optional zeroed conv_stats_floats(B, H * W) floats each - the outputs' sum x^2 per image (the input convolutions' activation scale)
int prep_inputs(const float *x, const float *x_cond, int B, int C, int H, int W, int Cpad, float *x_nhwc, float *xsum_nhwc,
                hipStream_t st, float *x_tot = nullptr, float *xsum_tot = nullptr);

// cond_type='cross_attention' (spatial_transformer.py): nn.LayerNorm over the channels of every pixel -> y dense (pixels, C); GEGLU on
// (pixels, 2F) -> (pixels, F); x (N, HW, C) += v (N, C)
int layernorm(const View &x, const float *gamma, const float *beta, float *y, hipStream_t st);
int geglu(const float *in, long npix, int F, float *out, hipStream_t st);
int add_rowvec(const View &x, const float *v, hipStream_t st, long vpitch = 0);   // x[n, p, c] += v[n * vpitch + c] (vpitch 0: C)
// use_3d_aware=True (unet.py:566-570, 613-614): (B, 3C, H, W) NCHW <-> the planes side by side, NHWC (B, H, 3W, Cpad) / NCHW (B, C, H, 3W)
int prep_inputs_3d(const float *x, const float *x_cond, int B, int C, int H, int W, int Cpad, float *x_nhwc, float *xsum_nhwc,
                   hipStream_t st);
int unroll_planes(const float *rolled_nchw, int B, int C, int H, int W, float *out, hipStream_t st);
// ResBlock step of unet.py:208-214: y (N, H, 3W, 3C dense) = silu(cat[A h + B, two plane means of it]); sums: N*3*(H + W/3)*C floats
int gn_apply_3d(const View &h, const float *coefA, const float *coefB, float *sums, float *y, hipStream_t st);

}  // namespace hl
