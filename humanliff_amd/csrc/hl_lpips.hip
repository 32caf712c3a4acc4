// LPIPS(net='vgg', version='0.1') forward on the device, MI355X (gfx950): the perceptual score of the reference's test mode
// (recon_NeRF/lib/all_test.py: loss_fn_vgg on the masked crops).  Contract: DESIGN.md 4f "LPIPS"; exact fp32 products throughout.
//
// k_lpips_prep: the scaling layer.  (B, 3, h, w) NCHW pairs -> one (N, h, w, 16) NHWC batch, (x - shift) / scale in channels 0..2 and
//   zeros in 3..15, so the first convolution is the same implicit GEMM as the other twelve with one (zero-padded) K chunk.
// k_lpips_conv: 3 x 3 / pad 1 convolution + bias + ReLU, NHWC fp32, any h, w.  A workgroup (4 waves) owns 8 x 16 output pixels x 64
//   output channels; wave w owns rows 2w, 2w + 1 (32 pixels = the M of v_mfma_f32_32x32x2_f32) x 2 N tiles.  K runs over chunks of 16
//   input channels; per chunk the 10 x 18 input patch (the tile and its one-pixel halo; pixels outside the image are staged as zeros -
//   nothing is padded in HBM) and the 64 x 9 x 16 weight block are staged in LDS, the next chunk's loads being in flight in registers
//   while this one is multiplied.  Lane half `h` takes channels 8h .. 8h + 7 of a chunk for both operands (a fixed permutation of K).
//   A chunk's 144 products are summed in a fresh accumulator (the MFMA's k-ordered fp32 chain) which is then added to the running
//   one: a blocked sum, so the rounding error grows with sqrt(144) + sqrt(Cin / 16) rather than sqrt(9 Cin).
//   Epilogue: bias, ReLU, the full-resolution store and - for the four pooled taps - the 2 x 2 / floor max-pool straight from the
//   accumulators (a lane holds both columns and both rows of each of its 2 x 2 windows), so no pool kernel and no re-read.
// k_lpips_head: grid (chunks of 64 pixels, pairs).  One wave per pixel: the two channel norms, then sum_c lin[c] (f0 / n0 - f1 / n1)^2,
//   all in float64 from the fp32 features, butterfly-reduced (every lane ends with the same bits); a wave adds its 16 pixels in order,
//   the workgroup its 4 waves in order -> one partial in a fixed slot.  No float atomics.
// k_lpips_finish: grid (pairs).  Adds each tap's partials in a fixed order, divides by the tap's pixel count, writes the five d_k
//   and their sum (d_1 + ... + d_5, left to right).
#include "hl_reduce.h"

namespace hl {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kReduceThreads, "strided_sum reduces a workgroup of kReduceThreads");
constexpr int kTH = 8, kTW = 16;              // output pixels per workgroup (rows x columns)
constexpr int kPH = kTH + 2, kPW = kTW + 2;   // the staged patch
constexpr int kBN = 64;                       // output channels per workgroup
constexpr int kCK = 16;                       // input channels per K chunk
constexpr int kLD = 20;                       // LDS row stride in floats: 16 lanes' float4 reads at 20-dword strides hit 16 distinct bank quads
constexpr int kPatchF4 = kPH * kPW * (kCK / 4);                      // 720 float4 per chunk
constexpr int kPatchPer = (kPatchF4 + kThreads - 1) / kThreads;      // 3 per thread (the last one ragged)
constexpr int kWRows = kBN * 9;                                      // 576 (channel, tap) rows of 16 floats
constexpr int kWPer = kWRows * (kCK / 4) / kThreads;                 // 9 float4 per thread, exactly
static_assert(kWRows * (kCK / 4) % kThreads == 0, "weight block divides over the workgroup");
static_assert(kTH == 2 * (kThreads / 64) && kTW == 16, "a wave owns two rows of 16 pixels");
static_assert((kPH * kPW + kWRows) * kLD * 4 <= 64 * 1024, "static LDS");

constexpr int kConvs = HL_LPIPS_CONVS, kTaps = HL_LPIPS_TAPS;
constexpr int kWidth[kConvs] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kLevel[kConvs] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};      // resolution level (h >> level, floor at every step)
constexpr int kTapConv[kTaps] = {1, 3, 6, 9, 12};                            // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
constexpr int kHeadPix = 64;                                                 // pixels per workgroup of k_lpips_head
constexpr int kMaxSide = 16384;

__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }                      // NaN stays NaN, like torch.relu
__device__ __forceinline__ float max_f(float a, float b) { return (a > b || a != a) ? a : b; }      // NaN wins, like max_pool2d

__global__ __launch_bounds__(kThreads) void k_lpips_prep(const float *__restrict__ in0, const float *__restrict__ in1, int B, int64_t hw,
                                                        float s0, float s1, float s2, float c0, float c1, float c2,
                                                        float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int n = blockIdx.y;
    if (p >= hw) return;
    const float *src = (n < B ? in0 + (int64_t)n * 3 * hw : in1 + (int64_t)(n - B) * 3 * hw) + p;
    f32x4 v;
    v[0] = (src[0] - s0) / c0;
    v[1] = (src[hw] - s1) / c1;
    v[2] = (src[2 * hw] - s2) / c2;
    v[3] = 0.f;
    f32x4 *dst = reinterpret_cast<f32x4 *>(out + ((int64_t)n * hw + p) * kCK);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    dst[0] = v;
    dst[1] = z;
    dst[2] = z;
    dst[3] = z;
}

// in (N, H, W, Cin), Cin % 16 == 0; wpk (Cin / 16, Cout, 9, 16); out (N, H, W, Cout), Cout % 64 == 0; pool (N, H / 2, W / 2, Cout) or NULL
__global__ __launch_bounds__(kThreads, 2) void k_lpips_conv(const float *__restrict__ in, int H, int W, int Cin, const float *__restrict__ wpk,
                                                           const float *__restrict__ bias, int Cout, int tiles_x, float *__restrict__ out,
                                                           float *__restrict__ pool) {
    __shared__ __attribute__((aligned(16))) float s_patch[kPH * kPW * kLD];
    __shared__ __attribute__((aligned(16))) float s_w[kWRows * kLD];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int y0 = tyi * kTH, x0 = txi * kTW, n0 = (int)blockIdx.y * kBN;
    const int64_t img = blockIdx.z;
    const float *inb = in + img * H * W * Cin;

    int64_t p_off[kPatchPer];
    int p_lds[kPatchPer];
    bool p_ok[kPatchPer], p_st[kPatchPer];
#pragma unroll
    for (int i = 0; i < kPatchPer; ++i) {
        const int e = tid + i * kThreads, pix = e >> 2, q = e & 3;
        const int py = pix / kPW, px = pix - py * kPW;
        const int gy = y0 + py - 1, gx = x0 + px - 1;
        p_st[i] = e < kPatchF4;
        p_ok[i] = p_st[i] && gy >= 0 && gy < H && gx >= 0 && gx < W;          // the image border and ragged tiles: zeros in LDS
        p_off[i] = p_ok[i] ? ((int64_t)gy * W + gx) * Cin + q * 4 : 0;
        p_lds[i] = pix * kLD + q * 4;
    }
    const float *wsrc = wpk + (int64_t)n0 * (9 * kCK) + tid * 4;              // + chunk * Cout * 144; float4 i of this thread: + i * 1024
    const int w_lds = (tid >> 2) * kLD + (tid & 3) * 4;                        // float4 i: row + 64 i
    const int64_t w_chunk = (int64_t)Cout * (9 * kCK);

    f32x4 ra[kPatchPer], rw[kWPer];
    auto load_regs = [&](int c) {
#pragma unroll
        for (int i = 0; i < kPatchPer; ++i) {
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p_ok[i]) ra[i] = *reinterpret_cast<const f32x4 *>(inb + p_off[i] + c * kCK);
        }
#pragma unroll
        for (int i = 0; i < kWPer; ++i) rw[i] = *reinterpret_cast<const f32x4 *>(wsrc + c * w_chunk + i * (kThreads * 4));
    };
    auto store_lds = [&]() {
#pragma unroll
        for (int i = 0; i < kPatchPer; ++i)
            if (p_st[i]) *reinterpret_cast<f32x4 *>(s_patch + p_lds[i]) = ra[i];
#pragma unroll
        for (int i = 0; i < kWPer; ++i) *reinterpret_cast<f32x4 *>(s_w + w_lds + i * (kThreads / 4) * kLD) = rw[i];
    };

    const int a_base = ((2 * wave + (l31 >> 4)) * kPW + (l31 & 15)) * kLD + half * 8;
    const int b_base = l31 * 9 * kLD + half * 8;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int nch = Cin / kCK;
    load_regs(0);
    for (int c = 0; c < nch; ++c) {
        __syncthreads();                      // the previous chunk's reads are done
        store_lds();
        __syncthreads();
        if (c + 1 < nch) load_regs(c + 1);
        f32x16 part[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[j][r] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            const float *ap = s_patch + a_base + (ky * kPW + kx) * kLD;
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ap), a1 = *reinterpret_cast<const f32x4 *>(ap + 4);
            f32x4 b[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float *bp = s_w + b_base + (j * 32 * 9 + tap) * kLD;
                b[j][0] = *reinterpret_cast<const f32x4 *>(bp);
                b[j][1] = *reinterpret_cast<const f32x4 *>(bp + 4);
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(s < 4 ? a0[s & 3] : a1[s & 3], b[j][s >> 2][s & 3], part[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] += part[j];
    }

    // a lane holds channel n of the wave's pixels m = (r & 3) + 8 (r >> 2) + 4 half: row m >> 4, column m & 15
    const int row0 = y0 + 2 * wave;
    float *outb = out + img * H * W * Cout;
    const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + j * 32 + l31;
        const float bs = bias[n];
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            v[r] = relu_f(acc[j][r] + bs);
            const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int y = row0 + (m >> 4), x = x0 + (m & 15);
            if (y < H && x < W) outb[((int64_t)y * W + x) * Cout + n] = v[r];
        }
        if (pool) {                           // registers r, r + 1 are one row's column pair, r + 8 the row below (y0, x0 and m are even)
            const int yp = row0 >> 1;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int xp = (x0 + m) >> 1;
                if (yp < Hp && xp < Wp)       // floor mode: an odd last row or column is dropped
                    pool[((img * Hp + yp) * Wp + xp) * Cout + n] = max_f(max_f(v[r], v[r + 1]), max_f(v[r + 8], v[r + 9]));
            }
        }
    }
}

// f (N, hw, C) with C = 64 KC; pair b = images b and B + b
template <int KC>
__global__ __launch_bounds__(kThreads) void k_lpips_head(const float *__restrict__ f, int B, int64_t hw, const float *__restrict__ lin,
                                                        double *__restrict__ partial) {
    __shared__ double sh[kThreads / 64];
    constexpr int C = 64 * KC;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t b = blockIdx.y;
    const float *f0 = f + b * hw * C, *f1 = f + (b + B) * hw * C;
    float w[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) w[t] = lin[lane + 64 * t];
    double tot = 0.0;
    for (int i = 0; i < kHeadPix / 4; ++i) {
        const int64_t p = (int64_t)blockIdx.x * kHeadPix + 4 * i + wave;      // (uniform over the wave)
        if (p >= hw) break;
        float a[KC], c[KC];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int t = 0; t < KC; ++t) {
            a[t] = f0[p * C + lane + 64 * t];
            c[t] = f1[p * C + lane + 64 * t];
            s0 += (double)a[t] * (double)a[t];
            s1 += (double)c[t] * (double)c[t];
        }
        const double n0 = sqrt(wave_xor_sum(s0)) + 1e-10, n1 = sqrt(wave_xor_sum(s1)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int t = 0; t < KC; ++t) {
            const double e = (double)a[t] / n0 - (double)c[t] / n1;
            d += (double)w[t] * (e * e);
        }
        tot += wave_xor_sum(d);
    }
    if (lane == 0) sh[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct FinishArgs {
    int64_t off[kTaps];       // of a tap's partials, in doubles; pair b's run starts at off + b * chunks
    int chunks[kTaps];
    double hw[kTaps];
};

__global__ __launch_bounds__(kThreads) void k_lpips_finish(const double *__restrict__ partial, FinishArgs fa, double *__restrict__ out) {
    __shared__ double sh[kThreads];
    const int64_t b = blockIdx.x;
    const int tid = (int)threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < kTaps; ++k) {
        const double d = strided_sum(partial + fa.off[k] + b * fa.chunks[k], fa.chunks[k], 1, sh) / fa.hw[k];
        total += d;
        if (tid == 0) out[b * (kTaps + 1) + k] = d;
    }
    if (tid == 0) out[b * (kTaps + 1) + kTaps] = total;
}

// Workspace of N images of h x w: the five taps (kept for the head and for callers who want the features), two scratch tensors the
// other activations alternate between, the head's partials (one run per tap for N / 2 pairs at the most; sized for N).
struct Plan {
    int h[kTaps], w[kTaps];
    size_t tap_off[kTaps], scratch_off[2], part_off[kTaps], bytes;
    int chunks[kTaps];
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline bool plan(int N, int h, int w, Plan &p) {
    if (N <= 0 || N > 65535 || h < 16 || w < 16 || h > kMaxSide || w > kMaxSide) return false;
    size_t off = 0;
    for (int k = 0; k < kTaps; ++k) {
        p.h[k] = h >> k;
        p.w[k] = w >> k;
        p.tap_off[k] = off;
        off = align256(off + (size_t)N * p.h[k] * p.w[k] * kWidth[kTapConv[k]] * sizeof(float));
    }
    const size_t scratch = align256((size_t)N * h * w * 64 * sizeof(float));      // the largest non-tap activation: conv1_1's output
    for (int s = 0; s < 2; ++s) {
        p.scratch_off[s] = off;
        off += scratch;
    }
    for (int k = 0; k < kTaps; ++k) {
        p.chunks[k] = (int)(((int64_t)p.h[k] * p.w[k] + kHeadPix - 1) / kHeadPix);
        p.part_off[k] = off;
        off = align256(off + (size_t)N * p.chunks[k] * sizeof(double));
    }
    p.bytes = off;
    return true;
}

int launch_conv(const float *in, int N, int H, int W, int Cin, const float *wpk, const float *bias, int Cout, float *out, float *pool,
                hipStream_t st) {
    const int tx = (W + kTW - 1) / kTW, ty = (H + kTH - 1) / kTH;
    hipLaunchKernelGGL(k_lpips_conv, dim3(tx * ty, Cout / kBN, N), dim3(kThreads), 0, st, in, H, W, Cin, wpk, bias, Cout, tx, out, pool);
    return check_launch("k_lpips_conv");
}

bool params_ok(const hl_lpips_params *P) {
    if (!P) return false;
    for (int l = 0; l < kConvs; ++l)
        if (!P->conv_w[l] || !P->conv_b[l]) return false;
    for (int k = 0; k < kTaps; ++k)
        if (!P->lin[k]) return false;
    for (int c = 0; c < 3; ++c)
        if (!(P->scale[c] != 0.f)) return false;
    return true;
}

int trunk(const hl_lpips_params *P, const float *in0, const float *in1, int B, int N, int h, int w, const Plan &p, char *ws, hipStream_t st) {
    float *scratch[2] = {reinterpret_cast<float *>(ws + p.scratch_off[0]), reinterpret_cast<float *>(ws + p.scratch_off[1])};
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(k_lpips_prep, dim3((unsigned)((hw + kThreads - 1) / kThreads), N), dim3(kThreads), 0, st, in0, in1, B, hw, P->shift[0],
                       P->shift[1], P->shift[2], P->scale[0], P->scale[1], P->scale[2], scratch[1]);
    int rc = check_launch("k_lpips_prep");
    if (rc != HL_OK) return rc;
    const float *cur = scratch[1];
    int side = 0, cin = kCK, tap = 0;          // the next non-tap output goes to scratch[side]
    for (int l = 0; l < kConvs; ++l) {
        const int lv = kLevel[l];
        const bool is_tap = l == kTapConv[tap];
        float *out = is_tap ? reinterpret_cast<float *>(ws + p.tap_off[tap]) : scratch[side];
        float *pool = is_tap && tap + 1 < kTaps ? scratch[side] : nullptr;
        rc = launch_conv(cur, N, p.h[lv], p.w[lv], cin, P->conv_w[l], P->conv_b[l], kWidth[l], out, pool, st);
        if (rc != HL_OK) return rc;
        cur = scratch[side];                   // this layer's output, or its pooled form after a tap
        side ^= 1;
        cin = kWidth[l];
        if (is_tap) ++tap;
    }
    return HL_OK;
}

template <int KC>
int launch_head(const float *f, int B, int64_t hw, const float *lin, double *partial, int chunks, hipStream_t st) {
    hipLaunchKernelGGL(k_lpips_head<KC>, dim3(chunks, B), dim3(kThreads), 0, st, f, B, hw, lin, partial);
    return check_launch("k_lpips_head");
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

size_t hl_lpips_workspace_bytes(int N, int h, int w) {
    Plan p;
    return plan(N, h, w, p) ? p.bytes : 0;
}

int hl_lpips_tap_shape(int N, int h, int w, int k, size_t *offset_bytes, int *hk, int *wk, int *channels) {
    Plan p;
    HL_REQUIRE(plan(N, h, w, p), "hl_lpips_tap_shape: bad shape (%d images of %d x %d; 1..65535 images, 16 <= h, w <= %d)", N, h, w, kMaxSide);
    HL_REQUIRE(k >= 0 && k < kTaps && offset_bytes && hk && wk && channels, "hl_lpips_tap_shape: tap %d of %d, or a NULL result", k, kTaps);
    *offset_bytes = p.tap_off[k];
    *hk = p.h[k];
    *wk = p.w[k];
    *channels = kWidth[kTapConv[k]];
    return HL_OK;
}

int hl_lpips_features(const hl_lpips_params *params, const float *in0, const float *in1, int B, int h, int w, void *workspace,
                      size_t workspace_bytes, void *stream) {
    Plan p;
    const int N = in1 ? 2 * B : B;
    HL_REQUIRE(params_ok(params) && in0, "hl_lpips_features: NULL argument or a zero scale");
    HL_REQUIRE(B > 0 && plan(N, h, w, p), "hl_lpips_features: bad shape (%d images of %d x %d; 1..65535 images, 16 <= h, w <= %d)", N, h, w,
               kMaxSide);
    HL_REQUIRE(workspace && workspace_bytes >= p.bytes, "hl_lpips_features: workspace too small (%zu bytes, need %zu)", workspace_bytes, p.bytes);
    return trunk(params, in0, in1 ? in1 : in0, B, N, h, w, p, static_cast<char *>(workspace), (hipStream_t)stream);
}

int hl_lpips(const hl_lpips_params *params, const float *in0, const float *in1, int B, int h, int w, double *out, void *workspace,
             size_t workspace_bytes, void *stream) {
    Plan p;
    HL_REQUIRE(params_ok(params) && in0 && in1 && out, "hl_lpips: NULL argument or a zero scale");
    HL_REQUIRE(B > 0 && B <= 32767 && plan(2 * B, h, w, p), "hl_lpips: bad shape (%d pairs of %d x %d; 1..32767 pairs, 16 <= h, w <= %d)", B, h, w,
               kMaxSide);
    HL_REQUIRE(workspace && workspace_bytes >= p.bytes, "hl_lpips: workspace too small (%zu bytes, need %zu)", workspace_bytes, p.bytes);
    char *ws = static_cast<char *>(workspace);
    const hipStream_t st = (hipStream_t)stream;
    int rc = trunk(params, in0, in1, B, 2 * B, h, w, p, ws, st);
    if (rc != HL_OK) return rc;
    FinishArgs fa;
    for (int k = 0; k < kTaps; ++k) {
        const float *f = reinterpret_cast<const float *>(ws + p.tap_off[k]);
        double *part = reinterpret_cast<double *>(ws + p.part_off[k]);
        const int64_t hw = (int64_t)p.h[k] * p.w[k];
        switch (kWidth[kTapConv[k]] / 64) {
        case 1: rc = launch_head<1>(f, B, hw, params->lin[k], part, p.chunks[k], st); break;
        case 2: rc = launch_head<2>(f, B, hw, params->lin[k], part, p.chunks[k], st); break;
        case 4: rc = launch_head<4>(f, B, hw, params->lin[k], part, p.chunks[k], st); break;
        default: rc = launch_head<8>(f, B, hw, params->lin[k], part, p.chunks[k], st); break;
        }
        if (rc != HL_OK) return rc;
        fa.off[k] = (int64_t)((p.part_off[k] - p.part_off[0]) / sizeof(double));
        fa.chunks[k] = p.chunks[k];
        fa.hw[k] = (double)hw;
    }
    hipLaunchKernelGGL(k_lpips_finish, dim3(B), dim3(kThreads), 0, st, reinterpret_cast<const double *>(ws + p.part_off[0]), fa, out);
    return check_launch("k_lpips_finish");
}

}  // extern "C"
