// FID on the device, MI355X (gfx950): the pool3 features of pytorch-fid's InceptionV3 (the FID variant of torchvision's Inception3) and
// the float64 moments of a feature set.  Contract: DESIGN.md 4l "FID"; exact fp32 products throughout.  The architecture was written
// down from the published description of the network; it has NOT been checked against pytorch-fid's own weights.
//
// k_fid_prep: (N, 3, h, w) NCHW in [0, 1] -> (N, H, W, 16) NHWC: optional bilinear resize to 299 x 299 (align_corners = False, no
//   antialiasing; coordinates, weights and the blend in float64, rounded once), optional 2 x - 1, zeros in channels 3..15 so that the
//   first convolution is the same implicit GEMM as the other 93 with one (zero-padded) K chunk.
// k_fid_conv<NT>: convolution (kH x kW, stride sH x sW, pad pH x pW) + bias + ReLU, NHWC fp32, BatchNorm folded into weight and bias by
//   the caller.  An implicit GEMM on v_mfma_f32_32x32x2_f32 whose M is the flattened output pixel (image, row, column): the batch folds
//   into M, so the 8 x 8 and 17 x 17 maps of a batch still fill 128-pixel tiles.  A workgroup (4 waves) owns 128 pixels x NT tiles of 32
//   output channels; wave w owns pixels 32 w .. 32 w + 31.  K runs over steps (tap, chunk of 16 input channels), taps outermost, in one
//   fixed order; per step each pixel's 16 input values at that tap (zeros where the tap falls outside the image - nothing is padded in
//   HBM) and the NT x 32 x 16 weight block go through registers (the next step's loads in flight while this one is multiplied) into one
//   of two LDS buffers: one barrier per step.  Lane half `h` takes channels 8 h .. 8 h + 7 of a chunk for both operands (a fixed
//   permutation of K).  Eight steps (128 products) are summed in a fresh accumulator, the MFMA's k-ordered fp32 chain, which is then
//   added to the running one: a blocked sum.  No split-K, no atomics: an output element's sum has one order, whatever tile it falls in,
//   so an image's result has the same bits alone and inside a batch.  Epilogue: bias, ReLU, store at a channel offset of a wider
//   output (the block's concatenation); channels past Cout (the packed weights are padded to 32 with zeros) are not stored.
// k_fid_pool<MODE>: 3 x 3 max (stride 1 or 2, pad 0 or 1; NaN wins, like max_pool2d) or 3 x 3 / stride 1 / pad 1 average over the in-image
//   taps (count_include_pad = False: taps added in row-major order, divided by their count), written at a channel offset.
// k_fid_gap: the mean over the map, float64 accumulation in pixel order, stored as fp32.
// k_fid_moments_s / k_fid_moments_S: s[i] += x[i], S[i][j] += x[i] x[j] over the images of a batch strictly in order, fp32 features
//   widened to float64, the product and the sum rounded separately.  S is computed on the 64 x 64 tiles of the upper triangle only.
// k_fid_finalize: mu = s / N; sigma[i][j] = (S[i][j] - (N mu[i]) mu[j]) / (N - 1) for i <= j, every operation rounded separately, and
//   sigma[j][i] = sigma[i][j].
#include "hl_common.h"

namespace hl {
namespace {

constexpr int kThreads = 256;
constexpr int kBM = 128;                      // output pixels per workgroup
constexpr int kCK = 16;                       // input channels per K step
constexpr int kLD = 20;                       // LDS row stride in floats: 16 lanes' float4 reads at 20-dword strides hit 16 distinct bank quads
constexpr int kFold = 8;                      // K steps summed in the fresh accumulator before it is added to the running one
constexpr int kLayers = HL_FID_LAYERS;
constexpr int kD = HL_FID_DIMS;
constexpr int kSide = 299;
constexpr int kMinSide = 75;                  // the smallest map every stride-2 stage still maps to >= 1 pixel
constexpr int kMaxSide = 16384;
constexpr int kMaxImages = 4096;

struct Layer {
    char name[40];
    int cin, cout, kh, kw, sh, sw, ph, pw;
};

// ---- the layer table: the 94 BasicConv2d of the network in the order the forward runs them ----
struct Table {
    Layer row[kLayers];
    int n = 0;
    void add(const char *block, const char *name, int cin, int cout, int kh, int kw, int s = 1, int ph = 0, int pw = 0) {
        Layer &l = row[n++];
        snprintf(l.name, sizeof(l.name), "%s%s%s", block, *block ? "." : "", name);
        l.cin = cin, l.cout = cout, l.kh = kh, l.kw = kw, l.sh = s, l.sw = s, l.ph = ph, l.pw = pw;
    }
    void a(const char *b, int cin, int pf) {
        add(b, "branch1x1", cin, 64, 1, 1);
        add(b, "branch5x5_1", cin, 48, 1, 1);
        add(b, "branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
        add(b, "branch3x3dbl_1", cin, 64, 1, 1);
        add(b, "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
        add(b, "branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
        add(b, "branch_pool", cin, pf, 1, 1);
    }
    void c(const char *b, int c7) {
        add(b, "branch1x1", 768, 192, 1, 1);
        add(b, "branch7x7_1", 768, c7, 1, 1);
        add(b, "branch7x7_2", c7, c7, 1, 7, 1, 0, 3);
        add(b, "branch7x7_3", c7, 192, 7, 1, 1, 3, 0);
        add(b, "branch7x7dbl_1", 768, c7, 1, 1);
        add(b, "branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0);
        add(b, "branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3);
        add(b, "branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0);
        add(b, "branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3);
        add(b, "branch_pool", 768, 192, 1, 1);
    }
    void e(const char *b, int cin) {
        add(b, "branch1x1", cin, 320, 1, 1);
        add(b, "branch3x3_1", cin, 384, 1, 1);
        add(b, "branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
        add(b, "branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
        add(b, "branch3x3dbl_1", cin, 448, 1, 1);
        add(b, "branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
        add(b, "branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
        add(b, "branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
        add(b, "branch_pool", cin, 192, 1, 1);
    }
    Table() {
        add("", "Conv2d_1a_3x3", 3, 32, 3, 3, 2);
        add("", "Conv2d_2a_3x3", 32, 32, 3, 3);
        add("", "Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
        add("", "Conv2d_3b_1x1", 64, 80, 1, 1);
        add("", "Conv2d_4a_3x3", 80, 192, 3, 3);
        a("Mixed_5b", 192, 32);
        a("Mixed_5c", 256, 64);
        a("Mixed_5d", 288, 64);
        add("Mixed_6a", "branch3x3", 288, 384, 3, 3, 2);
        add("Mixed_6a", "branch3x3dbl_1", 288, 64, 1, 1);
        add("Mixed_6a", "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
        add("Mixed_6a", "branch3x3dbl_3", 96, 96, 3, 3, 2);
        c("Mixed_6b", 128);
        c("Mixed_6c", 160);
        c("Mixed_6d", 160);
        c("Mixed_6e", 192);
        add("Mixed_7a", "branch3x3_1", 768, 192, 1, 1);
        add("Mixed_7a", "branch3x3_2", 192, 320, 3, 3, 2);
        add("Mixed_7a", "branch7x7x3_1", 768, 192, 1, 1);
        add("Mixed_7a", "branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
        add("Mixed_7a", "branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
        add("Mixed_7a", "branch7x7x3_4", 192, 192, 3, 3, 2);
        e("Mixed_7b", 1280);
        e("Mixed_7c", 2048);
    }
};

const Table &table() {
    static const Table t;
    return t;
}

__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }                      // NaN stays NaN, like torch.relu
__device__ __forceinline__ float max_f(float a, float b) { return (a > b || a != a) ? a : b; }      // NaN wins, like max_pool2d

// ---- prep ----
__global__ __launch_bounds__(kThreads) void k_fid_prep(const float *__restrict__ in, int h, int w, int H, int W, int resize, int normalize,
                                                      float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t n = blockIdx.y;
    if (p >= (int64_t)H * W) return;
    const int oy = (int)(p / W), ox = (int)(p - (int64_t)oy * W);
    const float *src = in + n * 3 * h * w;
    const int64_t hw = (int64_t)h * w;
    double v[3];
    if (resize) {
        // torch's area_pixel_compute_source_index for align_corners = False: scale (dst + 0.5) - 0.5, negative -> 0
        double sy = ((double)h / (double)H) * ((double)oy + 0.5) - 0.5, sx = ((double)w / (double)W) * ((double)ox + 0.5) - 0.5;
        sy = sy < 0.0 ? 0.0 : sy;
        sx = sx < 0.0 ? 0.0 : sx;
        int y0 = (int)sy, x0 = (int)sx;
        y0 = y0 > h - 1 ? h - 1 : y0;
        x0 = x0 > w - 1 ? w - 1 : x0;
        const int y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1, x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1;
        const double ly = sy - (double)y0, lx = sx - (double)x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *s = src + c * hw;
            const double top = (1.0 - lx) * (double)s[(int64_t)y0 * w + x0] + lx * (double)s[(int64_t)y0 * w + x1];
            const double bot = (1.0 - lx) * (double)s[(int64_t)y1 * w + x0] + lx * (double)s[(int64_t)y1 * w + x1];
            v[c] = (1.0 - ly) * top + ly * bot;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)src[c * hw + p];
    }
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (float)(normalize ? 2.0 * v[c] - 1.0 : v[c]);
    o[3] = 0.f;
    f32x4 *dst = reinterpret_cast<f32x4 *>(out + (n * H * W + p) * kCK);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    dst[0] = o;
    dst[1] = z;
    dst[2] = z;
    dst[3] = z;
}

// ---- convolution ----
struct ConvArgs {
    const float *in;      // (N, H, W, Cin), Cin % 16 == 0
    const float *wpk;     // (kH kW, Cin / 16, CoutP, 16), CoutP = Cout rounded up to 32, zeros in the padding
    const float *bias;    // (Cout)
    float *out;           // (N, Ho, Wo, ldo); this layer's channels start at coff
    int H, W, Cin, Ho, Wo, Cout, kH, kW, sH, sW, pH, pW, ldo, coff;
    int64_t M;            // N Ho Wo
};

template <int NT>
__global__ __launch_bounds__(kThreads, 2) void k_fid_conv(const ConvArgs a) {
    constexpr int kAPer = kBM * (kCK / 4) / kThreads;                     // 2 float4 of the pixel block per thread
    constexpr int kBF4 = NT * 32 * (kCK / 4);                             // float4 of the weight block
    constexpr int kBPer = (kBF4 + kThreads - 1) / kThreads;
    __shared__ __attribute__((aligned(16))) float s_a[2][kBM * kLD];
    __shared__ __attribute__((aligned(16))) float s_b[2][NT * 32 * kLD];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int64_t m0 = (int64_t)blockIdx.x * kBM;
    const int nt0 = (int)blockIdx.y * NT;                                 // first tile of 32 output channels
    const int CoutP = (a.Cout + 31) & ~31;
    const int nch = a.Cin / kCK, steps = a.kH * a.kW * nch;

    int64_t p_img[kAPer];                                                 // the image's first element
    int p_y[kAPer], p_x[kAPer], p_lds[kAPer];                             // input row / column of tap (0, 0)
    bool p_ok[kAPer];
#pragma unroll
    for (int i = 0; i < kAPer; ++i) {
        const int e = tid + i * kThreads, pix = e >> 2, q = e & 3;
        const int64_t m = m0 + pix;
        p_ok[i] = m < a.M;
        const int64_t mm = p_ok[i] ? m : 0;
        const int64_t img = mm / ((int64_t)a.Ho * a.Wo);
        const int rem = (int)(mm - img * a.Ho * a.Wo);
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        p_img[i] = img * a.H * a.W * a.Cin + q * 4;
        p_y[i] = oy * a.sH - a.pH;
        p_x[i] = ox * a.sW - a.pW;
        p_lds[i] = pix * kLD + q * 4;
    }
    int b_lds[kBPer];
    int64_t b_off[kBPer];
    bool b_st[kBPer], b_ok[kBPer];
#pragma unroll
    for (int i = 0; i < kBPer; ++i) {
        const int e = tid + i * kThreads, row = e >> 2, q = e & 3;
        b_st[i] = e < kBF4;
        b_ok[i] = b_st[i] && nt0 * 32 + row < CoutP;                     // a last, partly empty group of tiles: zeros
        b_off[i] = b_ok[i] ? ((int64_t)(nt0 * 32 + row)) * kCK + q * 4 : 0;
        b_lds[i] = row * kLD + q * 4;
    }
    const int64_t w_step = (int64_t)CoutP * kCK;

    f32x4 ra[kAPer], rb[kBPer];
    auto load_regs = [&](int s) {
        const int tap = s / nch, c = s - tap * nch;
        const int ky = tap / a.kW, kx = tap - ky * a.kW;
#pragma unroll
        for (int i = 0; i < kAPer; ++i) {
            const int iy = p_y[i] + ky, ix = p_x[i] + kx;
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p_ok[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                ra[i] = *reinterpret_cast<const f32x4 *>(a.in + p_img[i] + ((int64_t)iy * a.W + ix) * a.Cin + c * kCK);
        }
#pragma unroll
        for (int i = 0; i < kBPer; ++i) {
            rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (b_ok[i]) rb[i] = *reinterpret_cast<const f32x4 *>(a.wpk + s * w_step + b_off[i]);
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kAPer; ++i) *reinterpret_cast<f32x4 *>(s_a[buf] + p_lds[i]) = ra[i];
#pragma unroll
        for (int i = 0; i < kBPer; ++i)
            if (b_st[i]) *reinterpret_cast<f32x4 *>(s_b[buf] + b_lds[i]) = rb[i];
    };

    const int a_base = (32 * wave + l31) * kLD + half * 8;
    const int b_base = l31 * kLD + half * 8;
    f32x16 acc[NT], part[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f, part[j][r] = 0.f;

    load_regs(0);
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        store_lds(buf);                       // (this buffer was last read two steps ago, before the previous step's barrier)
        __syncthreads();
        if (s + 1 < steps) load_regs(s + 1);
        const float *ap = s_a[buf] + a_base;
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ap), a1 = *reinterpret_cast<const f32x4 *>(ap + 4);
        f32x4 b[NT][2];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float *bp = s_b[buf] + b_base + j * 32 * kLD;
            b[j][0] = *reinterpret_cast<const f32x4 *>(bp);
            b[j][1] = *reinterpret_cast<const f32x4 *>(bp + 4);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(k < 4 ? a0[k & 3] : a1[k & 3], b[j][k >> 2][k & 3], part[j], 0, 0, 0);
        if ((s & (kFold - 1)) == kFold - 1 || s + 1 == steps) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] += part[j];
#pragma unroll
                for (int r = 0; r < 16; ++r) part[j][r] = 0.f;
            }
        }
    }

    // a lane holds channel l31 of the wave's pixels (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = (nt0 + j) * 32 + l31;
        if (n >= a.Cout) continue;
        const float bs = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m < a.M) a.out[m * a.ldo + a.coff + n] = relu_f(acc[j][r] + bs);
        }
    }
}

// ---- pools ----
enum { kPoolMax = 0, kPoolAvg = 1 };

// in (N, H, W, C), C % 4 == 0; out (N, Ho, Wo, ldo) at channel offset coff; 3 x 3 window
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_fid_pool(const float *__restrict__ in, int H, int W, int C, int Ho, int Wo, int stride, int pad,
                                                      float *__restrict__ out, int ldo, int coff, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int c4 = C / 4;
    const int q = (int)(idx % c4);
    const int64_t m = idx / c4;
    const int64_t img = m / ((int64_t)Ho * Wo);
    const int rem = (int)(m - img * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const float *src = in + img * H * W * C + q * 4;
    const float ninf = -__builtin_inff();
    f32x4 v = MODE == kPoolMax ? f32x4{ninf, ninf, ninf, ninf} : f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const f32x4 x = *reinterpret_cast<const f32x4 *>(src + ((int64_t)iy * W + ix) * C);
            ++cnt;
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = MODE == kPoolMax ? max_f(v[t], x[t]) : v[t] + x[t];
        }
    if (MODE == kPoolAvg) {
        const float d = (float)cnt;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = v[t] / d;
    }
    *reinterpret_cast<f32x4 *>(out + m * ldo + coff + q * 4) = v;
}

// in (N, hw, C) -> out (N, C) (and out2, if given): the mean over the map
__global__ __launch_bounds__(kThreads) void k_fid_gap(const float *__restrict__ in, int64_t hw, int C, float *__restrict__ out,
                                                     float *__restrict__ out2) {
    const int c = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    const int64_t n = blockIdx.y;
    if (c >= C) return;
    const float *src = in + n * hw * C + c;
    double acc = 0.0;
    for (int64_t p = 0; p < hw; ++p) acc = __dadd_rn(acc, (double)src[p * C]);
    const float r = (float)__ddiv_rn(acc, (double)hw);
    out[n * C + c] = r;
    if (out2) out2[n * C + c] = r;
}

// ---- moments ----
constexpr int kMT = 64;                       // tile of S per workgroup
constexpr int kMB = 32;                       // images staged per round
constexpr int kMTiles = kD / kMT;
static_assert(kD % kMT == 0 && kMT * kMT == kThreads * 16, "a thread owns 4 x 4 elements of a 64 x 64 tile");

__global__ __launch_bounds__(kThreads) void k_fid_moments_s(const float *__restrict__ x, int n, double *__restrict__ s) {
    const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i >= kD) return;
    double acc = s[i];
    for (int b = 0; b < n; ++b) acc = __dadd_rn(acc, (double)x[(int64_t)b * kD + i]);
    s[i] = acc;
}

__global__ __launch_bounds__(kThreads) void k_fid_moments_S(const float *__restrict__ x, int n, double *__restrict__ S) {
    __shared__ float xi[kMB][kMT], xj[kMB][kMT];
    // blockIdx.x -> the tile (ti, tj), ti <= tj, of the upper triangle in row-major order
    int ti = 0, left = (int)blockIdx.x;
    while (left >= kMTiles - ti) {
        left -= kMTiles - ti;
        ++ti;
    }
    const int tj = ti + left;
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = ti * kMT, j0 = tj * kMT;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = S[(int64_t)(i0 + ty + 16 * p) * kD + j0 + tx + 16 * q];
    for (int b0 = 0; b0 < n; b0 += kMB) {
        const int nb = n - b0 < kMB ? n - b0 : kMB;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMB * kMT / kThreads; ++k) {
            const int e = tid + k * kThreads, r = e >> 6, c = e & 63;
            if (r < nb) {
                xi[r][c] = x[(int64_t)(b0 + r) * kD + i0 + c];
                xj[r][c] = x[(int64_t)(b0 + r) * kD + j0 + c];
            }
        }
        __syncthreads();
        for (int r = 0; r < nb; ++r) {
            double u[4], v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) u[p] = (double)xi[r][ty + 16 * p], v[p] = (double)xj[r][tx + 16 * p];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = __dadd_rn(acc[p][q], __dmul_rn(u[p], v[q]));
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) S[(int64_t)(i0 + ty + 16 * p) * kD + j0 + tx + 16 * q] = acc[p][q];
}

__global__ __launch_bounds__(kThreads) void k_fid_mu(const double *__restrict__ s, double count, double *__restrict__ mu) {
    const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i < kD) mu[i] = __ddiv_rn(s[i], count);
}

// thread (i, j) evaluates the element (min, max) of the upper triangle: both halves get the same bits
__global__ __launch_bounds__(kThreads) void k_fid_finalize(const double *__restrict__ S, const double *__restrict__ mu, double count,
                                                          double *__restrict__ sigma) {
    const int j = (int)blockIdx.x * kThreads + (int)threadIdx.x, i = (int)blockIdx.y;
    if (j >= kD) return;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double v = __dsub_rn(S[(int64_t)lo * kD + hi], __dmul_rn(__dmul_rn(count, mu[lo]), mu[hi]));
    sigma[(int64_t)i * kD + j] = __ddiv_rn(v, count - 1.0);
}

// ---- the forward: one routine walks the network, as a dry run (sizes of the workspace's slots) or launching ----
enum Slot { kB0, kB1, kB2, kB3, kPrep, kTr0, kTr1, kT0, kT1, kT2, kSlots };

struct Plan {
    size_t size[kSlots], off[kSlots], bytes;
    int bh[4], bw[4], bc[4];       // the four block outputs
};

struct Tensor {
    int slot, h, w, c;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Walk {
    const hl_fid_params *P;        // NULL: dry run
    char *ws;
    Plan &plan;
    int N;
    hipStream_t st;
    int cur = 0, rc = HL_OK;

    float *ptr(const Tensor &t) const { return reinterpret_cast<float *>(ws + plan.off[t.slot]); }
    Tensor make(int slot, int h, int w, int c) {
        const size_t b = align256((size_t)N * h * w * c * sizeof(float));
        if (!P && b > plan.size[slot]) plan.size[slot] = b;
        return Tensor{slot, h, w, c};
    }
    // the next layer of the table, from `in` into channels coff .. of `out`
    void conv(const Tensor &in, const Tensor &out, int coff) {
        const Layer &l = table().row[cur];
        const int li = cur++;
        if (rc != HL_OK || !P) return;
        ConvArgs a;
        a.in = ptr(in), a.wpk = P->conv_w[li], a.bias = P->conv_b[li], a.out = ptr(out);
        a.H = in.h, a.W = in.w, a.Cin = in.c, a.Ho = out.h, a.Wo = out.w, a.Cout = l.cout;
        a.kH = l.kh, a.kW = l.kw, a.sH = l.sh, a.sW = l.sw, a.pH = l.ph, a.pW = l.pw, a.ldo = out.c, a.coff = coff;
        a.M = (int64_t)N * out.h * out.w;
        const int tiles = (l.cout + 31) / 32;
        const unsigned gm = (unsigned)((a.M + kBM - 1) / kBM);
        // three tiles per workgroup where they divide the layer (96, 192, 384), two otherwise; a launch that would leave most of the
        // device idle takes one tile per workgroup instead
        int nt = tiles % 3 == 0 ? 3 : 2;
        if ((int64_t)gm * ((tiles + nt - 1) / nt) < 256) nt = 1;
        const dim3 grid(gm, (tiles + nt - 1) / nt);
        if (nt == 3) hipLaunchKernelGGL(k_fid_conv<3>, grid, dim3(kThreads), 0, st, a);
        else if (nt == 2) hipLaunchKernelGGL(k_fid_conv<2>, grid, dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL(k_fid_conv<1>, grid, dim3(kThreads), 0, st, a);
        rc = check_launch("k_fid_conv");
    }
    int out_h(int h) const { const Layer &l = table().row[cur]; return (h + 2 * l.ph - l.kh) / l.sh + 1; }
    int out_w(int w) const { const Layer &l = table().row[cur]; return (w + 2 * l.pw - l.kw) / l.sw + 1; }
    // the next layer into a tensor of its own
    Tensor conv_to(const Tensor &in, int slot) {
        const Tensor out = make(slot, out_h(in.h), out_w(in.w), table().row[cur].cout);
        conv(in, out, 0);
        return out;
    }
    void pool(int mode, const Tensor &in, const Tensor &out, int coff, int stride, int pad) {
        if (rc != HL_OK || !P) return;
        const int64_t total = (int64_t)N * out.h * out.w * (in.c / 4);
        const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
        if (mode == kPoolMax)
            hipLaunchKernelGGL(k_fid_pool<kPoolMax>, grid, dim3(kThreads), 0, st, ptr(in), in.h, in.w, in.c, out.h, out.w, stride, pad, ptr(out),
                               out.c, coff, total);
        else
            hipLaunchKernelGGL(k_fid_pool<kPoolAvg>, grid, dim3(kThreads), 0, st, ptr(in), in.h, in.w, in.c, out.h, out.w, stride, pad, ptr(out),
                               out.c, coff, total);
        rc = check_launch("k_fid_pool");
    }
    Tensor pool_to(int mode, const Tensor &in, int slot, int stride, int pad) {
        const Tensor out = make(slot, (in.h + 2 * pad - 3) / stride + 1, (in.w + 2 * pad - 3) / stride + 1, in.c);
        pool(mode, in, out, 0, stride, pad);
        return out;
    }

    Tensor mixed_a(const Tensor &x, int slot, int pf) {
        const Tensor y = make(slot, x.h, x.w, 224 + pf);
        conv(x, y, 0);
        conv(conv_to(x, kT0), y, 64);
        conv(conv_to(conv_to(x, kT0), kT1), y, 128);
        conv(pool_to(kPoolAvg, x, kT2, 1, 1), y, 224);
        return y;
    }
    Tensor mixed_b(const Tensor &x, int slot) {
        const Tensor y = make(slot, (x.h - 3) / 2 + 1, (x.w - 3) / 2 + 1, 768);
        conv(x, y, 0);
        conv(conv_to(conv_to(x, kT0), kT1), y, 384);
        pool(kPoolMax, x, y, 480, 2, 0);
        return y;
    }
    Tensor mixed_c(const Tensor &x, int slot) {
        const Tensor y = make(slot, x.h, x.w, 768);
        conv(x, y, 0);
        conv(conv_to(conv_to(x, kT0), kT1), y, 192);
        conv(conv_to(conv_to(conv_to(conv_to(x, kT0), kT1), kT0), kT1), y, 384);
        conv(pool_to(kPoolAvg, x, kT2, 1, 1), y, 576);
        return y;
    }
    Tensor mixed_d(const Tensor &x, int slot) {
        const Tensor y = make(slot, (x.h - 3) / 2 + 1, (x.w - 3) / 2 + 1, 1280);
        conv(conv_to(x, kT0), y, 0);
        conv(conv_to(conv_to(conv_to(x, kT0), kT1), kT0), y, 320);
        pool(kPoolMax, x, y, 512, 2, 0);
        return y;
    }
    Tensor mixed_e(const Tensor &x, int slot, int pool_mode) {
        const Tensor y = make(slot, x.h, x.w, 2048);
        conv(x, y, 0);
        Tensor t = conv_to(x, kT0);
        conv(t, y, 320);
        conv(t, y, 704);
        t = conv_to(conv_to(x, kT0), kT1);
        conv(t, y, 1088);
        conv(t, y, 1472);
        conv(pool_to(pool_mode, x, kT2, 1, 1), y, 1856);
        return y;
    }

    // `in` (N, 3, h, w); the network's input is H x W (299 x 299 when resizing, h x w otherwise)
    int run(const float *in, int h, int w, int H, int W, int resize, int normalize, float *out) {
        Tensor x = make(kPrep, H, W, kCK);
        if (P) {
            hipLaunchKernelGGL(k_fid_prep, dim3((unsigned)(((int64_t)H * W + kThreads - 1) / kThreads), N), dim3(kThreads), 0, st, in, h, w, H, W,
                               resize, normalize, ptr(x));
            rc = check_launch("k_fid_prep");
        }
        x = conv_to(conv_to(conv_to(x, kT0), kT1), kT0);
        const Tensor b0 = pool_to(kPoolMax, x, kB0, 2, 0);
        x = conv_to(conv_to(b0, kT0), kT1);
        const Tensor b1 = pool_to(kPoolMax, x, kB1, 2, 0);
        x = mixed_a(b1, kTr0, 32);
        x = mixed_a(x, kTr1, 64);
        x = mixed_a(x, kTr0, 64);
        x = mixed_b(x, kTr1);
        x = mixed_c(x, kTr0);
        x = mixed_c(x, kTr1);
        x = mixed_c(x, kTr0);
        const Tensor b2 = mixed_c(x, kB2);
        x = mixed_d(b2, kTr0);
        x = mixed_e(x, kTr1, kPoolAvg);
        x = mixed_e(x, kTr0, kPoolMax);
        const Tensor b3 = make(kB3, 1, 1, kD);
        if (P && rc == HL_OK) {
            hipLaunchKernelGGL(k_fid_gap, dim3(kD / kThreads, N), dim3(kThreads), 0, st, ptr(x), (int64_t)x.h * x.w, kD, ptr(b3), out);
            rc = check_launch("k_fid_gap");
        }
        if (!P) {
            const Tensor *b[4] = {&b0, &b1, &b2, &b3};
            for (int k = 0; k < 4; ++k) plan.bh[k] = b[k]->h, plan.bw[k] = b[k]->w, plan.bc[k] = b[k]->c;
        }
        return cur == kLayers ? rc : fail(HL_ERR_RUNTIME, "hl_fid: the forward used %d of the table's %d layers", cur, kLayers);
    }
};

inline bool shape_ok(int N, int h, int w, int resize) {
    if (N <= 0 || N > kMaxImages || h > kMaxSide || w > kMaxSide) return false;
    return resize ? (h >= 1 && w >= 1) : (h >= kMinSide && w >= kMinSide);
}

inline bool make_plan(int N, int h, int w, int resize, Plan &p) {
    if (!shape_ok(N, h, w, resize)) return false;
    memset(&p, 0, sizeof(p));
    Walk wk{nullptr, nullptr, p, N, nullptr};
    if (wk.run(nullptr, h, w, resize ? kSide : h, resize ? kSide : w, resize, 0, nullptr) != HL_OK) return false;
    size_t off = 0;
    for (int s = 0; s < kSlots; ++s) {
        p.off[s] = off;
        off += p.size[s];
    }
    p.bytes = off;
    return true;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_fid_layer(int i, char *name, int name_bytes, int *desc) {
    HL_REQUIRE(i >= 0 && i < kLayers && name && name_bytes > 0 && desc, "hl_fid_layer: row %d of %d, or a NULL result", i, kLayers);
    const Layer &l = table().row[i];
    snprintf(name, (size_t)name_bytes, "%s", l.name);
    const int d[8] = {l.cin, l.cout, l.kh, l.kw, l.sh, l.sw, l.ph, l.pw};
    memcpy(desc, d, sizeof(d));
    return HL_OK;
}

size_t hl_fid_workspace_bytes(int N, int h, int w, int resize) {
    Plan p;
    return make_plan(N, h, w, resize, p) ? p.bytes : 0;
}

int hl_fid_block_shape(int N, int h, int w, int resize, int k, size_t *offset_bytes, int *hk, int *wk, int *channels) {
    Plan p;
    HL_REQUIRE(make_plan(N, h, w, resize, p), "hl_fid_block_shape: bad shape (%d images of %d x %d; 1..%d images, sides up to %d, at least %d without resize)",
               N, h, w, kMaxImages, kMaxSide, kMinSide);
    HL_REQUIRE(k >= 0 && k < 4 && offset_bytes && hk && wk && channels, "hl_fid_block_shape: block %d of 4, or a NULL result", k);
    const int slot[4] = {kB0, kB1, kB2, kB3};
    *offset_bytes = p.off[slot[k]];
    *hk = p.bh[k];
    *wk = p.bw[k];
    *channels = p.bc[k];
    return HL_OK;
}

int hl_fid_features(const hl_fid_params *params, const float *in, int N, int h, int w, int resize, int normalize, float *out, void *workspace,
                    size_t workspace_bytes, void *stream) {
    Plan p;
    HL_REQUIRE(params && in, "hl_fid_features: NULL argument");
    for (int l = 0; l < kLayers; ++l) HL_REQUIRE(params->conv_w[l] && params->conv_b[l], "hl_fid_features: layer %d has no weights", l);
    HL_REQUIRE(make_plan(N, h, w, resize, p), "hl_fid_features: bad shape (%d images of %d x %d; 1..%d images, sides up to %d, at least %d without resize)", N,
               h, w, kMaxImages, kMaxSide, kMinSide);
    HL_REQUIRE(workspace && workspace_bytes >= p.bytes, "hl_fid_features: workspace too small (%zu bytes, need %zu)", workspace_bytes, p.bytes);
    HL_REQUIRE(aligned16({workspace, in, out}), "hl_fid_features: pointers must be 16-byte aligned");
    Walk wk{params, static_cast<char *>(workspace), p, N, (hipStream_t)stream};
    return wk.run(in, h, w, resize ? kSide : h, resize ? kSide : w, resize, normalize, out);
}

int hl_fid_moments_update(void *state, const float *features, int n, void *stream) {
    HL_REQUIRE(state && features && n >= 1, "hl_fid_moments_update: NULL argument or no features (%d)", n);
    double *S = static_cast<double *>(state), *s = S + (size_t)kD * kD;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fid_moments_s, dim3(kD / kThreads), dim3(kThreads), 0, st, features, n, s);
    int rc = check_launch("k_fid_moments_s");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_fid_moments_S, dim3(kMTiles * (kMTiles + 1) / 2), dim3(kThreads), 0, st, features, n, S);
    return check_launch("k_fid_moments_S");
}

int hl_fid_moments_finalize(const void *state, int64_t count, double *mu, double *sigma, void *stream) {
    HL_REQUIRE(state && mu && sigma, "hl_fid_moments_finalize: NULL argument");
    HL_REQUIRE(count >= 2, "hl_fid_moments_finalize: a covariance needs at least 2 images, got %lld", (long long)count);
    const double *S = static_cast<const double *>(state), *s = S + (size_t)kD * kD;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fid_mu, dim3(kD / kThreads), dim3(kThreads), 0, st, s, (double)count, mu);
    int rc = check_launch("k_fid_mu");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_fid_finalize, dim3(kD / kThreads, kD), dim3(kThreads), 0, st, S, mu, (double)count, sigma);
    return check_launch("k_fid_finalize");
}

}  // extern "C"
