// Training kernels of the two UNet variants the base training path (hl_unet_train.hip) does not cover, MI355X (gfx950), fp32:
//
//   use_3d_aware=True         the ResBlock's tri-plane aggregation (human_diffusion/improved_diffusion/unet.py:203-215), forward + backward
//   cond_type=cross_attention the SpatialTransformer's LayerNorm (nn.LayerNorm, spatial_transformer.py:128-134) and GEGLU (:37-44), forward +
//                             backward, and its GroupNorm with eps 1e-6 (:66-67) on the training GroupNorm's statistics / apply kernels
//
// Every kernel here is enqueue-only (no host syncs, no allocations: scratch comes from the caller) and sums in a fixed order without
// float atomics, so a training step gives the same bits run to run.  Contracts: include/humanliff_hip.h; the autograd.Functions that use
// them: humanliff_amd/improved_diffusion/unet_train.py.
#include "hl_reduce.h"
#include "hl_unet_kernels.h"

namespace hl {
namespace {

__device__ __forceinline__ float sigm(float u) { return 1.f / (1.f + expf(-u)); }
__device__ __forceinline__ float silu_p(float u) { return u * sigm(u); }
__device__ __forceinline__ float dsilu(float u) {                  // d silu / du = s (1 + u (1 - s))
    const float s = sigm(u);
    return s * (1.f + u * (1.f - s));
}
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// ---------------------------------------------------------------------------------------------
// tri-plane aggregation (unet.py:208-214), g / dg (N, H, 3W, C) with the planes xy | xz | zy side by side, H == W
// ---------------------------------------------------------------------------------------------
// out (N, H, 3W, 3C) = silu(cat[g_p, m1_p, m2_p]) per plane p with
//   p = 0 (xy): m1 = rowmean(1)[y], m2 = colmean(2)[x]
//   p = 1 (xz): m1 = rowmean(0)[y], m2 = rowmean(2)[y]
//   p = 2 (zy): m1 = colmean(0)[x], m2 = colmean(1)[x]
// rowmean(q)[y] = mean over the W columns of row y of plane q, colmean(q)[x] = mean over the H rows of column x.
// Every mean is read by exactly one (plane, slot): rowmean(q) by RP[q] / RS[q], colmean(q) by CP[q] / CS[q] - the backward sums that
// slot's gradient along the broadcast axis and hands it back to plane q.
__constant__ int RP[3] = {1, 0, 1}, RS[3] = {1, 1, 2}, CP[3] = {2, 2, 0}, CS[3] = {1, 2, 2};

// grid (H + W, 3, N), 64 threads over channel quads.  item < H: row item of plane q -> rm[n][q][item][c]; else column item - H -> cm.
// fwd (src = g, slot 0 of plane q itself, pitch C): the means.  bwd (src = dout, the reading plane's slot, pitch 3C): the gradient sums
// times silu'(mean) / count, which is what plane q receives along the broadcast axis.
template <bool BWD>
__global__ __launch_bounds__(64) void k_plane_reduce(const float *__restrict__ src, int H, int W, int C, const float *__restrict__ rmean,
                                                     const float *__restrict__ cmean, float *__restrict__ rm, float *__restrict__ cm) {
    const int item = blockIdx.x, q = blockIdx.y, n = blockIdx.z, cq = C >> 2;
    const bool row = item < H;
    const int pl = BWD ? (row ? RP[q] : CP[q]) : q, slot = BWD ? (row ? RS[q] : CS[q]) : 0;
    const long pitch = BWD ? 3L * C : (long)C;
    const long img = (long)n * H * 3 * W;
    const int cnt = row ? W : H;
    for (int c4 = threadIdx.x; c4 < cq; c4 += 64) {
        const float *p = src + slot * C + c4 * 4;
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row) {
            const float *r = p + (img + (long)item * 3 * W + (long)pl * W) * pitch;
#pragma unroll 8
            for (int x = 0; x < W; ++x) a += ld4(r + (long)x * pitch);
        } else {
            const float *r = p + (img + (long)pl * W + (item - H)) * pitch;
#pragma unroll 8
            for (int y = 0; y < H; ++y) a += ld4(r + (long)y * 3 * W * pitch);
        }
        const long o = ((((long)n * 3 + q) * (row ? H : W)) + (row ? item : item - H)) * C + c4 * 4;
        f32x4 v = a / (float)cnt;
        if (BWD) {
            const f32x4 m = ld4((row ? rmean : cmean) + o);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] *= dsilu(m[i]);
        }
        st4((row ? rm : cm) + o, v);
    }
}

__global__ void k_agg_fwd(const float *__restrict__ g, int N, int H, int W, int C, const float *__restrict__ rmean, const float *__restrict__ cmean,
                          float *__restrict__ out) {
    const int cq = C >> 2;
    const long n4 = (long)N * H * 3 * W * cq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / cq;
        const int c = (int)(i - pix * cq) * 4;
        const int X = (int)(pix % (3 * W));
        const long ny = pix / (3 * W);
        const int y = (int)(ny % H);
        const long n = ny / H;
        const int pl = X / W, x = X - pl * W;
        auto rmq = [&](int q) { return ld4(rmean + ((n * 3 + q) * H + y) * C + c); };
        auto cmq = [&](int q) { return ld4(cmean + ((n * 3 + q) * W + x) * C + c); };
        const f32x4 v = ld4(g + pix * C + c);
        const f32x4 m1 = pl == 0 ? rmq(1) : (pl == 1 ? rmq(0) : cmq(0));
        const f32x4 m2 = pl == 0 ? cmq(2) : (pl == 1 ? rmq(2) : cmq(1));
        f32x4 o0, o1, o2;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o0[j] = silu_p(v[j]); o1[j] = silu_p(m1[j]); o2[j] = silu_p(m2[j]); }
        float *o = out + pix * 3 * C + c;
        st4(o, o0);
        st4(o + C, o1);
        st4(o + 2 * C, o2);
    }
}

// dg = dout[own slot] * silu'(g) + rg[n][p][y] + cg[n][p][x]
__global__ void k_agg_bwd_apply(const float *__restrict__ dout, const float *__restrict__ g, int N, int H, int W, int C, const float *__restrict__ rg,
                                const float *__restrict__ cg, float *__restrict__ dg) {
    const int cq = C >> 2;
    const long n4 = (long)N * H * 3 * W * cq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / cq;
        const int c = (int)(i - pix * cq) * 4;
        const int X = (int)(pix % (3 * W));
        const long ny = pix / (3 * W);
        const int y = (int)(ny % H);
        const long n = ny / H;
        const int pl = X / W, x = X - pl * W;
        const f32x4 v = ld4(g + pix * C + c), d = ld4(dout + pix * 3 * C + c);
        const f32x4 r = ld4(rg + ((n * 3 + pl) * H + y) * C + c), s = ld4(cg + ((n * 3 + pl) * W + x) * C + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (d[j] * dsilu(v[j]) + r[j]) + s[j];
        st4(dg + pix * C + c, o);
    }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the C channels of every pixel (nn.LayerNorm(C)), x / y / dy / dx dense (npix, C)
// ---------------------------------------------------------------------------------------------
// forward: one wave per pixel, the arithmetic of the inference kernel (k_layernorm: two passes, fp32); stat[p] = (mean, rstd)
__global__ __launch_bounds__(256) void k_ln_fwd(const float *__restrict__ x, long npix, int C, const float *__restrict__ gamma,
                                                const float *__restrict__ beta, float eps, float *__restrict__ y, float *__restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= npix) return;
    const float *xp = x + pix * C;
    float sm = 0.f;
    for (int c = lane; c < C; c += 64) sm += xp[c];
    sm = wave_xor_sum(sm);
    const float mean = sm / (float)C;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) { const float dv = xp[c] - mean; sq = fmaf(dv, dv, sq); }
    sq = wave_xor_sum(sq);
    const float rstd = 1.f / sqrtf(sq / (float)C + eps);
    for (int c = lane; c < C; c += 64) y[pix * C + c] = fmaf((xp[c] - mean) * rstd, gamma[c], beta[c]);
    if (lane == 0) { stat[pix * 2] = mean; stat[pix * 2 + 1] = rstd; }
}

// dx = rstd * (gd - mean_c(gd) - xh * mean_c(gd * xh)),  gd = dy * gamma, xh = (x - mean) * rstd;  one wave per pixel
__global__ __launch_bounds__(256) void k_ln_bwd_dx(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ stat,
                                                   long npix, int C, const float *__restrict__ gamma, float *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= npix) return;
    const float mean = stat[pix * 2], rstd = stat[pix * 2 + 1];
    const float *xp = x + pix * C, *dp = dy + pix * C;
    float a = 0.f, b = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float gd = dp[c] * gamma[c], xh = (xp[c] - mean) * rstd;
        a += gd;
        b = fmaf(gd, xh, b);
    }
    a = wave_xor_sum(a);
    b = wave_xor_sum(b);
    const float ma = a / (float)C, mb = b / (float)C;
    for (int c = lane; c < C; c += 64) {
        const float gd = dp[c] * gamma[c], xh = (xp[c] - mean) * rstd;
        dx[pix * C + c] = rstd * ((gd - ma) - xh * mb);
    }
}

// d gamma / d beta: column sums of dy * xh and dy over the pixels.  grid (chunks); a thread owns a channel quad of one of the k pixel rows
// of the workgroup; the rows meet in LDS in row order and part[chunk] = [dgamma(C) | dbeta(C)]; k_ln_bwd_fin adds the chunks in order.
__global__ void k_ln_bwd_reduce(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ stat, long npix, int C,
                                int nchunks, float *__restrict__ part) {
    const int cq = C >> 2, k = blockDim.x / cq;
    const int c4 = threadIdx.x % cq, prow = threadIdx.x / cq;
    extern __shared__ float sh[];                                   // [k][2C]
    const long per = (npix + nchunks - 1) / nchunks;
    const long p0 = (long)blockIdx.x * per, p1 = min(npix, p0 + per);
    f32x4 sg = f32x4{0.f, 0.f, 0.f, 0.f}, sb = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long p = p0 + prow; p < p1; p += k) {
        const float mean = stat[p * 2], rstd = stat[p * 2 + 1];
        const f32x4 xv = ld4(x + p * C + c4 * 4), dv = ld4(dy + p * C + c4 * 4);
        sg += dv * ((xv - mean) * rstd);
        sb += dv;
    }
    st4(sh + prow * 2 * C + c4 * 4, sg);
    st4(sh + prow * 2 * C + C + c4 * 4, sb);
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += blockDim.x) {
        float v = sh[e];
        for (int r = 1; r < k; ++r) v += sh[r * 2 * C + e];
        part[(long)blockIdx.x * 2 * C + e] = v;
    }
}

__global__ __launch_bounds__(256) void k_ln_bwd_fin(const float *__restrict__ part, int nchunks, int C, float *__restrict__ dgamma,
                                                    float *__restrict__ dbeta) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * C) return;
    float v = 0.f;
    for (int c = 0; c < nchunks; ++c) v += part[(long)c * 2 * C + e];
    if (e < C) dgamma[e] = v;
    else dbeta[e - C] = v;
}

// ---------------------------------------------------------------------------------------------
// GEGLU (spatial_transformer.py:37-44): in (npix, 2F) = [u | gate] -> out (npix, F) = u * gelu(gate), exact (erf) GELU
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_cdf(float g) { return 0.5f * (1.f + erff(g * 0.70710678118654752f)); }

__global__ void k_geglu_fwd(const float *__restrict__ in, long npix, int F, float *__restrict__ out) {
    const long n = npix * F;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / F;
        const int f = (int)(i - pix * F);
        const float a = in[pix * 2 * F + f], g = in[pix * 2 * F + F + f];
        out[i] = a * (g * gelu_cdf(g));
    }
}

// du = d * gelu(g),  dgate = d * u * (Phi(g) + g * phi(g))
__global__ void k_geglu_bwd(const float *__restrict__ in, const float *__restrict__ dout, long npix, int F, float *__restrict__ din) {
    const long n = npix * F;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / F;
        const int f = (int)(i - pix * F);
        const float a = in[pix * 2 * F + f], g = in[pix * 2 * F + F + f], d = dout[i];
        const float cdf = gelu_cdf(g), pdf = 0.39894228040143268f * expf(-0.5f * g * g);
        din[pix * 2 * F + f] = d * (g * cdf);
        din[pix * 2 * F + F + f] = d * a * (cdf + g * pdf);
    }
}

unsigned grid_for(long work) {
    long g = (work + 255) / 256;
    return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

int ln_chunks(long npix, int C) {
    int k = 256 / (C / 4);
    if (k < 1) k = 1;
    long ch = npix / ((long)k * 16);
    return (int)(ch < 1 ? 1 : (ch > 256 ? 256 : ch));
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_triplane_agg_forward(const float *g, int N, int H, int W, int C, float *rmean, float *cmean, float *out, void *stream) {
    HL_REQUIRE(g && rmean && cmean && out && N > 0 && H > 0 && H == W && C > 0 && C % 4 == 0, "hl_triplane_agg_forward: bad argument "
               "(N %d, H %d, W %d, C %d: the planes are square, C %% 4 == 0)", N, H, W, C);
    HL_REQUIRE((long)N * H * 3 * W * 3 * C < (1L << 31), "hl_triplane_agg_forward: tensor too large");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_plane_reduce<false>, dim3(H + W, 3, N), dim3(64), 0, st, g, H, W, C, nullptr, nullptr, rmean, cmean);
    int rc = check_launch("k_plane_reduce");
    if (rc) return rc;
    hipLaunchKernelGGL(k_agg_fwd, dim3(grid_for((long)N * H * 3 * W * (C / 4))), dim3(256), 0, st, g, N, H, W, C, rmean, cmean, out);
    return check_launch("k_agg_fwd");
}

// the row and column sums of every plane's gradient: rg (N,3,H,C) | cg (N,3,W,C)
size_t hl_triplane_agg_backward_scratch_bytes(int N, int H, int W, int C) { return (size_t)N * 3 * (H + W) * C * sizeof(float); }

int hl_triplane_agg_backward(const float *dout, const float *g, const float *rmean, const float *cmean, int N, int H, int W, int C, float *dg,
                             void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(dout && g && rmean && cmean && dg && N > 0 && H > 0 && H == W && C > 0 && C % 4 == 0, "hl_triplane_agg_backward: bad argument "
               "(N %d, H %d, W %d, C %d)", N, H, W, C);
    HL_REQUIRE((long)N * H * 3 * W * 3 * C < (1L << 31), "hl_triplane_agg_backward: tensor too large");
    const size_t need = hl_triplane_agg_backward_scratch_bytes(N, H, W, C);
    HL_REQUIRE(scratch && scratch_bytes >= need, "hl_triplane_agg_backward: scratch too small (%zu bytes, hl_triplane_agg_backward_scratch_bytes says %zu)",
               scratch_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    float *rg = static_cast<float *>(scratch), *cg = rg + (size_t)N * 3 * H * C;
    hipLaunchKernelGGL(k_plane_reduce<true>, dim3(H + W, 3, N), dim3(64), 0, st, dout, H, W, C, rmean, cmean, rg, cg);
    int rc = check_launch("k_plane_reduce");
    if (rc) return rc;
    hipLaunchKernelGGL(k_agg_bwd_apply, dim3(grid_for((long)N * H * 3 * W * (C / 4))), dim3(256), 0, st, dout, g, N, H, W, C, rg, cg, dg);
    return check_launch("k_agg_bwd_apply");
}

int hl_layernorm_train_forward(const float *x, int64_t npix, int C, const float *gamma, const float *beta, float eps, float *y, float *stat,
                               void *stream) {
    HL_REQUIRE(x && gamma && beta && y && stat && npix > 0 && C > 0, "hl_layernorm_train_forward: bad argument");
    hipLaunchKernelGGL(k_ln_fwd, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long)npix, C, gamma, beta, eps, y, stat);
    return check_launch("k_ln_fwd");
}

size_t hl_layernorm_backward_scratch_bytes(int64_t npix, int C) { return (size_t)ln_chunks(npix, C) * 2 * C * sizeof(float); }

int hl_layernorm_train_backward(const float *x, const float *dy, const float *stat, int64_t npix, int C, const float *gamma, float *dx,
                                float *dgamma, float *dbeta, void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(x && dy && stat && gamma && dgamma && dbeta && npix > 0 && C > 0 && C % 4 == 0 && C <= 1024,
               "hl_layernorm_train_backward: bad argument (C %d: a multiple of 4, at most 1024)", C);
    const size_t need = hl_layernorm_backward_scratch_bytes(npix, C);
    HL_REQUIRE(scratch && scratch_bytes >= need, "hl_layernorm_train_backward: scratch too small (%zu bytes, need %zu)", scratch_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    if (dx) {
        hipLaunchKernelGGL(k_ln_bwd_dx, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, st, x, dy, stat, (long)npix, C, gamma, dx);
        int rc = check_launch("k_ln_bwd_dx");
        if (rc) return rc;
    }
    const int cq = C / 4, chunks = ln_chunks(npix, C);
    int k = 256 / cq;
    if (k < 1) k = 1;
    hipLaunchKernelGGL(k_ln_bwd_reduce, dim3(chunks), dim3(cq * k), (size_t)k * 2 * C * sizeof(float), st, x, dy, stat, (long)npix, C, chunks,
                       static_cast<float *>(scratch));
    int rc = check_launch("k_ln_bwd_reduce");
    if (rc) return rc;
    hipLaunchKernelGGL(k_ln_bwd_fin, dim3((2 * C + 255) / 256), dim3(256), 0, st, static_cast<const float *>(scratch), chunks, C, dgamma, dbeta);
    return check_launch("k_ln_bwd_fin");
}

int hl_geglu_forward(const float *in, int64_t npix, int F, float *out, void *stream) {
    HL_REQUIRE(in && out && npix > 0 && F > 0, "hl_geglu_forward: bad argument");
    hipLaunchKernelGGL(k_geglu_fwd, dim3(grid_for((long)npix * F)), dim3(256), 0, (hipStream_t)stream, in, (long)npix, F, out);
    return check_launch("k_geglu_fwd");
}

int hl_geglu_backward(const float *in, const float *dout, int64_t npix, int F, float *din, void *stream) {
    HL_REQUIRE(in && dout && din && npix > 0 && F > 0, "hl_geglu_backward: bad argument");
    hipLaunchKernelGGL(k_geglu_bwd, dim3(grid_for((long)npix * F)), dim3(256), 0, (hipStream_t)stream, in, dout, (long)npix, F, din);
    return check_launch("k_geglu_bwd");
}

int hl_groupnorm_train_forward_eps(const float *x, int N, int H, int W, int C, const float *gamma, const float *beta, const float *scale_shift,
                                   int silu, float eps, float *coefA, float *coefB, float *gstat, float *y, void *scratch, size_t scratch_bytes,
                                   void *stream) {
    HL_REQUIRE(x && gamma && beta && coefA && coefB && gstat && y && eps > 0.f, "hl_groupnorm_train_forward_eps: bad argument");
    HL_REQUIRE(scratch && scratch_bytes >= hl_groupnorm_scratch_bytes(N), "hl_groupnorm_train_forward_eps: scratch too small (%zu bytes, hl_groupnorm_scratch_bytes says %zu)",
               scratch_bytes, hl_groupnorm_scratch_bytes(N));
    View v; v.p = const_cast<float *>(x); v.N = N; v.H = H; v.W = W; v.C = C; v.pitch = C;
    int rc = groupnorm_coef(v, gamma, beta, scale_shift, 2L * C, coefA, coefB, static_cast<float *>(scratch), (hipStream_t)stream, gstat, eps);
    if (rc) return rc;
    return gn_apply(v, coefA, coefB, silu, y, (hipStream_t)stream);
}

}  // extern "C"
