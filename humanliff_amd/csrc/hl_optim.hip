// The tail of a diffusion training step in one pass, MI355X (gfx950), fp32 parameters: the gradient's sum of squares (grad_norm of
// train_util._log_grad_norm), clip_grad_value_, AdamW and update_ema for up to four rates (human_diffusion/improved_diffusion/train_util.py
// optimize_normal).  One launch walks a multi-tensor table that the host packs once per parameter list (hl_adamw_table_pack) and keeps on
// the device; a second, one-workgroup launch sums the per-chunk partials into one fp64 scalar.
//
// Work split: every tensor is cut into chunks of HL_ADAMW_CHUNK elements - a size that does not depend on the grid - and one workgroup
// owns one chunk.  Inside a chunk every element has a fixed thread and a fixed position in that thread's fp64 sum, and the workgroup adds
// the 256 thread sums in a fixed tree: the partials, and so the norm, are the same bits run to run.  No float atomics.
//
// Per element, in this order (torch 2.x multi-tensor AdamW; fmaf where torch's device kernels compute `a + s * b`; the library builds
// with -ffp-contract=off, so there is no other fma):
//   acc += (double)g * g                                       the UNCLIPPED gradient
//   g = clamp(g, -clip, clip)   (clip > 0 only; NaN stays NaN)  clip_grad_value_
//   p = p * wd_scale            (wd != 0 only)                  _foreach_mul_(params, 1 - lr * wd)
//   m = lerp(m, g, 1 - beta1)                                   _foreach_lerp_
//   v = fma(1 - beta2, g * g, v * beta2)                        _foreach_mul_(v, beta2); _foreach_addcmul_(v, g, g, 1 - beta2)
//   p = fma(-lr / bc1, m / (sqrt(v) / sqrt(bc2) + eps), p)      _foreach_sqrt / _foreach_div_ / _foreach_add_ / _foreach_addcdiv_
//   e_k = fma(1 - r_k, p, e_k * r_k)                            update_ema: targ.mul_(r).add_(src, alpha=1 - r)
// The clipped gradient is NOT written back: .grad keeps the unclipped values (nothing in the training loop reads it after the step).
// A tensor without a gradient (g == NULL) gets its EMA updates only, as torch's optimizers skip it and update_ema does not.
#include "hl_adam.h"

#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = kOptThreads;
constexpr int64_t kChunk = HL_ADAMW_CHUNK;                 // elements per workgroup
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is whole float4 rows of the workgroup");
static_assert(kThreads == kReduceThreads, "block_sum / strided_sum reduce a workgroup of kReduceThreads");

struct OptTensor {            // 80 bytes, the table's first part (one per tensor)
    float *p;
    const float *g;           // NULL: no gradient this step (EMA only)
    float *m, *v;
    float *e[4];
    int64_t n;
    int32_t vec;              // every pointer shares one 16-B phase: the float4 path is used
    int32_t phase;            // (address of p / 4) mod 4: element i is 16-B aligned when (i + phase) % 4 == 0
};
struct OptChunk {             // 16 bytes, the table's second part (one per chunk)
    int32_t tensor;
    int32_t pad;
    int64_t start;
};

struct Coef {
    AdamCoef adam;
    float clip, wd_scale;
    float r[4], rc[4];
    int use_wd;
};

__device__ __forceinline__ void adam1(float g, float &p, float &m, float &v, const Coef &c) {
    if (c.clip > 0.f) g = g < -c.clip ? -c.clip : (g > c.clip ? c.clip : g);   // (comparisons with NaN are false: NaN passes through)
    if (c.use_wd) p = p * c.wd_scale;
    adam_moments(g, p, m, v, c.adam);
}

template <int NE>
__device__ __forceinline__ void ema1(float p, float *e, const Coef &c) {
#pragma unroll
    for (int k = 0; k < NE; ++k) e[k] = fmaf(c.rc[k], p, e[k] * c.r[k]);
}

// one element at index i of tensor t (head / tail / unaligned tensors)
template <int NE>
__device__ __forceinline__ double elem(const OptTensor &t, int64_t i, const Coef &c) {
    float p = t.p[i];
    double sq = 0.0;
    if (t.g) {
        const float g = t.g[i];
        sq = (double)g * (double)g;
        float m = t.m[i], v = t.v[i];
        adam1(g, p, m, v, c);
        t.m[i] = m;
        t.v[i] = v;
        t.p[i] = p;
    }
    float e[NE > 0 ? NE : 1];
#pragma unroll
    for (int k = 0; k < NE; ++k) e[k] = t.e[k][i];
    ema1<NE>(p, e, c);
#pragma unroll
    for (int k = 0; k < NE; ++k) t.e[k][i] = e[k];
    return sq;
}

// four elements at the 16-B-aligned index i
template <int NE>
__device__ __forceinline__ double quad(const OptTensor &t, int64_t i, const Coef &c) {
    f32x4 p = ld4(t.p + i);
    double sq = 0.0;
    if (t.g) {
        const f32x4 g = ld4(t.g + i);
        f32x4 m = ld4(t.m + i), v = ld4(t.v + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = p[j], mj = m[j], vj = v[j];
            sq += (double)g[j] * (double)g[j];
            adam1(g[j], pj, mj, vj, c);
            p[j] = pj;
            m[j] = mj;
            v[j] = vj;
        }
        st4(t.m + i, m);
        st4(t.v + i, v);
        st4(t.p + i, p);
    }
    if (NE > 0) {
        f32x4 e[NE > 0 ? NE : 1];
#pragma unroll
        for (int k = 0; k < NE; ++k) e[k] = ld4(t.e[k] + i);
#pragma unroll
        for (int k = 0; k < NE; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) e[k][j] = fmaf(c.rc[k], p[j], e[k][j] * c.r[k]);
#pragma unroll
        for (int k = 0; k < NE; ++k) st4(t.e[k] + i, e[k]);
    }
    return sq;
}

// grid (nchunks): workgroup b owns chunk b
template <int NE>
__global__ __launch_bounds__(kThreads) void k_adamw_ema(const OptTensor *__restrict__ tens, const OptChunk *__restrict__ chunks, Coef c,
                                                        double *__restrict__ partial) {
    __shared__ double sh[kThreads];
    const OptChunk ch = chunks[blockIdx.x];
    const OptTensor t = tens[ch.tensor];
    const int64_t s = ch.start, e = s + kChunk < t.n ? s + kChunk : t.n;
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (t.vec) {
        // [s, a): scalar head, [a, b): float4 rows, [b, e): scalar tail (each at most 3 elements)
        int64_t a = s + ((4 - ((s + t.phase) & 3)) & 3);
        if (a > e) a = e;
        const int64_t b = a + ((e - a) & ~(int64_t)3);
        if (tid < a - s) acc += elem<NE>(t, s + tid, c);
        const int64_t nq = (b - a) >> 2;
        for (int64_t q = tid; q < nq; q += kThreads) acc += quad<NE>(t, a + 4 * q, c);
        if (tid < e - b) acc += elem<NE>(t, b + tid, c);
    } else {
        for (int64_t i = s + tid; i < e; i += kThreads) acc += elem<NE>(t, i, c);
    }
    const double tot = block_sum(acc, sh);
    if (tid == 0) partial[blockIdx.x] = tot;
}

// one workgroup: out = sum of n partials (strided_sum's order)
__global__ __launch_bounds__(kThreads) void k_sum_partials(const double *__restrict__ partial, int64_t n, double *__restrict__ out) {
    __shared__ double sh[kThreads];
    const double tot = strided_sum(partial, n, 1, sh);
    if (threadIdx.x == 0) out[0] = tot;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int64_t hl_adamw_chunks(const int64_t *numel, int ntensors) {
    if (!numel || ntensors <= 0) return -1;
    int64_t nc = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (numel[i] <= 0) return -1;
        nc += (numel[i] + kChunk - 1) / kChunk;
    }
    return nc;
}

size_t hl_adamw_table_bytes(int ntensors, int64_t nchunks) {
    return (size_t)ntensors * sizeof(OptTensor) + (size_t)nchunks * sizeof(OptChunk);
}

int hl_adamw_table_pack(int ntensors, const int64_t *numel, void *const *ptrs, int n_ema, void *host_table, size_t table_bytes) {
    HL_REQUIRE(ntensors > 0 && numel && ptrs && host_table && n_ema >= 0 && n_ema <= 4, "hl_adamw_table_pack: bad argument "
               "(%d tensors, %d EMA rates: at most 4)", ntensors, n_ema);
    const int64_t nc = hl_adamw_chunks(numel, ntensors);
    HL_REQUIRE(nc > 0 && nc < (1L << 31), "hl_adamw_table_pack: empty tensor or too many chunks");
    HL_REQUIRE(table_bytes >= hl_adamw_table_bytes(ntensors, nc), "hl_adamw_table_pack: table buffer too small (%zu bytes, need %zu)",
               table_bytes, hl_adamw_table_bytes(ntensors, nc));
    OptTensor *T = static_cast<OptTensor *>(host_table);
    OptChunk *Ch = reinterpret_cast<OptChunk *>(T + ntensors);
    int64_t c = 0;
    for (int i = 0; i < ntensors; ++i) {
        void *const *q = ptrs + 8 * (size_t)i;
        OptTensor t{};
        t.p = static_cast<float *>(q[0]);
        t.g = static_cast<const float *>(q[1]);
        t.m = static_cast<float *>(q[2]);
        t.v = static_cast<float *>(q[3]);
        HL_REQUIRE(t.p && (!t.g || (t.m && t.v)), "hl_adamw_table_pack: tensor %d: NULL parameter, or a gradient without moments", i);
        for (int k = 0; k < 4; ++k) t.e[k] = k < n_ema ? static_cast<float *>(q[4 + k]) : nullptr;
        for (int k = 0; k < n_ema; ++k) HL_REQUIRE(t.e[k], "hl_adamw_table_pack: tensor %d: NULL EMA target %d", i, k);
        t.n = numel[i];
        // float4 path when every pointer the tensor uses sits at the same offset from a 16-B boundary (all of them fp32-aligned)
        const uintptr_t ph = (uintptr_t)t.p & 15;
        bool vec = (ph & 3) == 0;
        const void *all[8] = {t.g, t.m, t.v, t.e[0], t.e[1], t.e[2], t.e[3]};
        for (int k = 0; k < 7; ++k)
            if (all[k] && ((uintptr_t)all[k] & 15) != ph) vec = false;
        t.vec = vec ? 1 : 0;
        t.phase = vec ? (int32_t)(ph >> 2) : 0;
        T[i] = t;
        for (int64_t s = 0; s < t.n; s += kChunk) Ch[c++] = OptChunk{i, 0, s};
    }
    return HL_OK;
}

size_t hl_adamw_scratch_bytes(int64_t nchunks) { return nchunks > 0 ? (size_t)nchunks * sizeof(double) : 0; }

int hl_adamw_step(const void *table, int ntensors, int64_t nchunks, int n_ema, const float *ema_rates, float clip, float wd_scale,
                  float one_minus_beta1, float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float neg_step_size,
                  void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(table && ntensors > 0 && nchunks > 0 && nchunks < (1L << 31) && n_ema >= 0 && n_ema <= 4 && (n_ema == 0 || ema_rates),
               "hl_adamw_step: bad argument (%d tensors, %lld chunks, %d EMA rates)", ntensors, (long long)nchunks, n_ema);
    HL_REQUIRE(scratch && scratch_bytes >= hl_adamw_scratch_bytes(nchunks), "hl_adamw_step: scratch too small (%zu bytes, need %zu)",
               scratch_bytes, hl_adamw_scratch_bytes(nchunks));
    Coef c{};
    c.clip = clip;
    c.wd_scale = wd_scale;
    c.use_wd = wd_scale != 1.f;
    c.adam = adam_coef(one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, neg_step_size);
    for (int k = 0; k < n_ema; ++k) {
        c.r[k] = ema_rates[2 * k];
        c.rc[k] = ema_rates[2 * k + 1];
    }
    const OptTensor *T = static_cast<const OptTensor *>(table);
    const OptChunk *Ch = reinterpret_cast<const OptChunk *>(T + ntensors);
    double *partial = static_cast<double *>(scratch);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nchunks), block(kThreads);
    switch (n_ema) {
        case 0: hipLaunchKernelGGL(k_adamw_ema<0>, grid, block, 0, st, T, Ch, c, partial); break;
        case 1: hipLaunchKernelGGL(k_adamw_ema<1>, grid, block, 0, st, T, Ch, c, partial); break;
        case 2: hipLaunchKernelGGL(k_adamw_ema<2>, grid, block, 0, st, T, Ch, c, partial); break;
        case 3: hipLaunchKernelGGL(k_adamw_ema<3>, grid, block, 0, st, T, Ch, c, partial); break;
        default: hipLaunchKernelGGL(k_adamw_ema<4>, grid, block, 0, st, T, Ch, c, partial); break;
    }
    return check_launch("k_adamw_ema");
}

int hl_adamw_sum_partials(const void *scratch, int64_t n, double *out, void *stream) {
    HL_REQUIRE(scratch && out && n > 0, "hl_adamw_sum_partials: bad argument (n %lld)", (long long)n);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, static_cast<const double *>(scratch), n, out);
    return check_launch("k_sum_partials");
}

}  // extern "C"
