// The tail of a tri-plane fitting iteration, MI355X (gfx950), fp32 (recon_NeRF/run_nerf_batch.py:256-272 of the reference: the TV / L1
// regularisers on the batch's plane sets, Adam on Renderer.tri_planes, clamp_).  Two streaming, memory-bound kernels in the conventions
// of hl_optim.hip: 16-byte accesses, a work split that does not depend on the grid, fixed-order fp64 partial sums, no float atomics.
//
// k_fit_reg: one pass over the gathered copies x (nplanes = bs * 27 images of H x W).  Every texel owns the pair with its lower and the
//   pair with its right neighbour (where they exist) and adds |x - x_dn|, |x - x_rt| (fp32 differences) and |x| to its thread's three
//   fp64 sums; the workgroup adds its 256 threads in a fixed tree, k_fit_reg_finish adds the workgroups' partials in a fixed order.  The
//   same pass adds the regularisers' gradient to the buffer the render backward filled:
//       g += cx (sign(x - x_dn) - sign(x_up - x)) + cy (sign(x - x_rt) - sign(x_lf - x)) + cl sign(x)
//   with sign(0) = 0 and sign(NaN) = NaN, a missing neighbour contributing nothing, and cx, cy, cl = coef / n rounded to fp32 by the
//   host.  The sign differences are small integers, so the three products are exact and the sum costs three fp32 additions.
//   x is only read and g only written: neighbouring texels never race.
//
// k_fit_adam_planes: Adam over the WHOLE parameter (num_instances x num_layers slices of slice_numel elements) without a dense
//   gradient.  A workgroup owns one HL_FIT_CHUNK-element chunk of one slice, reads the batch's (instance, layer) pairs from DEVICE
//   memory, and forms g = 0 + g_b0 + g_b1 + ... over the entries b that select its slice, in batch order (index_put_(accumulate=True)
//   into zeros with the order fixed).  A slice that nothing selects takes g = 0 and moves p, m, v only.  Per element adam_moments()
//   (hl_adam.h: torch's multi-tensor Adam with weight_decay 0), then p = clamp(p, -1, 1) when asked (NaN stays NaN, like clamp_).
//   Negative indices wrap like torch's; an entry whose pair is out of range selects nothing.
#include "hl_adam.h"

#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = kOptThreads;
constexpr int64_t kChunk = HL_FIT_CHUNK;                   // elements of a slice per workgroup (k_fit_adam_planes)
constexpr int64_t kRegChunk = HL_FIT_REG_CHUNK;            // texels of an image per workgroup (k_fit_reg)
static_assert(kChunk % (4 * kThreads) == 0 && kRegChunk % (4 * kThreads) == 0, "a chunk is whole float4 rows of the workgroup");
static_assert(kThreads == kReduceThreads, "block_sum / strided_sum reduce a workgroup of kReduceThreads");

__device__ __forceinline__ float sgn(float d) { return d != d ? d : (float)((d > 0.f) - (d < 0.f)); }

struct RegCoef {
    float cx, cy, cl;
};

// one texel: its neighbours (and whether they exist), the gradient so far; returns the new gradient
__device__ __forceinline__ float reg1(float x, float up, bool has_up, float dn, bool has_dn, float lf, bool has_lf, float rt, bool has_rt,
                                      float g, const RegCoef &c, double &tvx, double &tvy, double &l1) {
    float dx = 0.f, dy = 0.f;
    if (has_dn) {
        const float d = x - dn;
        tvx += (double)fabsf(d);
        dx = sgn(d);
    }
    if (has_up) dx = dx - sgn(up - x);
    if (has_rt) {
        const float d = x - rt;
        tvy += (double)fabsf(d);
        dy = sgn(d);
    }
    if (has_lf) dy = dy - sgn(lf - x);
    l1 += (double)fabsf(x);
    float t = c.cx * dx;
    t = t + c.cy * dy;
    t = t + c.cl * sgn(x);
    return g + t;
}

// grid (nplanes * chunks per image): workgroup b owns texels [s, e) of image b / cpp
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_fit_reg(const float *__restrict__ planes, float *__restrict__ grad, int H, int W, int cpp,
                                                      RegCoef c, double *__restrict__ partial) {
    __shared__ double sh[kThreads];
    const int HW = H * W;                 // (< 2^31: the host refuses larger images, so texel indices are 32-bit)
    const int64_t img = blockIdx.x / cpp;
    const int s = (int)(blockIdx.x % cpp) * (int)kRegChunk, e = HW - s > (int)kRegChunk ? s + (int)kRegChunk : HW;
    const float *x = planes + img * HW;
    float *g = grad + img * HW;
    const int tid = threadIdx.x;
    double tvx = 0.0, tvy = 0.0, l1 = 0.0;
    if (VEC) {              // W % 4 == 0: a quad lies inside one row
        const int nq = (e - s) >> 2;
        for (int q = tid; q < nq; q += kThreads) {
            const int i = s + 4 * q;
            const int h = (int)((unsigned)i / (unsigned)W), w = i - h * W;
            const bool has_up = h > 0, has_dn = h + 1 < H, has_lf = w > 0, has_rt = w + 4 < W;
            const f32x4 xc = ld4(x + i);
            const f32x4 up = has_up ? ld4(x + i - W) : xc;
            const f32x4 dn = has_dn ? ld4(x + i + W) : xc;
            const float lf = has_lf ? x[i - 1] : 0.f, rt = has_rt ? x[i + 4] : 0.f;
            f32x4 gv = ld4(g + i);
            gv[0] = reg1(xc[0], up[0], has_up, dn[0], has_dn, lf, has_lf, xc[1], true, gv[0], c, tvx, tvy, l1);
            gv[1] = reg1(xc[1], up[1], has_up, dn[1], has_dn, xc[0], true, xc[2], true, gv[1], c, tvx, tvy, l1);
            gv[2] = reg1(xc[2], up[2], has_up, dn[2], has_dn, xc[1], true, xc[3], true, gv[2], c, tvx, tvy, l1);
            gv[3] = reg1(xc[3], up[3], has_up, dn[3], has_dn, xc[2], true, rt, has_rt, gv[3], c, tvx, tvy, l1);
            st4(g + i, gv);
        }
    } else {
        for (int i = s + tid; i < e; i += kThreads) {
            const int h = (int)((unsigned)i / (unsigned)W), w = i - h * W;
            const bool has_up = h > 0, has_dn = h + 1 < H, has_lf = w > 0, has_rt = w + 1 < W;
            const float xc = x[i];
            g[i] = reg1(xc, has_up ? x[i - W] : 0.f, has_up, has_dn ? x[i + W] : 0.f, has_dn, has_lf ? x[i - 1] : 0.f, has_lf,
                        has_rt ? x[i + 1] : 0.f, has_rt, g[i], c, tvx, tvy, l1);
        }
    }
    const double a = block_sum(tvx, sh), b = block_sum(tvy, sh), d = block_sum(l1, sh);
    if (tid == 0) {
        partial[3 * (int64_t)blockIdx.x] = a;
        partial[3 * (int64_t)blockIdx.x + 1] = b;
        partial[3 * (int64_t)blockIdx.x + 2] = d;
    }
}

// one workgroup: out[k] = sum over the n workgroups of partial[3 i + k] (strided_sum's order)
__global__ __launch_bounds__(kThreads) void k_fit_reg_finish(const double *__restrict__ partial, int64_t n, double *__restrict__ out) {
    __shared__ double sh[kThreads];
    for (int k = 0; k < 3; ++k) {
        const double tot = strided_sum(partial + k, n, 3, sh);
        if (threadIdx.x == 0) out[k] = tot;
    }
}

__device__ __forceinline__ float clamp1(float p) { return p < -1.f ? -1.f : (p > 1.f ? 1.f : p); }   // (comparisons with NaN are false)

struct PlanesArgs {
    float *p, *m, *v;
    const float *grad;                    // bs entries of slice_numel elements
    const int64_t *inst, *layer;          // bs each, on the device
    int64_t L;                            // slice_numel
    int bs, NI, NL, cps;                  // cps: chunks per slice
    int clamp;
};

// grid (NI * NL * cps): workgroup b owns elements [s, e) of slice b / cps
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_fit_adam_planes(PlanesArgs a, AdamCoef c) {
    const int64_t slice = blockIdx.x / a.cps;
    const int64_t s = (int64_t)(blockIdx.x % a.cps) * kChunk, e = s + kChunk < a.L ? s + kChunk : a.L;
    // the batch entries that select this slice, bit b = entry b (the same for every thread: scalar loads, a scalar loop below)
    uint64_t sel = 0;
    for (int b = 0; b < a.bs; ++b) {
        int64_t i = a.inst[b], l = a.layer[b];
        if (i < 0) i += a.NI;
        if (l < 0) l += a.NL;
        if (i >= 0 && i < a.NI && l >= 0 && l < a.NL && i * a.NL + l == slice) sel |= (uint64_t)1 << b;
    }
    float *p = a.p + slice * a.L, *m = a.m + slice * a.L, *v = a.v + slice * a.L;
    const int tid = threadIdx.x;
    if (VEC) {
        const int64_t nq = (e - s) >> 2;
        for (int64_t q = tid; q < nq; q += kThreads) {
            const int64_t i = s + 4 * q;
            f32x4 pq = ld4(p + i), mq = ld4(m + i), vq = ld4(v + i);
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            for (uint64_t r = sel; r; r &= r - 1) g = g + ld4(a.grad + (int64_t)__builtin_ctzll(r) * a.L + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pq[j], mj = mq[j], vj = vq[j];
                adam_moments(g[j], pj, mj, vj, c);
                pq[j] = a.clamp ? clamp1(pj) : pj;
                mq[j] = mj;
                vq[j] = vj;
            }
            st4(m + i, mq);
            st4(v + i, vq);
            st4(p + i, pq);
        }
    } else {
        for (int64_t i = s + tid; i < e; i += kThreads) {
            float pj = p[i], mj = m[i], vj = v[i];
            float g = 0.f;
            for (uint64_t r = sel; r; r &= r - 1) g = g + a.grad[(int64_t)__builtin_ctzll(r) * a.L + i];
            adam_moments(g, pj, mj, vj, c);
            p[i] = a.clamp ? clamp1(pj) : pj;
            m[i] = mj;
            v[i] = vj;
        }
    }
}

inline int64_t reg_blocks(int64_t nplanes, int H, int W) {
    if (nplanes <= 0 || H < 2 || W < 2 || (int64_t)H * W > (int64_t)0x7fffffff - kRegChunk) return -1;
    const int64_t cpp = ((int64_t)H * W + kRegChunk - 1) / kRegChunk;
    return nplanes * cpp;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

size_t hl_fit_reg_scratch_bytes(int64_t nplanes, int H, int W) {
    const int64_t nb = reg_blocks(nplanes, H, W);
    return nb > 0 ? (size_t)nb * 3 * sizeof(double) : 0;
}

int hl_fit_reg(const float *planes, float *grad, int64_t nplanes, int H, int W, float cx, float cy, float cl, double *sums, void *scratch,
               size_t scratch_bytes, void *stream) {
    const int64_t nb = reg_blocks(nplanes, H, W);
    HL_REQUIRE(planes && grad && sums && nb > 0 && nb < (1L << 31), "hl_fit_reg: bad argument (%lld images of %d x %d; H, W >= 2)",
               (long long)nplanes, H, W);
    HL_REQUIRE(scratch && scratch_bytes >= hl_fit_reg_scratch_bytes(nplanes, H, W), "hl_fit_reg: scratch too small (%zu bytes, need %zu)",
               scratch_bytes, hl_fit_reg_scratch_bytes(nplanes, H, W));
    const int cpp = (int)(nb / nplanes);
    const RegCoef c{cx, cy, cl};
    double *partial = static_cast<double *>(scratch);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nb), block(kThreads);
    if (W % 4 == 0 && aligned16({planes, grad}))
        hipLaunchKernelGGL(k_fit_reg<true>, grid, block, 0, st, planes, grad, H, W, cpp, c, partial);
    else
        hipLaunchKernelGGL(k_fit_reg<false>, grid, block, 0, st, planes, grad, H, W, cpp, c, partial);
    const int rc = check_launch("k_fit_reg");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_fit_reg_finish, dim3(1), block, 0, st, partial, nb, sums);
    return check_launch("k_fit_reg_finish");
}

int hl_fit_adam_planes(float *param, float *exp_avg, float *exp_avg_sq, const float *grad, const int64_t *instance_idx,
                       const int64_t *layer_idx, int bs, int num_instances, int num_layers, int64_t slice_numel, float one_minus_beta1,
                       float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float neg_step_size, int clamp, void *stream) {
    HL_REQUIRE(param && exp_avg && exp_avg_sq && grad && instance_idx && layer_idx, "hl_fit_adam_planes: NULL argument");
    HL_REQUIRE(bs > 0 && bs <= HL_FIT_MAX_BATCH && num_instances > 0 && num_layers > 0 && slice_numel > 0,
               "hl_fit_adam_planes: bad shape (batch %d: 1..%d, %d instances, %d layers, %lld elements per slice)", bs, HL_FIT_MAX_BATCH,
               num_instances, num_layers, (long long)slice_numel);
    const int64_t cps = (slice_numel + kChunk - 1) / kChunk;
    const int64_t nb = (int64_t)num_instances * num_layers * cps;
    HL_REQUIRE(nb < (1L << 31), "hl_fit_adam_planes: too many chunks (%lld)", (long long)nb);
    const PlanesArgs a{param, exp_avg, exp_avg_sq, grad, instance_idx, layer_idx, slice_numel, bs, num_instances, num_layers, (int)cps,
                       clamp ? 1 : 0};
    const AdamCoef c = adam_coef(one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, neg_step_size);
    const dim3 grid((unsigned)nb), block(kThreads);
    if (slice_numel % 4 == 0 && aligned16({param, exp_avg, exp_avg_sq, grad}))
        hipLaunchKernelGGL(k_fit_adam_planes<true>, grid, block, 0, (hipStream_t)stream, a, c);
    else
        hipLaunchKernelGGL(k_fit_adam_planes<false>, grid, block, 0, (hipStream_t)stream, a, c);
    return check_launch("k_fit_adam_planes");
}

}  // extern "C"
