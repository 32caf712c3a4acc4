// Fused kernels of the likelihood evaluation and the DDIM inversion, MI355X.
//
//   hl_diffusion_q_sample        GaussianDiffusion.q_sample                human_diffusion/improved_diffusion/gaussian_diffusion.py:175-193
//   hl_diffusion_reverse_step    GaussianDiffusion.ddim_reverse_sample     gaussian_diffusion.py:531-567 (everything after the model call)
//   hl_diffusion_vb_terms        one timestep of calc_bpd_loop after the model call: _vb_terms_bpd (:653-687) through p_mean_variance
//                                (:232-326) and q_posterior_mean_variance (:208-230), losses.py normal_kl / discretized_gaussian_log_likelihood,
//                                plus the two MSEs of calc_bpd_loop (:815-835)
//   hl_diffusion_prior_bpd       _prior_bpd (:774-790)
//
// Per-timestep scalars come from the device-resident (T, 16) eval table (layout in include/humanliff_hip.h).  Elementwise arithmetic follows
// the reference's fp32 op order (file built with -ffp-contract=off); exp / log / tanh are the device's, so those terms agree with PyTorch-CPU
// to a few ulp rather than bit for bit.  The per-sample means are accumulated in fp64 in a fixed order - per-workgroup partials into a
// caller-provided scratch, then one fixed-order pass per sample - with no atomics, so repeated calls give bit-identical results.
#include "hl_reduce.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == hl::kReduceThreads, "block_sum reduces a workgroup of kReduceThreads");
constexpr long MAX_BLOCKS = 1024;     // workgroups per sample (the grid-stride loops cover the rest)
constexpr int NCOL = 16;
// eval table columns (include/humanliff_hip.h)
enum { C_R = 0, C_RM1, C_PC1, C_PC2, C_IC1, C_C21, C_MINLOG, C_MAXLOG, C_FIXLOG, C_SA, C_S1MA, C_SAN, C_S1MAN, C_LOG1MA };

// clamp that keeps a NaN (torch.clamp does; fminf / fmaxf would drop it)
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clamp_min(float v, float lo) { return v < lo ? lo : v; }

long blocks_for(long n, bool vec) {
    const long work = vec ? n / 4 : n;
    long g = (work + TPB - 1) / TPB;
    return g > MAX_BLOCKS ? MAX_BLOCKS : g;
}

// ---- q_sample / reverse DDIM step ---------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_q_sample(const float *__restrict__ x0, const float *__restrict__ noise, const float *__restrict__ coef,
                                                   const int64_t *__restrict__ t, float *__restrict__ out, long n, int T) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const bool in_range = tb >= 0 && tb < (int64_t)T;
    const float *c = coef + (in_range ? tb : 0) * NCOL;
    const float poison = in_range ? 0.f : __builtin_nanf("");
    const float sa = c[C_SA] + poison, s1 = c[C_S1MA];
    const long base = (long)b * n;
    if (VEC) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += (long)gridDim.x * blockDim.x) {
            const f32x4 xv = reinterpret_cast<const f32x4 *>(x0 + base)[i];
            const f32x4 nv = reinterpret_cast<const f32x4 *>(noise + base)[i];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = sa * xv[k] + s1 * nv[k];
            reinterpret_cast<f32x4 *>(out + base)[i] = o;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
            out[base + i] = sa * x0[base + i] + s1 * noise[base + i];
    }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_reverse(const float *__restrict__ x, const float *__restrict__ eps, const float *__restrict__ coef,
                                                  const int64_t *__restrict__ t, float *__restrict__ sample, float *__restrict__ x0_out, long n,
                                                  int T, int clip, int x0_given) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const bool in_range = tb >= 0 && tb < (int64_t)T;
    const float *c = coef + (in_range ? tb : 0) * NCOL;
    const float poison = in_range ? 0.f : __builtin_nanf("");
    const float r = c[C_R] + poison, rm1 = c[C_RM1], san = c[C_SAN], s1man = c[C_S1MAN];
    const long base = (long)b * n;
    auto one = [&](float xv, float ev, float &sv, float &x0v) {
        // x0_given: `eps` holds pred_xstart already processed by the caller (denoised_fn + clamp, or START_X / PREVIOUS_X, :293-304)
        float x0 = x0_given ? ev + poison : r * xv - rm1 * ev;
        if (clip && !x0_given) x0 = clampf(x0, -1.f, 1.f);
        const float e = (r * xv - x0) / rm1;         // eps re-derived from pred_xstart (:555-558)
        sv = x0 * san + s1man * e;                   // Equation 12 reversed (:562-565)
        x0v = x0;
    };
    if (VEC) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += (long)gridDim.x * blockDim.x) {
            const f32x4 xv = reinterpret_cast<const f32x4 *>(x + base)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(eps + base)[i];
            f32x4 sv, zv;
#pragma unroll
            for (int k = 0; k < 4; ++k) { float s, z; one(xv[k], ev[k], s, z); sv[k] = s; zv[k] = z; }
            reinterpret_cast<f32x4 *>(sample + base)[i] = sv;
            if (x0_out) reinterpret_cast<f32x4 *>(x0_out + base)[i] = zv;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
            float s, z;
            one(x[base + i], eps[base + i], s, z);
            sample[base + i] = s;
            if (x0_out) x0_out[base + i] = z;
        }
    }
}

// ---- variational-bound terms ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float normal_kl(float m1, float lv1, float m2, float lv2) {
    // losses.py:35-41: 0.5 * (-1.0 + lv2 - lv1 + exp(lv1 - lv2) + ((m1 - m2) ** 2) * exp(-lv2))
    const float d = m1 - m2;
    return 0.5f * ((((-1.0f + lv2) - lv1) + expf(lv1 - lv2)) + (d * d) * expf(-lv2));
}

__device__ __forceinline__ float approx_cdf(float x) {
    // losses.py:44-49; np.sqrt(2 / pi) and 0.044715 enter as fp32 scalars, th.pow(x, 3) is x * x * x
    const float s = 0.7978845608028654f;
    return 0.5f * (1.0f + tanhf(s * (x + 0.044715f * ((x * x) * x))));
}

__device__ __forceinline__ float decoder_nll(float x, float mean, float logvar) {
    // -discretized_gaussian_log_likelihood (losses.py:52-77) with log_scales = 0.5 * log_variance (:679-681)
    const float ls = 0.5f * logvar;
    const float cx = x - mean;
    const float inv = expf(-ls);
    const float w = 1.0f / 255.0f;
    const float cdf_plus = approx_cdf(inv * (cx + w));
    const float cdf_min = approx_cdf(inv * (cx - w));
    float lp;
    if (x < -0.999f) lp = logf(clamp_min(cdf_plus, 1e-12f));
    else if (x > 0.999f) lp = logf(clamp_min(1.0f - cdf_min, 1e-12f));
    else lp = logf(clamp_min(cdf_plus - cdf_min, 1e-12f));
    return -lp;
}

struct Acc { double vb, xm, mse; };
__device__ __forceinline__ Acc operator+(Acc a, Acc b) { return Acc{a.vb + b.vb, a.xm + b.xm, a.mse + b.mse}; }     // three sums through one tree

// One element of one timestep: the selected vb term (decoder NLL at t == 0, else KL), (pred_xstart - x_start)^2, (eps_hat - noise)^2.
struct VbElem {
    float r, rm1, pc1, pc2, ic1, c21, minlog, maxlog, fixlog;
    int mean_type, var_type, clip, t0;
    float poison;
    __device__ __forceinline__ void operator()(float xs, float xt, float nz, float mo, float vv, Acc &a) const {
        float x0;
        if (mean_type == HL_MEAN_EPSILON) x0 = r * xt - rm1 * mo;
        else if (mean_type == HL_MEAN_START_X) x0 = mo;
        else x0 = ic1 * mo - c21 * xt;                                    // _predict_xstart_from_xprev (:335-343)
        x0 = x0 + poison;
        if (clip) x0 = clampf(x0, -1.f, 1.f);
        const float mean = mean_type == HL_MEAN_PREVIOUS_X ? mo + poison : pc1 * x0 + pc2 * xt;
        float lv;
        if (var_type == HL_VAR_FIXED) lv = fixlog;
        else if (var_type == HL_VAR_LEARNED) lv = vv;
        else {                                                            // LEARNED_RANGE (:265-272)
            const float frac = (vv + 1.f) / 2.f;
            lv = frac * maxlog + (1.f - frac) * minlog;
        }
        float term;
        if (t0) term = decoder_nll(xs, mean, lv);
        else term = normal_kl(pc1 * xs + pc2 * xt, minlog, mean, lv);     // true posterior (:208-230) against the model
        const float dx = x0 - xs;
        const float e = (r * xt - x0) / rm1;                              // _predict_eps_from_xstart (:345-349)
        const float de = e - nz;
        a.vb += (double)(term + poison);
        a.xm += (double)(dx * dx);
        a.mse += (double)(de * de);
    }
};

// PRIOR: KL(q(x_T | x_0) || N(0, 1)) per element (:786-789) into the vb slot; x_t, noise, model output unused.
template <bool VEC, bool PRIOR>
__global__ __launch_bounds__(TPB) void k_vb_partial(const float *__restrict__ xs, const float *__restrict__ xt, const float *__restrict__ nz,
                                                     const float *__restrict__ mo, const float *__restrict__ vv, long out_stride,
                                                     const float *__restrict__ coef, const int64_t *__restrict__ t, long n, int T, int mean_type,
                                                     int var_type, int clip, double *__restrict__ partial) {
    __shared__ Acc sh[TPB];
    const int b = blockIdx.y;
    const int64_t tb = PRIOR ? (int64_t)T - 1 : t[b];
    const bool in_range = tb >= 0 && tb < (int64_t)T;
    const float *c = coef + (in_range ? tb : 0) * NCOL;
    Acc a{0.0, 0.0, 0.0};
    const long base = (long)b * n, mbase = (long)b * out_stride;
    if (PRIOR) {
        const float sa = c[C_SA], lv1 = c[C_LOG1MA];
        auto one = [&](float x) { a.vb += (double)normal_kl(sa * x, lv1, 0.f, 0.f); };
        if (VEC) {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += (long)gridDim.x * blockDim.x) {
                const f32x4 xv = reinterpret_cast<const f32x4 *>(xs + base)[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) one(xv[k]);
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) one(xs[base + i]);
        }
    } else {
        const VbElem f{c[C_R], c[C_RM1], c[C_PC1], c[C_PC2], c[C_IC1], c[C_C21], c[C_MINLOG], c[C_MAXLOG], c[C_FIXLOG],
                       mean_type, var_type, clip, tb == 0 ? 1 : 0, in_range ? 0.f : __builtin_nanf("")};
        if (VEC) {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += (long)gridDim.x * blockDim.x) {
                const f32x4 s4 = reinterpret_cast<const f32x4 *>(xs + base)[i];
                const f32x4 t4 = reinterpret_cast<const f32x4 *>(xt + base)[i];
                const f32x4 n4 = reinterpret_cast<const f32x4 *>(nz + base)[i];
                const f32x4 m4 = reinterpret_cast<const f32x4 *>(mo + mbase)[i];
                const f32x4 v4 = vv ? reinterpret_cast<const f32x4 *>(vv + mbase)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) f(s4[k], t4[k], n4[k], m4[k], v4[k], a);
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
                f(xs[base + i], xt[base + i], nz[base + i], mo[mbase + i], vv ? vv[mbase + i] : 0.f, a);
        }
    }
    a = hl::block_sum(a, sh);
    if (threadIdx.x == 0) {
        double *dst = partial + ((long)b * gridDim.x + blockIdx.x) * 3;
        dst[0] = a.vb;
        dst[1] = a.xm;
        dst[2] = a.mse;
    }
}

// One workgroup per sample: the sample's partials in a fixed order -> mean over n, / ln 2 for the vb term -> column j of the (B, ld) outputs.
__global__ __launch_bounds__(TPB) void k_vb_final(const double *__restrict__ partial, long nparts, long n, float *__restrict__ vb,
                                                   float *__restrict__ xstart_mse, float *__restrict__ mse, long ld, long j) {
    __shared__ Acc sh[TPB];
    const int b = blockIdx.x;
    Acc a{0.0, 0.0, 0.0};
    const double *p = partial + (long)b * nparts * 3;
    for (long q = threadIdx.x; q < nparts; q += TPB) { a.vb += p[q * 3]; a.xm += p[q * 3 + 1]; a.mse += p[q * 3 + 2]; }      // (strided_sum's order, three sums at once)
    a = hl::block_sum(a, sh);
    if (threadIdx.x == 0) {
        const double inv_n = 1.0 / (double)n, ln2 = 0.69314718055994530942;
        vb[(long)b * ld + j] = (float)(a.vb * inv_n / ln2);
        if (xstart_mse) xstart_mse[(long)b * ld + j] = (float)(a.xm * inv_n);
        if (mse) mse[(long)b * ld + j] = (float)(a.mse * inv_n);
    }
}

}  // namespace

extern "C" int hl_diffusion_q_sample(const float *x_start, const float *noise, const float *coef, const int64_t *t, float *x_t,
                                     int64_t n_per_sample, int B, int T, void *stream) {
    HL_REQUIRE(x_start && noise && coef && t && x_t, "hl_diffusion_q_sample: null argument");
    HL_REQUIRE(n_per_sample > 0 && B > 0 && T > 0, "hl_diffusion_q_sample: bad sizes");
    const bool vec = n_per_sample % 4 == 0 && hl::aligned16({x_start, noise, x_t});
    dim3 grid((unsigned)blocks_for(n_per_sample, vec), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(k_q_sample<true>, grid, dim3(TPB), 0, st, x_start, noise, coef, t, x_t, (long)n_per_sample, T);
    else hipLaunchKernelGGL(k_q_sample<false>, grid, dim3(TPB), 0, st, x_start, noise, coef, t, x_t, (long)n_per_sample, T);
    return hl::check_launch("k_q_sample");
}

extern "C" int hl_diffusion_reverse_step(int mode, const float *x, const float *eps, const float *coef, const int64_t *t, float *sample,
                                         float *pred_xstart, int64_t n_per_sample, int B, int T, int clip, void *stream) {
    HL_REQUIRE(x && eps && coef && t && sample, "hl_diffusion_reverse_step: null argument");
    HL_REQUIRE(mode == 0 || mode == 1, "hl_diffusion_reverse_step: mode %d", mode);
    HL_REQUIRE(n_per_sample > 0 && B > 0 && T > 0, "hl_diffusion_reverse_step: bad sizes");
    const bool vec = n_per_sample % 4 == 0 && hl::aligned16({x, eps, sample, pred_xstart});
    dim3 grid((unsigned)blocks_for(n_per_sample, vec), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(k_reverse<true>, grid, dim3(TPB), 0, st, x, eps, coef, t, sample, pred_xstart, (long)n_per_sample, T, clip, mode);
    else hipLaunchKernelGGL(k_reverse<false>, grid, dim3(TPB), 0, st, x, eps, coef, t, sample, pred_xstart, (long)n_per_sample, T, clip, mode);
    return hl::check_launch("k_reverse");
}

extern "C" size_t hl_diffusion_vb_scratch_bytes(int64_t n_per_sample, int B) {
    if (n_per_sample <= 0 || B <= 0) return 0;
    return (size_t)B * (size_t)blocks_for(n_per_sample, false) * 3 * sizeof(double);
}

extern "C" int hl_diffusion_vb_terms(int mean_type, int var_type, int clip, const float *x_start, const float *x_t, const float *noise,
                                     const float *model_out, const float *model_var, int64_t out_stride, const float *coef, const int64_t *t,
                                     int64_t n_per_sample, int B, int T, float *vb, float *xstart_mse, float *mse, int64_t ld, int64_t j,
                                     void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(x_start && x_t && noise && model_out && coef && t && vb && xstart_mse && mse && scratch, "hl_diffusion_vb_terms: null argument");
    HL_REQUIRE(mean_type >= HL_MEAN_EPSILON && mean_type <= HL_MEAN_PREVIOUS_X, "hl_diffusion_vb_terms: mean_type %d", mean_type);
    HL_REQUIRE(var_type >= HL_VAR_FIXED && var_type <= HL_VAR_LEARNED_RANGE, "hl_diffusion_vb_terms: var_type %d", var_type);
    HL_REQUIRE((var_type == HL_VAR_FIXED) == (model_var == nullptr), "hl_diffusion_vb_terms: model_var must be given exactly for learned variances");
    HL_REQUIRE(n_per_sample > 0 && B > 0 && T > 0 && out_stride >= n_per_sample, "hl_diffusion_vb_terms: bad sizes");
    HL_REQUIRE(ld > 0 && j >= 0 && j < ld, "hl_diffusion_vb_terms: column %lld outside a row of %lld", (long long)j, (long long)ld);
    HL_REQUIRE(scratch_bytes >= hl_diffusion_vb_scratch_bytes(n_per_sample, B), "hl_diffusion_vb_terms: scratch too small");
    const bool vec = n_per_sample % 4 == 0 && out_stride % 4 == 0 && hl::aligned16({x_start, x_t, noise, model_out, model_var});
    const long g = blocks_for(n_per_sample, vec);
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)scratch;
#define HL_GO(V) hipLaunchKernelGGL((k_vb_partial<V, false>), dim3((unsigned)g, (unsigned)B), dim3(TPB), 0, st, x_start, x_t, noise, model_out, \
                                    model_var, (long)out_stride, coef, t, (long)n_per_sample, T, mean_type, var_type, clip, partial)
    if (vec) HL_GO(true); else HL_GO(false);
#undef HL_GO
    int rc = hl::check_launch("k_vb_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(k_vb_final, dim3((unsigned)B), dim3(TPB), 0, st, partial, g, (long)n_per_sample, vb, xstart_mse, mse, (long)ld, (long)j);
    return hl::check_launch("k_vb_final");
}

extern "C" int hl_diffusion_prior_bpd(const float *x_start, const float *coef, int64_t n_per_sample, int B, int T, float *prior_bpd,
                                      void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(x_start && coef && prior_bpd && scratch, "hl_diffusion_prior_bpd: null argument");
    HL_REQUIRE(n_per_sample > 0 && B > 0 && T > 0, "hl_diffusion_prior_bpd: bad sizes");
    HL_REQUIRE(scratch_bytes >= hl_diffusion_vb_scratch_bytes(n_per_sample, B), "hl_diffusion_prior_bpd: scratch too small");
    const bool vec = n_per_sample % 4 == 0 && hl::aligned16({x_start});
    const long g = blocks_for(n_per_sample, vec);
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)scratch;
#define HL_GO(V) hipLaunchKernelGGL((k_vb_partial<V, true>), dim3((unsigned)g, (unsigned)B), dim3(TPB), 0, st, x_start, nullptr, nullptr, nullptr, \
                                    nullptr, (long)n_per_sample, coef, nullptr, (long)n_per_sample, T, 0, 0, 0, partial)
    if (vec) HL_GO(true); else HL_GO(false);
#undef HL_GO
    int rc = hl::check_launch("k_vb_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(k_vb_final, dim3((unsigned)B), dim3(TPB), 0, st, partial, g, (long)n_per_sample, prior_bpd, nullptr, nullptr, 1L, 0L);
    return hl::check_launch("k_vb_final");
}
