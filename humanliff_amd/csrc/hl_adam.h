// What the optimizer kernels share (hl_optim.hip, hl_fit.hip): Adam's per-element update in torch's multi-tensor op order, the host's
// scalars for it and 16-byte accesses.  The workgroup's fixed-order fp64 sum is hl_reduce.h's.
#pragma once
#include "hl_reduce.h"

#include <cmath>

namespace hl {

constexpr int kOptThreads = 256;

// bc2_sqrt = sqrt(1 - beta2^step), neg_step = -lr / (1 - beta1^step): computed in double on the host, as torch does, handed over as floats
struct AdamCoef {
    float b1c, b1c_hi, b2, b2c, bc2_sqrt, eps, neg_step;
    int lerp_lo;
};

inline AdamCoef adam_coef(float one_minus_beta1, float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float neg_step_size) {
    AdamCoef c{};
    c.b1c = one_minus_beta1;
    c.b1c_hi = 1.f - one_minus_beta1;          // (at::lerp's 1 - weight, in the weight's precision)
    c.lerp_lo = fabsf(one_minus_beta1) < 0.5f;
    c.b2 = beta2;
    c.b2c = one_minus_beta2;
    c.bc2_sqrt = bc2_sqrt;
    c.eps = eps;
    c.neg_step = neg_step_size;
    return c;
}

#if defined(__HIPCC__)
// m = lerp(m, g, 1 - beta1); v = v * beta2 + (1 - beta2) g g; p += neg_step * m / (sqrt(v) / bc2_sqrt + eps)   (hl_optim.hip lists torch's ops)
__device__ __forceinline__ void adam_moments(float g, float &p, float &m, float &v, const AdamCoef &c) {
    // at::lerp: weight < 0.5 ? self + w (end - self) : end - (end - self)(1 - w)
    m = c.lerp_lo ? fmaf(c.b1c, g - m, m) : fmaf(-(g - m), c.b1c_hi, g);
    v = fmaf(c.b2c, g * g, v * c.b2);
    const float den = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = fmaf(c.neg_step, m / den, p);
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }
#endif

}  // namespace hl
