// Device code the two body models share (csrc/hl_body.hip: SMPL, csrc/hl_smplx.hip: SMPL-X): the transpose that packs a model and the
// world bounds of a frame.  Included by those two files only; every kernel here sits in an unnamed namespace, so each file gets its own
// copy.  fp32 on the vector ALU, every sum in a fixed order.
#pragma once
#include "hl_reduce.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kReduceThreads, "block_reduce reduces a workgroup of kReduceThreads");

// out[(k C + c) V + v] = in[(v C + c) cols + k], k < K  (a caller that wants columns k0 .. k0 + K - 1 passes in + k0)
__global__ __launch_bounds__(kThreads) void k_body_transpose(const float *__restrict__ in, int V, int C, int cols, int K,
                                                             float *__restrict__ out) {
    const int64_t n = (int64_t)K * C * V;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int v = (int)(i % V);
    const int64_t kc = i / V;
    const int c = (int)(kc % C), k = (int)(kc / C);
    out[i] = in[((int64_t)v * C + c) * cols + k];
}

// one workgroup per frame: min / max of the frame's vertices (thread t takes t, t + 256, ..., then the tree), - / + margin, y once more
// by y_margin: two fp32 subtractions
__global__ __launch_bounds__(kThreads) void k_body_bounds(const float *__restrict__ vertices, int V, float margin, float y_margin,
                                                          float *__restrict__ bounds) {
    __shared__ float sh[kThreads];
    const float *p = vertices + (int64_t)blockIdx.x * V * 3;
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = INFINITY, hi[c] = -INFINITY;
    for (int v = (int)threadIdx.x; v < V; v += kThreads)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = p[3 * (int64_t)v + c];
            lo[c] = fminf(lo[c], x);
            hi[c] = fmaxf(hi[c], x);
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = block_reduce(lo[c], sh, Min());
        hi[c] = block_reduce(hi[c], sh, Max());
    }
    if (threadIdx.x == 0) {
        float *o = bounds + (int64_t)blockIdx.x * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float a = lo[c] - margin, b = hi[c] + margin;
            if (c == 1) a = a - y_margin, b = b + y_margin;
            o[c] = a, o[3 + c] = b;
        }
    }
}

}  // namespace
}  // namespace hl
