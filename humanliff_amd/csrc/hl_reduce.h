// The fixed-order reductions every "bit-identical run to run" promise of the library rests on (geometry, bits-per-dim evaluation, the
// fused AdamW step, the FitLoop, the image metrics, LPIPS, and the wave sums of the renderer and the UNet).  Two orders, stated once:
//
//   workgroup tree (block_reduce, 256 threads): sh[t] = x_t; for s = 128, 64, ..., 1: threads t < s do sh[t] = op(sh[t], sh[t + s]).
//     Over partials in memory (strided_sum): thread t first adds p[stride * i] for i = t, t + 256, ... in that order, then the tree.
//   wave butterfly (wave_xor_*, 64 lanes): for d = 32, 16, ..., 1: v = op(v, v of lane ^ d).  Every lane ends with the same bits.
//
// Floating-point addition is not associative: a sum keeps its bits only while it keeps its order, so a change to either loop changes
// results (tests/test_reduce_gpu.py pins the tree's order).  hl_stats.h has two look-alikes that are NOT these functions:
// wave_sum_f32 adds inside each row of 16 lanes with four DPP steps (lane ^ 1, lane ^ 2, half mirror, mirror) and then the four rows as
// (r0 + r1) + (r2 + r3) - another association than the butterfly's, so swapping one for the other changes the low bits of a float sum;
// wave_max_u32 is the same shape on unsigned values (a maximum would survive the swap, but it stays next to its twin).
//
// Some butterflies of hl_render.hip, hl_unet_kernels.hip and hl_unet_train.hip stay written out in their kernels: the same order, but
// calling wave_xor_* there changed the instruction schedule of kernels the benchmark times, and this header is not worth that risk.
#pragma once
#include <cstdint>

#include "hl_common.h"

namespace hl {

constexpr int kReduceThreads = 256;       // the workgroup size of every kernel that calls block_reduce / block_sum / strided_sum

#if defined(__HIPCC__)
struct Add {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct Min {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; }
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct Max {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};

// fixed-shape tree over the workgroup's 256 values (T may be a small struct); every thread ends with the result, and `sh` is free again on return
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T x, T *sh, Op op) {
    sh[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const T tot = sh[0];
    __syncthreads();
    return tot;
}

template <class T>
__device__ __forceinline__ T block_sum(T x, T *sh) { return block_reduce(x, sh, Add()); }

// sum of p[0], p[stride], ..., p[stride (n - 1)]: thread t adds i = t, t + 256, ... in order, then the tree
__device__ __forceinline__ double strided_sum(const double *__restrict__ p, int64_t n, int64_t stride, double *sh) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kReduceThreads) acc += p[stride * i];
    return block_sum(acc, sh);
}

template <class T, class Op>
__device__ __forceinline__ T wave_xor_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_xor_sum(T v) { return wave_xor_reduce(v, Add()); }
template <class T>
__device__ __forceinline__ T wave_xor_max(T v) { return wave_xor_reduce(v, Max()); }
template <class T>
__device__ __forceinline__ T wave_xor_min(T v) { return wave_xor_reduce(v, Min()); }
#endif

}  // namespace hl
