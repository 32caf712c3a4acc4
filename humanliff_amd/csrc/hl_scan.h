// The three-kernel exclusive scan of the mesh path (hl_geometry.hip: band, marching-cubes and component offsets; hl_mesh_simplify.hip:
// cluster ids, surviving triangles, surviving vertices; hl_mesh_distance.hip: triangle areas, cell starts, wide triangles).  The values
// are packed (low 32, high 32) integer counts and every sum is an integer sum, so the result does not depend on any order.
//
//   k_scan_reduce: a workgroup per tile of kScanTile values -> the tile's sum.
//   k_scan_top:    one workgroup: tile sums -> exclusive tile offsets (in place); the grand total unpacked into counts[0] (low) / [1] (high).
//   k_scan_down:   a workgroup per tile, kScanItems consecutive values per thread: out(i, exclusive prefix of i, value of i).
//
//   scan_exclusive: the three on a stream, then check_launch(what); `blocks` holds scan_blocks(n) words.
//   scan_total:     reduce and top alone: only the total, in counts[0] / [1].
//
// F is a functor `unsigned long long operator()(long i)`, O a functor `void operator()(long i, unsigned long long run, unsigned long long v)`.
// The kernels have internal linkage: every file that includes this header gets its own.
#pragma once
#include "hl_reduce.h"

namespace hl {

constexpr int kScanThreads = kReduceThreads;
constexpr int kScanItems = 16;
constexpr int kScanTile = kScanThreads * kScanItems;

inline long scan_blocks(long n) { return (n + kScanTile - 1) / kScanTile; }

#if defined(__HIPCC__)
namespace {

template <class F>
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(F f, long n, unsigned long long *__restrict__ block_sums) {
    __shared__ unsigned long long red[kScanThreads];
    const long base = (long)blockIdx.x * kScanTile;
    unsigned long long s = 0;
    for (int k = 0; k < kScanItems; ++k) {
        const long i = base + (long)k * kScanThreads + threadIdx.x;
        if (i < n) s += f(i);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s;
}

__device__ unsigned long long block_exclusive(unsigned long long v, unsigned long long *sh, unsigned long long *total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 1; w < kScanThreads; w <<= 1) {            // Hillis-Steele inclusive scan
        const unsigned long long add = (int)threadIdx.x >= w ? sh[threadIdx.x - w] : 0ull;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long incl = sh[threadIdx.x];
    if (total) *total = sh[kScanThreads - 1];
    __syncthreads();
    return incl - v;
}

// one workgroup: block sums -> exclusive block offsets (in place); the grand total unpacked into counts[0] (low) / counts[1] (high)
__global__ __launch_bounds__(kScanThreads) void k_scan_top(unsigned long long *__restrict__ block_sums, long nblocks, int64_t *__restrict__ counts) {
    __shared__ unsigned long long sh[kScanThreads];
    const long chunk = (nblocks + kScanThreads - 1) / kScanThreads;
    const long b0 = (long)threadIdx.x * chunk;
    const long b1 = b0 + chunk < nblocks ? b0 + chunk : nblocks;
    unsigned long long s = 0;
    for (long b = b0; b < b1; ++b) s += block_sums[b];
    unsigned long long total;
    unsigned long long run = block_exclusive(s, sh, &total);
    for (long b = b0; b < b1; ++b) {
        const unsigned long long v = block_sums[b];
        block_sums[b] = run;
        run += v;
    }
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)(total & 0xffffffffull);
        counts[1] = (int64_t)(total >> 32);
    }
}

template <class F, class O>
__global__ __launch_bounds__(kScanThreads) void k_scan_down(F f, O out, long n, const unsigned long long *__restrict__ block_off) {
    __shared__ unsigned long long sh[kScanThreads];
    const long base = (long)blockIdx.x * kScanTile + (long)threadIdx.x * kScanItems;
    unsigned long long s = 0;
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) s += f(base + k);
    unsigned long long run = block_off[blockIdx.x] + block_exclusive(s, sh, nullptr);
    for (int k = 0; k < kScanItems; ++k) {
        const long i = base + k;
        if (i >= n) break;
        const unsigned long long v = f(i);
        out(i, run, v);
        run += v;
    }
}

template <class F>
int scan_total(F f, long n, unsigned long long *blocks, int64_t *counts, hipStream_t st, const char *what) {
    const long nb = scan_blocks(n);
    hipLaunchKernelGGL((k_scan_reduce<F>), dim3((unsigned)nb), dim3(kScanThreads), 0, st, f, n, blocks);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanThreads), 0, st, blocks, nb, counts);
    return check_launch(what);
}

template <class F, class O>
int scan_exclusive(F f, O out, long n, unsigned long long *blocks, int64_t *counts, hipStream_t st, const char *what) {
    const long nb = scan_blocks(n);
    hipLaunchKernelGGL((k_scan_reduce<F>), dim3((unsigned)nb), dim3(kScanThreads), 0, st, f, n, blocks);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanThreads), 0, st, blocks, nb, counts);
    hipLaunchKernelGGL((k_scan_down<F, O>), dim3((unsigned)nb), dim3(kScanThreads), 0, st, f, out, n, (const unsigned long long *)blocks);
    return check_launch(what);
}

}  // namespace
#endif

}  // namespace hl
