// Pairwise float64 metrics on feature sets, MI355X (gfx950): KID, the k-NN radii and the manifold pass of improved precision / recall and
// density / coverage.  Contract: DESIGN.md 4m "Feature metrics".
//
// One workgroup tile body (tile_gram) and four epilogues.  Inputs are row-major fp32 matrices x (N, D), y (M, D); a workgroup (256
// threads) owns 64 rows of one side x 64 rows of the other, thread (ty, tx) the 4 x 4 block of rows 4 ty.. and columns 4 tx...  D runs in
// chunks of 32 staged in LDS as fp32, transposed to [k][row] (16 KB for both sides; the next chunk's loads are in flight in registers
// while this one is multiplied); per k a thread reads one float4 of each side, widens the 8 values and issues 16 v_fma_f64.
//
// The Gram entry: g(a, b) = fma(a_k, b_k, g) for k = 0, 1, ..., D - 1 in that order, from g = +0 (gram_step).  The product of two fp32
// values is exact in float64, so the fused step rounds exactly like a separate product and sum: one rounding per k, in one order.  A
// padded k (a tile's last chunk past D) adds +0 x +0, which changes nothing.  So g depends on the two rows' contents alone - not on their
// indices, the set sizes, the tile, the side, nor on the chunking - and g(a, b) = g(b, a) bit for bit.  No split-K, no float atomics.
// k_feat_norms runs the same chain for g(a, a), so d2(a, b) = max(0, (g(a,a) + g(b,b)) - 2 g(a,b)) is exactly 0 for bit-equal rows.
//
// Epilogues: k_feat_pairwise (dense g or d2), k_feat_kid (per-tile partial sums of the cubic kernel over gathered subsets; k_feat_kid_total
// adds them in the fixed order of hl_reduce.h), k_feat_knn (per thread the 8 smallest d2 of each of its rows, merged over the 16 threads
// of a row with a butterfly; k_feat_knn_merge merges the column chunks and picks the k-th), k_feat_manifold (hit counts and the nearest
// distance; integer atomic adds and a 64-bit atomic min on the bits of a non-negative double, both independent of the order).
#include "hl_common.h"
#include "hl_reduce.h"

namespace hl {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kT = 64;                        // rows of either side per workgroup tile
constexpr int kKC = 32;                       // values of D per staged chunk
constexpr int kList = HL_FEAT_MAX_K;          // every k-list keeps this many, the k-th is picked at the end
constexpr int kTargetBlocks = 1024;           // the column split aims at this many workgroups (256 CUs x 4)
constexpr int64_t kMaxTiles = 1 << 30;
static_assert(kT * kT == kThreads * 16 && kT * kKC == kThreads * 8, "a thread owns 4 x 4 results and loads 2 float4 of each side per chunk");

__device__ __forceinline__ double gram_step(double g, float a, float b) { return fma((double)a, (double)b, g); }

__device__ __forceinline__ double dist2(double gaa, double gbb, double gab) {
    const double d = __dsub_rn(__dadd_rn(gaa, gbb), __dmul_rn(2.0, gab));
    return d > 0.0 ? d : 0.0;
}

// row `r` of a set of n rows, through an optional index table (a row the table sends outside the set counts as absent)
__device__ __forceinline__ int64_t gather(const int32_t *idx, int64_t r, int64_t count, int64_t n) {
    if (r >= count) return -1;
    const int64_t g = idx ? (int64_t)idx[r] : r;
    return g >= 0 && g < n ? g : -1;
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float *row, int64_t k, int64_t D) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row) return v;
    if (VEC) {
        if (k < D) v = *reinterpret_cast<const float4 *>(row + k);
    } else {
        if (k < D) v.x = row[k];
        if (k + 1 < D) v.y = row[k + 1];
        if (k + 2 < D) v.z = row[k + 2];
        if (k + 3 < D) v.w = row[k + 3];
    }
    return v;
}

struct alignas(16) Stage {
    float x[kKC][kT], y[kKC][kT];
};

// acc[p][q] = g(row 4 ty + p of the x tile, row 4 tx + q of the y tile).  xrow / yrow: the row this thread loads for the workgroup (tile
// row tid & 63; NULL: absent, zeros).  Barriers inside: every thread of the workgroup calls it, in uniform control flow.
template <bool VEC>
__device__ __forceinline__ void tile_gram(const float *xrow, const float *yrow, int64_t D, Stage &sh, double (&acc)[4][4]) {
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid & 63, kq = (tid >> 6) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    float4 px[2], py[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) px[h] = load4<VEC>(xrow, kq + 16 * h, D), py[h] = load4<VEC>(yrow, kq + 16 * h, D);
    for (int64_t k0 = 0; k0 < D; k0 += kKC) {
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = kq + 16 * h;
            sh.x[k][lr] = px[h].x, sh.x[k + 1][lr] = px[h].y, sh.x[k + 2][lr] = px[h].z, sh.x[k + 3][lr] = px[h].w;
            sh.y[k][lr] = py[h].x, sh.y[k + 1][lr] = py[h].y, sh.y[k + 2][lr] = py[h].z, sh.y[k + 3][lr] = py[h].w;
        }
        __syncthreads();
        if (k0 + kKC < D) {
#pragma unroll
            for (int h = 0; h < 2; ++h) px[h] = load4<VEC>(xrow, k0 + kKC + kq + 16 * h, D), py[h] = load4<VEC>(yrow, k0 + kKC + kq + 16 * h, D);
        }
#pragma unroll 4
        for (int k = 0; k < kKC; ++k) {
            const float4 a = *reinterpret_cast<const float4 *>(&sh.x[k][4 * ty]);
            const float4 b = *reinterpret_cast<const float4 *>(&sh.y[k][4 * tx]);
            const float u[4] = {a.x, a.y, a.z, a.w}, v[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = gram_step(acc[p][q], u[p], v[q]);
        }
    }
}

__device__ __forceinline__ const float *row_ptr(const float *base, int64_t g, int64_t D) { return g < 0 ? nullptr : base + g * D; }

// ---- norms: g(a, a) by the chain of the tile body ----
__global__ __launch_bounds__(kThreads) void k_feat_norms(const float *__restrict__ x, int64_t n, int64_t D, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float *row = x + i * D;
    double g = 0.0;
#pragma unroll 8
    for (int64_t k = 0; k < D; ++k) g = gram_step(g, row[k], row[k]);
    out[i] = g;
}

// ---- dense ----
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_feat_pairwise(const float *__restrict__ x, int64_t N, const float *__restrict__ y, int64_t M, int64_t D,
                                                           const double *__restrict__ nx, const double *__restrict__ ny, int d2, int64_t tcols,
                                                           double *__restrict__ out) {
    __shared__ Stage sh;
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid & 63;
    const int64_t i0 = ((int64_t)blockIdx.x / tcols) * kT, j0 = ((int64_t)blockIdx.x % tcols) * kT;
    double acc[4][4];
    tile_gram<VEC>(row_ptr(x, gather(nullptr, i0 + lr, N, N), D), row_ptr(y, gather(nullptr, j0 + lr, M, M), D), D, sh, acc);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = i0 + 4 * ty + p;
        if (i >= N) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = j0 + 4 * tx + q;
            if (j < M) out[i * M + j] = d2 ? dist2(nx[i], ny[j], acc[p][q]) : acc[p][q];
        }
    }
}

// ---- KID ----
__device__ __forceinline__ double cubic(double g, double D) {
    const double t = __dadd_rn(__ddiv_rn(g, D), 1.0);
    return __dmul_rn(__dmul_rn(t, t), t);
}

// grid (tiles x tiles, S, 3): z = 0: x with x, 1: y with y, 2: x with y.  partial[(s 3 + z) tiles^2 + tile] = the tile's sum of k in the
// order: a thread's 16 values row-major, then the workgroup tree.  Same-set pairs: the diagonal (by position in the subset) is left out,
// tiles above the diagonal count twice (g is symmetric bit for bit), tiles below it write 0.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_feat_kid(const float *__restrict__ x, int64_t N, const float *__restrict__ y, int64_t M, int64_t D,
                                                      const int32_t *__restrict__ xi, const int32_t *__restrict__ yi, int64_t m, int64_t tiles,
                                                      double *__restrict__ partial) {
    __shared__ Stage sh;
    __shared__ double red[kThreads];
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid & 63;
    const int z = (int)blockIdx.z;
    const int64_t s = blockIdx.y, ti = (int64_t)blockIdx.x / tiles, tj = (int64_t)blockIdx.x % tiles;
    double *dst = partial + (s * 3 + z) * tiles * tiles + blockIdx.x;
    if (z < 2 && tj < ti) {
        if (tid == 0) *dst = 0.0;
        return;
    }
    const float *a = z == 1 ? y : x, *b = z == 0 ? x : y;
    const int64_t na = z == 1 ? M : N, nb = z == 0 ? N : M;
    const int32_t *ia = (z == 1 ? yi : xi) + s * m, *ib = (z == 0 ? xi : yi) + s * m;
    const int64_t i0 = ti * kT, j0 = tj * kT;
    double acc[4][4];
    tile_gram<VEC>(row_ptr(a, gather(ia, i0 + lr, m, na), D), row_ptr(b, gather(ib, j0 + lr, m, nb), D), D, sh, acc);
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 4 * ty + p, j = j0 + 4 * tx + q;
            if (i < m && j < m && !(z < 2 && i == j)) sum = __dadd_rn(sum, cubic(acc[p][q], (double)D));
        }
    sum = block_sum(sum, red);
    if (tid == 0) *dst = (z < 2 && tj > ti) ? __dmul_rn(2.0, sum) : sum;
}

__global__ __launch_bounds__(kThreads) void k_feat_kid_total(const double *__restrict__ partial, int64_t tiles2, int64_t m, double *__restrict__ out) {
    __shared__ double red[kThreads];
    const double *p = partial + (int64_t)blockIdx.x * 3 * tiles2;
    const double xx = strided_sum(p, tiles2, 1, red), yy = strided_sum(p + tiles2, tiles2, 1, red), xy = strided_sum(p + 2 * tiles2, tiles2, 1, red);
    if (threadIdx.x == 0) {
        const double mm1 = __dmul_rn((double)m, (double)(m - 1)), mm = __dmul_rn((double)m, (double)m);
        out[blockIdx.x] = __dsub_rn(__dadd_rn(__ddiv_rn(xx, mm1), __ddiv_rn(yy, mm1)), __ddiv_rn(__dmul_rn(2.0, xy), mm));
    }
}

// ---- k-NN radii ----
struct KList {
    double v[kList];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < kList; ++s) v[s] = __longlong_as_double(0x7ff0000000000000LL);
    }
    // keep the kList smallest, ascending; a multiset operation: the kept values do not depend on the order of the insertions
    __device__ __forceinline__ void insert(double d) {
        if (!(d < v[kList - 1])) return;
        v[kList - 1] = d;
#pragma unroll
        for (int s = kList - 1; s > 0; --s) {
            const double lo = v[s - 1], hi = v[s];
            const bool sw = hi < lo;
            v[s - 1] = sw ? hi : lo, v[s] = sw ? lo : hi;
        }
    }
};

// the column tiles of chunk c of `splits`
__device__ __forceinline__ void chunk_range(int64_t tcols, int splits, int c, int64_t &t0, int64_t &t1) {
    const int64_t per = (tcols + splits - 1) / splits;
    t0 = per * c;
    t1 = t0 + per < tcols ? t0 + per : tcols;
}

// grid (row tiles, splits): lists[(c N + i) kList + .] = the kList smallest d2 of row i to the rows j != i of column chunk c, ascending
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_feat_knn(const float *__restrict__ x, int64_t N, int64_t D, const double *__restrict__ nx, int splits,
                                                      double *__restrict__ lists) {
    __shared__ Stage sh;
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid & 63;
    const int64_t i0 = (int64_t)blockIdx.x * kT, tcols = (N + kT - 1) / kT;
    int64_t t0, t1;
    chunk_range(tcols, splits, (int)blockIdx.y, t0, t1);
    const float *xrow = row_ptr(x, gather(nullptr, i0 + lr, N, N), D);
    double ni[4];
    KList L[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = i0 + 4 * ty + p;
        ni[p] = i < N ? nx[i] : 0.0;
        L[p].clear();
    }
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kT;
        double acc[4][4], nj[4];
        tile_gram<VEC>(xrow, row_ptr(x, gather(nullptr, j0 + lr, N, N), D), D, sh, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) nj[q] = j0 + 4 * tx + q < N ? nx[j0 + 4 * tx + q] : 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t i = i0 + 4 * ty + p, j = j0 + 4 * tx + q;
                if (j < N && j != i) L[p].insert(dist2(ni[p], nj[q], acc[p][q]));
            }
    }
    // the 16 threads of a row are 16 neighbouring lanes of one wave
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) {
            double other[kList];
#pragma unroll
            for (int s = 0; s < kList; ++s) other[s] = __shfl_xor(L[p].v[s], d);
#pragma unroll
            for (int s = 0; s < kList; ++s) L[p].insert(other[s]);
        }
        const int64_t i = i0 + 4 * ty + p;
        if (tx == 0 && i < N) {
            double *dst = lists + ((int64_t)blockIdx.y * N + i) * kList;
#pragma unroll
            for (int s = 0; s < kList; ++s) dst[s] = L[p].v[s];
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_feat_knn_merge(const double *__restrict__ lists, int64_t N, int splits, int k, double *__restrict__ r2) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    KList L;
    L.clear();
    for (int c = 0; c < splits; ++c) {
        const double *src = lists + ((int64_t)c * N + i) * kList;
#pragma unroll
        for (int s = 0; s < kList; ++s) L.insert(src[s]);
    }
    double r = L.v[0];
#pragma unroll
    for (int s = 1; s < kList; ++s) r = s == k - 1 ? L.v[s] : r;
    r2[i] = r;
}

// ---- manifold pass ----
__global__ __launch_bounds__(kThreads) void k_feat_manifold_init(int32_t *hits_fake, int64_t M, int32_t *hits_real, unsigned long long *nearest, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < M) hits_fake[i] = 0;
    if (i < N) hits_real[i] = 0, nearest[i] = 0x7ff0000000000000ULL;
}

// grid (real row tiles, splits of the fake tiles)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_feat_manifold(const float *__restrict__ real, int64_t N, const float *__restrict__ fake, int64_t M, int64_t D,
                                                           const double *__restrict__ nr, const double *__restrict__ nf, const double *__restrict__ r2_real,
                                                           const double *__restrict__ r2_fake, int splits, int32_t *__restrict__ hits_fake,
                                                           int32_t *__restrict__ hits_real, unsigned long long *__restrict__ nearest) {
    __shared__ Stage sh;
    const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid & 63;
    const int64_t i0 = (int64_t)blockIdx.x * kT, tcols = (M + kT - 1) / kT;
    int64_t t0, t1;
    chunk_range(tcols, splits, (int)blockIdx.y, t0, t1);
    const float *xrow = row_ptr(real, gather(nullptr, i0 + lr, N, N), D);
    double ni[4], ri[4], best[4];
    int cnt_i[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = i0 + 4 * ty + p;
        ni[p] = i < N ? nr[i] : 0.0;
        ri[p] = i < N ? r2_real[i] : -1.0;
        best[p] = __longlong_as_double(0x7ff0000000000000LL);
        cnt_i[p] = 0;
    }
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * kT;
        double acc[4][4], nj[4], rj[4];
        int cnt_j[4];
        tile_gram<VEC>(xrow, row_ptr(fake, gather(nullptr, j0 + lr, M, M), D), D, sh, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = j0 + 4 * tx + q;
            nj[q] = j < M ? nf[j] : 0.0;
            rj[q] = j < M ? r2_fake[j] : -1.0;
            cnt_j[q] = 0;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t i = i0 + 4 * ty + p, j = j0 + 4 * tx + q;
                if (i < N && j < M) {
                    const double d = dist2(ni[p], nj[q], acc[p][q]);
                    cnt_j[q] += d <= ri[p] ? 1 : 0;
                    cnt_i[p] += d <= rj[q] ? 1 : 0;
                    best[p] = d < best[p] ? d : best[p];
                }
            }
        // a column's 16 threads: 4 per wave (lane bits 4, 5), 4 waves
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int c = cnt_j[q];
            c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            const int64_t j = j0 + 4 * tx + q;
            if ((tid & 48) == 0 && j < M && c) atomicAdd(&hits_fake[j], c);
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        int c = cnt_i[p];
        double b = best[p];
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) {
            c += __shfl_xor(c, d);
            const double o = __shfl_xor(b, d);
            b = o < b ? o : b;
        }
        const int64_t i = i0 + 4 * ty + p;
        if (tx == 0 && i < N && t1 > t0) {
            if (c) atomicAdd(&hits_real[i], c);
            atomicMin(&nearest[i], (unsigned long long)__double_as_longlong(b));
        }
    }
}

// ---- host ----
inline int64_t tiles_of(int64_t n) { return (n + kT - 1) / kT; }

inline bool vec_ok(int64_t D, std::initializer_list<const void *> ps) { return D % 4 == 0 && aligned16(ps); }

// the column split: enough chunks to reach kTargetBlocks workgroups, at most one chunk per column tile; a caller's `split` > 0 is taken as given
inline int resolve_split(int64_t rows, int64_t cols, int split) {
    const int64_t tr = tiles_of(rows), tc = tiles_of(cols);
    int64_t s = split > 0 ? split : (kTargetBlocks + tr - 1) / tr;
    s = s < tc ? s : tc;
    s = s < 1 ? 1 : (s > 65535 ? 65535 : s);
    return (int)s;
}

inline int norms(const float *x, int64_t n, int64_t D, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_feat_norms, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, x, n, D, out);
    return check_launch("k_feat_norms");
}

inline bool sizes_ok(int64_t N, int64_t M, int64_t D) {
    return N >= 1 && M >= 1 && D >= 1 && tiles_of(N) * tiles_of(M) <= kMaxTiles && N <= (int64_t)1 << 40 && M <= (int64_t)1 << 40 && D <= (int64_t)1 << 30;
}

inline size_t pad16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace
}  // namespace hl

using namespace hl;

#define FEAT_LAUNCH(kernel, vec, grid, st, ...)                                                      \
    do {                                                                                             \
        if (vec)                                                                                     \
            hipLaunchKernelGGL(kernel<true>, grid, dim3(kThreads), 0, st, __VA_ARGS__);              \
        else                                                                                         \
            hipLaunchKernelGGL(kernel<false>, grid, dim3(kThreads), 0, st, __VA_ARGS__);             \
    } while (0)

extern "C" {

size_t hl_feat_workspace_bytes(int op, int64_t N, int64_t M, int64_t S, int64_t m, int split) {
    switch (op) {
    case HL_FEAT_OP_PAIRWISE:
    case HL_FEAT_OP_MANIFOLD:
        return N >= 1 && M >= 1 ? pad16((size_t)N * 8) + pad16((size_t)M * 8) : 0;
    case HL_FEAT_OP_KID:
        return S >= 1 && S <= 65535 && m >= 2 && tiles_of(m) * tiles_of(m) <= kMaxTiles ? (size_t)S * 3 * tiles_of(m) * tiles_of(m) * 8 : 0;
    case HL_FEAT_OP_KNN:
        return N >= 2 ? pad16((size_t)N * 8) + (size_t)resolve_split(N, N, split) * N * kList * 8 : 0;
    }
    return 0;
}

int hl_feat_split(int64_t rows, int64_t cols, int split) { return rows >= 1 && cols >= 1 ? resolve_split(rows, cols, split) : 0; }

int hl_feat_pairwise(const float *x, int64_t N, const float *y, int64_t M, int64_t D, int kind, double *out, void *workspace, size_t workspace_bytes,
                     void *stream) {
    HL_REQUIRE(x && y && out, "hl_feat_pairwise: NULL argument");
    HL_REQUIRE(sizes_ok(N, M, D), "hl_feat_pairwise: bad sizes (N %lld, M %lld, D %lld)", (long long)N, (long long)M, (long long)D);
    HL_REQUIRE(kind == HL_FEAT_GRAM || kind == HL_FEAT_D2, "hl_feat_pairwise: kind %d is neither HL_FEAT_GRAM nor HL_FEAT_D2", kind);
    const size_t need = hl_feat_workspace_bytes(HL_FEAT_OP_PAIRWISE, N, M, 0, 0, 0);
    HL_REQUIRE(workspace && workspace_bytes >= need && aligned16({workspace}), "hl_feat_pairwise: workspace too small or unaligned (%zu bytes, need %zu)",
               workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    double *nx = static_cast<double *>(workspace), *ny = reinterpret_cast<double *>(static_cast<char *>(workspace) + pad16((size_t)N * 8));
    if (kind == HL_FEAT_D2) {
        int rc = norms(x, N, D, nx, st);
        if (rc == HL_OK) rc = norms(y, M, D, ny, st);
        if (rc != HL_OK) return rc;
    }
    const int64_t tcols = tiles_of(M);
    FEAT_LAUNCH(k_feat_pairwise, vec_ok(D, {x, y}), dim3((unsigned)(tiles_of(N) * tcols)), st, x, N, y, M, D, (const double *)nx, (const double *)ny,
                kind == HL_FEAT_D2 ? 1 : 0, tcols, out);
    return check_launch("k_feat_pairwise");
}

int hl_feat_kid(const float *x, int64_t N, const float *y, int64_t M, int64_t D, const int32_t *x_index, const int32_t *y_index, int64_t S, int64_t m,
                double *out, void *workspace, size_t workspace_bytes, void *stream) {
    HL_REQUIRE(x && y && x_index && y_index && out, "hl_feat_kid: NULL argument");
    HL_REQUIRE(sizes_ok(N, M, D), "hl_feat_kid: bad sizes (N %lld, M %lld, D %lld)", (long long)N, (long long)M, (long long)D);
    HL_REQUIRE(m >= 2 && m <= N && m <= M, "hl_feat_kid: subsets of %lld need 2 <= m <= min(N, M) = %lld", (long long)m, (long long)(N < M ? N : M));
    HL_REQUIRE(S >= 1 && S <= 65535, "hl_feat_kid: %lld subsets (1 .. 65535)", (long long)S);
    const size_t need = hl_feat_workspace_bytes(HL_FEAT_OP_KID, N, M, S, m, 0);
    HL_REQUIRE(need && workspace && workspace_bytes >= need && aligned16({workspace}), "hl_feat_kid: workspace too small or unaligned (%zu bytes, need %zu)",
               workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = tiles_of(m);
    double *partial = static_cast<double *>(workspace);
    FEAT_LAUNCH(k_feat_kid, vec_ok(D, {x, y}), dim3((unsigned)(tiles * tiles), (unsigned)S, 3), st, x, N, y, M, D, x_index, y_index, m, tiles, partial);
    int rc = check_launch("k_feat_kid");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_feat_kid_total, dim3((unsigned)S), dim3(kThreads), 0, st, (const double *)partial, tiles * tiles, m, out);
    return check_launch("k_feat_kid_total");
}

int hl_feat_knn_radii(const float *x, int64_t N, int64_t D, int k, int split, double *r2, void *workspace, size_t workspace_bytes, void *stream) {
    HL_REQUIRE(x && r2, "hl_feat_knn_radii: NULL argument");
    HL_REQUIRE(sizes_ok(N, N, D), "hl_feat_knn_radii: bad sizes (N %lld, D %lld)", (long long)N, (long long)D);
    HL_REQUIRE(k >= 1 && k <= HL_FEAT_MAX_K && k < N, "hl_feat_knn_radii: k = %d; 1 <= k <= %d and k < N = %lld", k, HL_FEAT_MAX_K, (long long)N);
    const size_t need = hl_feat_workspace_bytes(HL_FEAT_OP_KNN, N, N, 0, 0, split);
    HL_REQUIRE(workspace && workspace_bytes >= need && aligned16({workspace}), "hl_feat_knn_radii: workspace too small or unaligned (%zu bytes, need %zu)",
               workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    const int splits = resolve_split(N, N, split);
    double *nx = static_cast<double *>(workspace), *lists = reinterpret_cast<double *>(static_cast<char *>(workspace) + pad16((size_t)N * 8));
    int rc = norms(x, N, D, nx, st);
    if (rc != HL_OK) return rc;
    FEAT_LAUNCH(k_feat_knn, vec_ok(D, {x}), dim3((unsigned)tiles_of(N), (unsigned)splits), st, x, N, D, (const double *)nx, splits, lists);
    rc = check_launch("k_feat_knn");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_feat_knn_merge, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const double *)lists, N, splits, k, r2);
    return check_launch("k_feat_knn_merge");
}

int hl_feat_manifold(const float *real, int64_t N, const float *fake, int64_t M, int64_t D, const double *r2_real, const double *r2_fake, int split,
                     int32_t *hits_fake, int32_t *hits_real, double *nearest_real, void *workspace, size_t workspace_bytes, void *stream) {
    HL_REQUIRE(real && fake && r2_real && r2_fake && hits_fake && hits_real && nearest_real, "hl_feat_manifold: NULL argument");
    HL_REQUIRE(sizes_ok(N, M, D), "hl_feat_manifold: bad sizes (N %lld, M %lld, D %lld)", (long long)N, (long long)M, (long long)D);
    const size_t need = hl_feat_workspace_bytes(HL_FEAT_OP_MANIFOLD, N, M, 0, 0, 0);
    HL_REQUIRE(workspace && workspace_bytes >= need && aligned16({workspace}), "hl_feat_manifold: workspace too small or unaligned (%zu bytes, need %zu)",
               workspace_bytes, need);
    HL_REQUIRE((uintptr_t)nearest_real % 8 == 0, "hl_feat_manifold: nearest_real must be 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int splits = resolve_split(N, M, split);
    double *nr = static_cast<double *>(workspace), *nf = reinterpret_cast<double *>(static_cast<char *>(workspace) + pad16((size_t)N * 8));
    int rc = norms(real, N, D, nr, st);
    if (rc == HL_OK) rc = norms(fake, M, D, nf, st);
    if (rc != HL_OK) return rc;
    unsigned long long *nearest = reinterpret_cast<unsigned long long *>(nearest_real);
    const int64_t most = N > M ? N : M;
    hipLaunchKernelGGL(k_feat_manifold_init, dim3((unsigned)((most + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, hits_fake, M, hits_real, nearest, N);
    rc = check_launch("k_feat_manifold_init");
    if (rc != HL_OK) return rc;
    FEAT_LAUNCH(k_feat_manifold, vec_ok(D, {real, fake}), dim3((unsigned)tiles_of(N), (unsigned)splits), st, real, N, fake, M, D, (const double *)nr,
                (const double *)nf, r2_real, r2_fake, splits, hits_fake, hits_real, nearest);
    return check_launch("k_feat_manifold");
}

}  // extern "C"
