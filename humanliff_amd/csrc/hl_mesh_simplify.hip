// Simplifying a triangle mesh by vertex clustering with quadrics, MI355X (gfx950): (vertices, triangles, normals, colours), a cell size
// and an origin -> one vertex per occupied grid cell that a surviving triangle references, placed by the quadric error of the triangles
// that touch the cell (Lindstrom 2000), the triangles whose three corners fall into three different cells, once per oriented triple,
// and the map from input to output vertices.  Contract: DESIGN.md "Simplifying the mesh"; tests/mesh_simplify_restatement.py states it
// again in numpy.  All geometry is float64 in cell units q = (v - origin) / cell (-ffp-contract=off: a product and the sum it goes into
// are two roundings), every accumulation is a 64-bit integer sum in fixed point at 2^30 per unit, the duplicate test keeps the smallest
// triangle index of a key: nothing depends on scheduling, so a result has the same bits on every run and for any order of the triangles
// (their output order apart).  Integer atomics only (32-bit or, 64-bit add / compare-and-swap, 32-bit min), all vector; no float atomics.
//
// hl_mesh_simplify_bounds
//   k_simplify_bounds / k_simplify_bounds_finish: componentwise min and max of the valid vertices (finite, and no coordinate below the
//     origin when one is given): per-workgroup partials by the fixed tree, then one workgroup.  The host derives origin and extents.
// hl_mesh_simplify_count
//   k_simplify_mark:   a thread per vertex: ci = floor(q), key = (cz gy + cy) gx + cx (64-bit), atomicOr into the bitmap of cells;
//                      the key (or -1: no cell, status bit 0) is kept per vertex.
//   scan of the bitmap words' popcounts (hl_scan.h) -> rank of every word, counts[0] = clusters.
// hl_mesh_simplify_emit
//   k_simplify_ids:    cluster id = rank of the vertex's key among the occupied keys; the cluster's key is stored beside it.
//   k_simplify_members: count, sum of llrint(2^30 (q - centre)), of llrint(2^30 n), of the colours: 64-bit atomic adds.
//   k_simplify_quadrics: a thread per triangle; its plane goes once to each distinct cluster among its corners (10 atomic adds each).
//   k_simplify_insert: a thread per triangle with three different ids: rotate the smallest first, key = c0 << 42 | c1 << 21 | c2,
//                      open addressing (atomicCAS claims a slot, atomicMin keeps the smallest triangle index), probes bounded.
//   k_simplify_used:   a triangle survives when it is its key's smallest index; survivors flag their three clusters.
//   scan over the clusters -> new vertex index;  k_simplify_solve: a thread per surviving cluster, the representative by Cramer's rule;
//   scan over the triangles -> k_simplify_triangles writes the survivors in input order, renumbered;  k_simplify_vertex_map.
#include "hl_mesh.h"
#include "hl_scan.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = kMeshThreads;
static_assert(kThreads == kScanThreads, "the scans and reductions run workgroups of kThreads");
constexpr int kBoundsBlocks = HL_SIMPLIFY_BOUNDS_BLOCKS;
constexpr int kAccWords = HL_SIMPLIFY_ACC_WORDS;    // count, position x y z, normal x y z, colour r g b, quadric xx xy xz yy yz zz xd yd zd dd
constexpr int64_t kMaxCells = (int64_t)1 << 31;
constexpr int64_t kMaxClusters = (int64_t)1 << 21;
constexpr double kFix = 1073741824.0;               // 2^30
constexpr double kLambda = 1e-3;
constexpr unsigned long long kEmptyKey = ~0ull;
enum { kStatusVertex = 1, kStatusIndex = 2, kStatusTable = 4 };

struct Grid {
    double origin[3], cell[3];
    int64_t g[3];
    int has_origin;
};

inline bool grid_ok(const double *cell, const double *origin) {
    for (int a = 0; a < 3; ++a) {
        if (!(cell[a] > 0.0 && finite_host(cell[a]))) return false;
        if (origin && !finite_host(origin[a])) return false;
    }
    return true;
}

struct Layout {                                     // the scratch, in this order; every part a multiple of 16 bytes
    size_t vkey, acc, ckey, used, newidx, bitmap, rank, tkeys, tmin, slot, blocks, total;
    int64_t words, max_clusters, capacity;
};

inline Layout layout_of(int64_t N, int64_t T, int64_t cells) {
    Layout l;
    l.words = (cells + 31) / 32;
    l.max_clusters = N < cells ? N : cells;
    if (l.max_clusters > kMaxClusters) l.max_clusters = kMaxClusters;
    l.capacity = 64;
    while (l.capacity < 2 * T) l.capacity *= 2;
    const int64_t sb = scan_blocks(l.words > T ? l.words : T);      // (the cluster scan is no longer than the triangle or word scans need)
    const int64_t sbc = scan_blocks(l.max_clusters);
    l.vkey = 0;
    l.acc = l.vkey + up16((size_t)N * 4);
    l.ckey = l.acc + (size_t)l.max_clusters * kAccWords * 8;
    l.used = l.ckey + up16((size_t)l.max_clusters * 4);
    l.newidx = l.used + up16((size_t)l.max_clusters * 4);
    l.bitmap = l.newidx + up16((size_t)l.max_clusters * 4);
    l.rank = l.bitmap + up16((size_t)l.words * 4);
    l.tkeys = l.rank + up16((size_t)l.words * 4);
    l.tmin = l.tkeys + (size_t)l.capacity * 8;
    l.slot = l.tmin + up16((size_t)l.capacity * 4);
    l.blocks = l.slot + up16((size_t)T * 8);
    l.total = l.blocks + up16((size_t)(sb > sbc ? sb : sbc) * 8);
    return l;
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vertex_valid(const Grid &gr, const double (&v)[3]) {
    return finite3(v[0], v[1], v[2]) && (!gr.has_origin || (v[0] >= gr.origin[0] && v[1] >= gr.origin[1] && v[2] >= gr.origin[2]));
}

// partial (blocks, 6): min x y z, max x y z of the block's valid vertices (+inf / -inf where it has none)
__global__ __launch_bounds__(kThreads) void k_simplify_bounds(const double *__restrict__ vertices, int64_t N, const Grid gr, double *__restrict__ partial) {
    __shared__ double sh[kThreads];
    double lo[3] = {(double)INFINITY, (double)INFINITY, (double)INFINITY}, hi[3] = {-(double)INFINITY, -(double)INFINITY, -(double)INFINITY};
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += stride) {
        const double v[3] = {vertices[i * 3], vertices[i * 3 + 1], vertices[i * 3 + 2]};
        if (!vertex_valid(gr, v)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], v[a]), hi[a] = fmax(hi[a], v[a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double l = block_reduce(lo[a], sh, Min()), h = block_reduce(hi[a], sh, Max());
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * 6 + a] = l, partial[(int64_t)blockIdx.x * 6 + 3 + a] = h;
    }
}

__global__ __launch_bounds__(kThreads) void k_simplify_bounds_finish(const double *__restrict__ partial, int blocks, double *__restrict__ bounds) {
    __shared__ double sh[kThreads];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double l = (double)INFINITY, h = -(double)INFINITY;
        for (int b = threadIdx.x; b < blocks; b += kThreads) l = fmin(l, partial[b * 6 + a]), h = fmax(h, partial[b * 6 + 3 + a]);
        l = block_reduce(l, sh, Min()), h = block_reduce(h, sh, Max());
        if (threadIdx.x == 0) bounds[a] = l, bounds[3 + a] = h;
    }
}

// ---- cells ----------------------------------------------------------------------------------------------------------------------
// q = (v - origin) / cell and ci = floor(q) per axis; false: the vertex belongs to no cell
__device__ __forceinline__ bool cell_of(const Grid &gr, const double *__restrict__ vp, double (&q)[3], int64_t (&ci)[3]) {
    const double v[3] = {vp[0], vp[1], vp[2]};
    bool ok = finite3(v[0], v[1], v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = (v[a] - gr.origin[a]) / gr.cell[a];
        const double f = floor(q[a]);
        ok = ok && q[a] >= 0.0 && f < (double)gr.g[a];      // (past the extents: never indexed; the host derives them so that it cannot happen)
        ci[a] = ok ? (int64_t)f : 0;
    }
    return ok;
}

__global__ __launch_bounds__(kThreads) void k_simplify_mark(const double *__restrict__ vertices, int64_t N, const Grid gr, unsigned *__restrict__ bitmap,
                                                            int *__restrict__ vkey, int *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    double q[3];
    int64_t ci[3];
    if (!cell_of(gr, vertices + i * 3, q, ci)) {
        vkey[i] = -1;
        atomicOr(status, kStatusVertex);
        return;
    }
    const int64_t key = (ci[2] * gr.g[1] + ci[1]) * gr.g[0] + ci[0];      // < 2^31: the grid holds at most 2^31 cells
    atomicOr(bitmap + (key >> 5), 1u << (key & 31));
    vkey[i] = (int)key;
}

struct PopCount {
    const unsigned *bitmap;
    __device__ unsigned long long operator()(long i) const { return (unsigned long long)__popc(bitmap[i]); }
};
struct RankOut {
    unsigned *rank;
    __device__ void operator()(long i, unsigned long long run, unsigned long long) const { rank[i] = (unsigned)run; }
};

// vkey: the cell key of each vertex -> its cluster id, in place; ckey[id] = the key (every member stores the same value)
__global__ __launch_bounds__(kThreads) void k_simplify_ids(int *__restrict__ vkey, int64_t N, const unsigned *__restrict__ bitmap, const unsigned *__restrict__ rank,
                                                           int64_t clusters, int *__restrict__ ckey) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int key = vkey[i];
    if (key < 0) return;
    const unsigned w = (unsigned)key >> 5, b = (unsigned)key & 31u;
    const int64_t id = (int64_t)rank[w] + __popc(bitmap[w] & ((1u << b) - 1u));
    if (id >= clusters) {                           // (cannot happen: clusters is the bitmap's own popcount)
        vkey[i] = -1;
        return;
    }
    vkey[i] = (int)id;
    ckey[id] = key;
}

__device__ __forceinline__ void add64(int64_t *p, int64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);      // (two's complement: the unsigned add is the signed one)
}

// llrint(2^30 x), 0 for a non-finite x
__device__ __forceinline__ int64_t fix30(double x) { return fabs(x) < (double)INFINITY ? (int64_t)llrint(kFix * x) : 0; }

struct MeshIn {
    const double *vertices;                         // (N,3)
    const double *normals;                          // (N,3) or NULL
    const unsigned char *colors;                    // (N,3) or NULL
    const int *triangles;                           // (T,3)
    int64_t N, T;
};

__global__ __launch_bounds__(kThreads) void k_simplify_members(const MeshIn m, const Grid gr, const int *__restrict__ vid, int64_t *__restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m.N) return;
    const int id = vid[i];
    if (id < 0) return;
    double q[3];
    int64_t ci[3];
    if (!cell_of(gr, m.vertices + i * 3, q, ci)) return;
    int64_t *a = acc + (int64_t)id * kAccWords;
    add64(a, 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) add64(a + 1 + c, fix30(q[c] - ((double)ci[c] + 0.5)));
    if (m.normals) {
#pragma unroll
        for (int c = 0; c < 3; ++c) add64(a + 4 + c, fix30(m.normals[i * 3 + c]));
    }
    if (m.colors) {
#pragma unroll
        for (int c = 0; c < 3; ++c) add64(a + 7 + c, (int64_t)m.colors[i * 3 + c]);
    }
}

__global__ __launch_bounds__(kThreads) void k_simplify_quadrics(const MeshIn m, const Grid gr, const int *__restrict__ vid, int64_t *__restrict__ acc,
                                                                int *__restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m.T) return;
    int iv[3];
    if (!load_indices(m.triangles, t, m.N, iv)) {
        atomicOr(status, kStatusIndex);
        return;
    }
    const int id[3] = {vid[iv[0]], vid[iv[1]], vid[iv[2]]};
    if (id[0] < 0 || id[1] < 0 || id[2] < 0) return;
    double q[3][3];
    int64_t ci[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (!cell_of(gr, m.vertices + (int64_t)iv[k] * 3, q[k], ci[k])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // once per distinct cluster: at the first corner that lies in it, which is also the plane's point (|p| < 0.87: inside the cell)
        if ((k >= 1 && id[k] == id[0]) || (k == 2 && id[k] == id[1])) continue;
        double p[3][3];                             // the corners relative to this cluster's centre
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[j][c] = q[j][c] - ((double)ci[k][c] + 0.5);
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double l = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        if (!(l > 0.0 && l < (double)INFINITY)) continue;
        const double u[3] = {n[0] / l, n[1] / l, n[2] / l};
        const double d = -((u[0] * p[k][0] + u[1] * p[k][1]) + u[2] * p[k][2]);
        const double w = fmin(l / 2.0, 1.0);
        const double wu[3] = {w * u[0], w * u[1], w * u[2]}, wd = w * d;
        int64_t *a = acc + (int64_t)id[k] * kAccWords + 10;
        add64(a + 0, fix30(wu[0] * u[0])), add64(a + 1, fix30(wu[0] * u[1])), add64(a + 2, fix30(wu[0] * u[2]));
        add64(a + 3, fix30(wu[1] * u[1])), add64(a + 4, fix30(wu[1] * u[2])), add64(a + 5, fix30(wu[2] * u[2]));
        add64(a + 6, fix30(wu[0] * d)), add64(a + 7, fix30(wu[1] * d)), add64(a + 8, fix30(wu[2] * d));
        add64(a + 9, fix30(wd * d));
    }
}

// ---- triangles ------------------------------------------------------------------------------------------------------------------
// the three cluster ids of triangle t, rotated so that the smallest comes first; false: dropped (bad index, a vertex without a cell,
// two equal ids)
__device__ __forceinline__ bool triangle_ids(const MeshIn &m, const int *__restrict__ vid, int64_t t, int (&c)[3]) {
    int iv[3];
    if (!load_indices(m.triangles, t, m.N, iv)) return false;
    const int a = vid[iv[0]], b = vid[iv[1]], d = vid[iv[2]];
    if (a < 0 || b < 0 || d < 0 || a == b || b == d || a == d) return false;
    if (a < b && a < d)
        c[0] = a, c[1] = b, c[2] = d;
    else if (b < d)
        c[0] = b, c[1] = d, c[2] = a;
    else
        c[0] = d, c[1] = a, c[2] = b;
    return true;
}

struct Table {
    unsigned long long *keys;                       // (capacity) kEmptyKey where free
    unsigned *min_tri;                              // (capacity) the smallest triangle index that holds the slot's key
    int64_t capacity;                               // a power of two
    int shift;                                      // 64 - log2(capacity)
};

__global__ __launch_bounds__(kThreads) void k_simplify_insert(const MeshIn m, const int *__restrict__ vid, const Table tb, int64_t *__restrict__ slot_of,
                                                              int *__restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m.T) return;
    int c[3];
    int64_t found = -1;
    if (triangle_ids(m, vid, t, c)) {
        const unsigned long long key = ((unsigned long long)c[0] << 42) | ((unsigned long long)c[1] << 21) | (unsigned long long)c[2];
        const unsigned long long mask = (unsigned long long)tb.capacity - 1ull;
        unsigned long long s = (key * 0x9E3779B97F4A7C15ull) >> tb.shift;
        for (int64_t probe = 0; probe < tb.capacity; ++probe, s = (s + 1ull) & mask) {
            unsigned long long have = tb.keys[s];
            if (have == kEmptyKey) have = atomicCAS(tb.keys + s, kEmptyKey, key);
            if (have == kEmptyKey || have == key) {
                atomicMin(tb.min_tri + s, (unsigned)t);
                found = (int64_t)s;
                break;
            }
        }
        if (found < 0) atomicOr(status, kStatusTable);
    }
    slot_of[t] = found;
}

__device__ __forceinline__ bool survives(const int64_t *__restrict__ slot_of, const unsigned *__restrict__ min_tri, int64_t t) {
    const int64_t s = slot_of[t];
    return s >= 0 && min_tri[s] == (unsigned)t;
}

__global__ __launch_bounds__(kThreads) void k_simplify_used(const MeshIn m, const int *__restrict__ vid, const int64_t *__restrict__ slot_of,
                                                            const unsigned *__restrict__ min_tri, unsigned *__restrict__ used) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m.T || !survives(slot_of, min_tri, t)) return;
    int c[3];
    if (!triangle_ids(m, vid, t, c)) return;
    used[c[0]] = 1u, used[c[1]] = 1u, used[c[2]] = 1u;
}

struct UsedCount {
    const unsigned *used;
    __device__ unsigned long long operator()(long i) const { return used[i] ? 1ull : 0ull; }
};
struct NewIndexOut {
    int *newidx;
    __device__ void operator()(long i, unsigned long long run, unsigned long long v) const { newidx[i] = v ? (int)run : -1; }
};
struct SurvivorCount {
    const int64_t *slot_of;
    const unsigned *min_tri;
    __device__ unsigned long long operator()(long i) const { return survives(slot_of, min_tri, i) ? 1ull : 0ull; }
};
struct TriangleOut {
    MeshIn m;
    const int *vid, *newidx;
    int64_t *triangles;                             // (T,3), the first counts[2] rows written
    __device__ void operator()(long i, unsigned long long run, unsigned long long v) const {
        int c[3];
        if (!v || !triangle_ids(m, vid, i, c)) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) triangles[(int64_t)run * 3 + k] = (int64_t)newidx[c[k]];
    }
};

// ---- representatives ------------------------------------------------------------------------------------------------------------
struct SolveArgs {
    const int64_t *acc;
    const int *ckey, *newidx;
    int64_t clusters;
    Grid gr;
    double *vertices, *normals;                     // (V,3); normals or NULL
    unsigned char *colors;                          // (V,3) or NULL
};

__global__ __launch_bounds__(kThreads) void k_simplify_solve(const SolveArgs s) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= s.clusters) return;
    const int64_t o = s.newidx[c];
    if (o < 0) return;
    const int64_t *a = s.acc + c * kAccWords;
    const int64_t count = a[0];                     // >= 1: a cluster has a member
    const double cnt = (double)count;
    const double m[3] = {((double)a[1] / kFix) / cnt, ((double)a[2] / kFix) / cnt, ((double)a[3] / kFix) / cnt};
    const double Axx = (double)a[10] / kFix, Axy = (double)a[11] / kFix, Axz = (double)a[12] / kFix, Ayy = (double)a[13] / kFix, Ayz = (double)a[14] / kFix,
                 Azz = (double)a[15] / kFix;
    const double b[3] = {(double)a[16] / kFix, (double)a[17] / kFix, (double)a[18] / kFix};
    const double t = (Axx + Ayy) + Azz;
    double p[3] = {m[0], m[1], m[2]};
    if (t != 0.0) {
        const double eps = (kLambda * t) / 3.0;
        const double m00 = Axx + eps, m11 = Ayy + eps, m22 = Azz + eps, m01 = Axy, m02 = Axz, m12 = Ayz;
        const double r0 = ((Axx * m[0] + Axy * m[1]) + Axz * m[2]) + b[0], r1 = ((Axy * m[0] + Ayy * m[1]) + Ayz * m[2]) + b[1],
                     r2 = ((Axz * m[0] + Ayz * m[1]) + Azz * m[2]) + b[2];
        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11, c11 = m00 * m22 - m02 * m02,
                     c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double det = (m00 * c00 + m01 * c01) + m02 * c02;
        if (det > 0.0 && det < (double)INFINITY) {
            p[0] = m[0] - ((c00 * r0 + c01 * r1) + c02 * r2) / det;
            p[1] = m[1] - ((c01 * r0 + c11 * r1) + c12 * r2) / det;
            p[2] = m[2] - ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        }
    }
    int64_t key = s.ckey[c];
    int64_t ci[3];
    ci[0] = key % s.gr.g[0], key /= s.gr.g[0];
    ci[1] = key % s.gr.g[1], ci[2] = key / s.gr.g[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pk = fmin(fmax(p[k], -0.5), 0.5);
        s.vertices[o * 3 + k] = s.gr.origin[k] + (((double)ci[k] + 0.5) + pk) * s.gr.cell[k];
    }
    if (s.normals) {
        const double x = (double)a[4] / kFix, y = (double)a[5] / kFix, z = (double)a[6] / kFix;
        const double len = sqrt((x * x + y * y) + z * z);
        const bool ok = len > 0.0 && len < (double)INFINITY;
        s.normals[o * 3] = ok ? x / len : 0.0, s.normals[o * 3 + 1] = ok ? y / len : 0.0, s.normals[o * 3 + 2] = ok ? z / len : 0.0;
    }
    if (s.colors) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.colors[o * 3 + k] = (unsigned char)((2 * a[7 + k] + count) / (2 * count));      // round half up
    }
}

__global__ __launch_bounds__(kThreads) void k_simplify_vertex_map(const int *__restrict__ vid, const int *__restrict__ newidx, int64_t N, int64_t *__restrict__ vertex_map) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int id = vid[i];
    vertex_map[i] = id < 0 ? -1 : (int64_t)newidx[id];
}

inline Grid grid_of(const double *cell, const double *origin, int64_t gx, int64_t gy, int64_t gz) {
    Grid gr;
    for (int a = 0; a < 3; ++a) gr.cell[a] = cell[a], gr.origin[a] = origin ? origin[a] : 0.0;
    gr.g[0] = gx, gr.g[1] = gy, gr.g[2] = gz;
    gr.has_origin = origin != nullptr;
    return gr;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_mesh_simplify_bounds(const double *vertices, int64_t N, const double *h_origin, double *bounds, void *stream) {
    HL_REQUIRE(count_ok(N), "hl_mesh_simplify_bounds: bad vertex count %lld (1 .. 2^31 - 1)", (long long)N);
    HL_REQUIRE(!h_origin || origin_ok(h_origin), "hl_mesh_simplify_bounds: the origin must be finite");
    HL_REQUIRE(vertices && bounds, "hl_mesh_simplify_bounds: NULL argument");
    const double one[3] = {1.0, 1.0, 1.0};
    const Grid gr = grid_of(one, h_origin, 1, 1, 1);
    const int blocks = (int)(blocks_of(N) < kBoundsBlocks ? blocks_of(N) : kBoundsBlocks);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_simplify_bounds, dim3((unsigned)blocks), dim3(kThreads), 0, st, vertices, N, gr, bounds + 6);
    const int rc = check_launch("k_simplify_bounds");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_bounds_finish, dim3(1), dim3(kThreads), 0, st, (const double *)(bounds + 6), blocks, bounds);
    return check_launch("k_simplify_bounds_finish");
}

size_t hl_mesh_simplify_scratch_bytes(int64_t N, int64_t T, int64_t gx, int64_t gy, int64_t gz) {
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    return count_ok(N) && count_ok(T) && cells ? layout_of(N, T, cells).total : 0;
}

int hl_mesh_simplify_count(const double *vertices, int64_t N, int64_t T, const double *h_cell, const double *h_origin, int64_t gx, int64_t gy, int64_t gz,
                           int64_t *counts, int32_t *status, void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(count_ok(N) && count_ok(T), "hl_mesh_simplify_count: bad sizes (N %lld, T %lld; both 1 .. 2^31 - 1)", (long long)N, (long long)T);
    HL_REQUIRE(h_cell && h_origin && grid_ok(h_cell, h_origin), "hl_mesh_simplify_count: the cell must be positive and finite, the origin finite");
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    HL_REQUIRE(cells, "hl_mesh_simplify_count: a grid of %lld x %lld x %lld cells (each >= 1, at most 2^31 in all: use a larger cell)", (long long)gx,
               (long long)gy, (long long)gz);
    HL_REQUIRE(vertices && counts && status && scratch, "hl_mesh_simplify_count: NULL argument");
    const Layout l = layout_of(N, T, cells);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_simplify_count: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_simplify_count: scratch must be 16-byte aligned");
    char *base = static_cast<char *>(scratch);
    unsigned *bitmap = reinterpret_cast<unsigned *>(base + l.bitmap), *rank = reinterpret_cast<unsigned *>(base + l.rank);
    int *vkey = reinterpret_cast<int *>(base + l.vkey);
    unsigned long long *blocks = reinterpret_cast<unsigned long long *>(base + l.blocks);
    const hipStream_t st = (hipStream_t)stream;
    const Grid gr = grid_of(h_cell, h_origin, gx, gy, gz);
    HL_HIP(hipMemsetAsync(bitmap, 0, (size_t)l.words * 4, st));
    HL_HIP(hipMemsetAsync(status, 0, 4, st));
    HL_HIP(hipMemsetAsync(counts, 0, 6 * 8, st));
    hipLaunchKernelGGL(k_simplify_mark, dim3((unsigned)blocks_of(N)), dim3(kThreads), 0, st, vertices, N, gr, bitmap, vkey, status);
    int rc = check_launch("k_simplify_mark");
    if (rc != HL_OK) return rc;
    return scan_exclusive(PopCount{bitmap}, RankOut{rank}, (long)l.words, blocks, counts, st, "hl_mesh_simplify_count: scan");
}

int hl_mesh_simplify_emit(const double *vertices, const double *normals, const unsigned char *colors, int64_t N, const int32_t *triangles, int64_t T,
                          const double *h_cell, const double *h_origin, int64_t gx, int64_t gy, int64_t gz, int64_t clusters, double *out_vertices,
                          double *out_normals, unsigned char *out_colors, int64_t *out_triangles, int64_t *vertex_map, int64_t *counts, int32_t *status,
                          void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(count_ok(N) && count_ok(T), "hl_mesh_simplify_emit: bad sizes (N %lld, T %lld; both 1 .. 2^31 - 1)", (long long)N, (long long)T);
    HL_REQUIRE(h_cell && h_origin && grid_ok(h_cell, h_origin), "hl_mesh_simplify_emit: the cell must be positive and finite, the origin finite");
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    HL_REQUIRE(cells, "hl_mesh_simplify_emit: a grid of %lld x %lld x %lld cells (each >= 1, at most 2^31 in all: use a larger cell)", (long long)gx,
               (long long)gy, (long long)gz);
    HL_REQUIRE(clusters <= kMaxClusters, "hl_mesh_simplify_emit: %lld clusters, at most 2^21 (use a larger cell)", (long long)clusters);
    HL_REQUIRE(clusters >= 1 && clusters <= N && clusters <= cells, "hl_mesh_simplify_emit: %lld clusters of %lld vertices in %lld cells", (long long)clusters,
               (long long)N, (long long)cells);
    HL_REQUIRE(vertices && triangles && out_vertices && out_triangles && vertex_map && counts && status && scratch, "hl_mesh_simplify_emit: NULL argument");
    HL_REQUIRE((!normals) == (!out_normals) && (!colors) == (!out_colors), "hl_mesh_simplify_emit: normals / colors go in and out together");
    const Layout l = layout_of(N, T, cells);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_simplify_emit: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_simplify_emit: scratch must be 16-byte aligned");
    char *base = static_cast<char *>(scratch);
    int *vid = reinterpret_cast<int *>(base + l.vkey), *ckey = reinterpret_cast<int *>(base + l.ckey), *newidx = reinterpret_cast<int *>(base + l.newidx);
    int64_t *acc = reinterpret_cast<int64_t *>(base + l.acc), *slot_of = reinterpret_cast<int64_t *>(base + l.slot);
    unsigned *used = reinterpret_cast<unsigned *>(base + l.used), *bitmap = reinterpret_cast<unsigned *>(base + l.bitmap),
             *rank = reinterpret_cast<unsigned *>(base + l.rank);
    unsigned long long *blocks = reinterpret_cast<unsigned long long *>(base + l.blocks);
    Table tb;
    tb.keys = reinterpret_cast<unsigned long long *>(base + l.tkeys), tb.min_tri = reinterpret_cast<unsigned *>(base + l.tmin), tb.capacity = l.capacity;
    tb.shift = 64;
    for (int64_t c = l.capacity; c > 1; c >>= 1) --tb.shift;
    const hipStream_t st = (hipStream_t)stream;
    const Grid gr = grid_of(h_cell, h_origin, gx, gy, gz);
    MeshIn m;
    m.vertices = vertices, m.normals = normals, m.colors = colors, m.triangles = triangles, m.N = N, m.T = T;
    const dim3 bt(kThreads), gn((unsigned)blocks_of(N)), gt((unsigned)blocks_of(T)), gc((unsigned)blocks_of(clusters));

    HL_HIP(hipMemsetAsync(acc, 0, (size_t)clusters * kAccWords * 8, st));
    HL_HIP(hipMemsetAsync(used, 0, (size_t)clusters * 4, st));
    HL_HIP(hipMemsetAsync(tb.keys, 0xff, (size_t)l.capacity * 8, st));
    HL_HIP(hipMemsetAsync(tb.min_tri, 0xff, (size_t)l.capacity * 4, st));

    hipLaunchKernelGGL(k_simplify_ids, gn, bt, 0, st, vid, N, (const unsigned *)bitmap, (const unsigned *)rank, clusters, ckey);
    int rc = check_launch("k_simplify_ids");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_members, gn, bt, 0, st, m, gr, (const int *)vid, acc);
    rc = check_launch("k_simplify_members");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_quadrics, gt, bt, 0, st, m, gr, (const int *)vid, acc, status);
    rc = check_launch("k_simplify_quadrics");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_insert, gt, bt, 0, st, m, (const int *)vid, tb, slot_of, status);
    rc = check_launch("k_simplify_insert");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_used, gt, bt, 0, st, m, (const int *)vid, (const int64_t *)slot_of, (const unsigned *)tb.min_tri, used);
    rc = check_launch("k_simplify_used");
    if (rc != HL_OK) return rc;

    // surviving clusters -> new vertex indices (counts[4]), then their representatives
    rc = scan_exclusive(UsedCount{used}, NewIndexOut{newidx}, (long)clusters, blocks, counts + 4, st, "hl_mesh_simplify_emit: cluster scan");
    if (rc != HL_OK) return rc;
    SolveArgs sa;
    sa.acc = acc, sa.ckey = ckey, sa.newidx = newidx, sa.clusters = clusters, sa.gr = gr, sa.vertices = out_vertices, sa.normals = out_normals,
    sa.colors = out_colors;
    hipLaunchKernelGGL(k_simplify_solve, gc, bt, 0, st, sa);
    rc = check_launch("k_simplify_solve");
    if (rc != HL_OK) return rc;

    // surviving triangles, in input order (counts[2])
    rc = scan_exclusive(SurvivorCount{slot_of, tb.min_tri}, TriangleOut{m, vid, newidx, out_triangles}, (long)T, blocks, counts + 2, st,
                        "hl_mesh_simplify_emit: triangle scan");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_simplify_vertex_map, gn, bt, 0, st, (const int *)vid, (const int *)newidx, N, vertex_map);
    return check_launch("k_simplify_vertex_map");
}

}  // extern "C"
