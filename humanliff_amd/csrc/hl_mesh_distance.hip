// Measuring the distance from points to a triangle mesh, MI355X (gfx950): for every query point the exact closest point of the mesh -
// squared distance, triangle, barycentrics, the point itself and optionally the cosine between the query's normal and the hit
// triangle's - found through a uniform grid of cubic cells over the mesh; a deterministic surface sampler (area-weighted, the R2
// sequence in integers); and the fixed-order sums the scores are made of.  Contract: DESIGN.md "Measuring mesh distance";
// tests/mesh_distance_restatement.py states it again in numpy.  All geometry is float64 relative to an origin o (the lower corner of
// the mesh's bounds), -ffp-contract=off: a product and the sum it goes into are two roundings.  Between triangles the smallest
// (d2, triangle index) wins, so the answer does not depend on the order in which triangles are visited, on the cell size or on
// scheduling; areas are 64-bit integers.  Integer atomics only (32-bit add / or), all vector; no float atomics.
//
// hl_mesh_distance_areas
//   k_dist_area:    a thread per triangle: a_i = llrint((sqrt(nn) / 2) / unit), 0 for an invalid or degenerate triangle.
//   scan (hl_scan.h), in place -> the exclusive prefix P, counts[0] | counts[1] << 32 = the total.
// hl_mesh_distance_count
//   k_dist_records: a thread per triangle: validate, gather the corners relative to o into a record of ten doubles (80 bytes), the
//                   box of cells floor(min / h) .. floor(max / h); more than kWideCells cells: wide (flag 2), otherwise flag 1 and
//                   one atomicAdd per cell of the box.  Invalid: flag 0 and a status bit; never dereferenced.
//   scan over the cells, in place -> the start of every cell's list, counts[0] | counts[1] << 32 = references in all;
//   scan over the triangles -> the wide list in index order, counts[2] = wide triangles, counts[3] = valid triangles.
// hl_mesh_distance_fill
//   k_dist_fill:    a thread per registered triangle: refs[start[key] + atomicAdd(cursor[key], 1)] = t for every cell of its box.
// hl_mesh_distance_query
//   k_dist_query:   a thread per query: the wide list, then rings r = 0, 1, ... of cells at Chebyshev distance r around the query's
//                   (clamped) cell until the best squared distance is within the visited block.  A row of a ring's face is one
//                   contiguous range of references.  The winner is evaluated once more for its barycentrics and point.
// hl_mesh_distance_sample
//   k_dist_sample:  a thread per sample: stratified position in the area prefix, binary search, R2 barycentrics.
// hl_mesh_distance_reduce
//   k_dist_reduce / k_dist_reduce_finish: per-workgroup partials by the fixed tree, then strided_sum in one workgroup.
#include "hl_mesh.h"
#include "hl_scan.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = kMeshThreads;
static_assert(kThreads == kScanThreads, "the scans and reductions run workgroups of kThreads");
constexpr int64_t kMaxCells = (int64_t)1 << 27;
constexpr int64_t kMaxRefs = (int64_t)1 << 31;
constexpr int64_t kWideCells = HL_DISTANCE_WIDE_CELLS;
constexpr int64_t kMaxWide = HL_DISTANCE_MAX_WIDE;
constexpr int kRecWords = HL_DISTANCE_RECORD_WORDS;
constexpr int kReduceBlocks = HL_DISTANCE_REDUCE_BLOCKS;
constexpr int kReduceWords = HL_DISTANCE_REDUCE_FIELDS;       // sum d, sum d2, sum normal_dot, count normal_dot, max d, count, 2 spare, within[8]
constexpr int kMaxThresholds = 8;
constexpr double kInf = (double)INFINITY;
constexpr double kSlack = 9.5367431640625e-07;                // 2^-20 of a cell
enum { kStatusIndex = 1, kStatusCorner = 2, kStatusQuery = 4 };

struct Layout {                                     // the scratch, in this order; every part a multiple of 16 bytes
    size_t rec, flag, start, cursor, wide, blocks, total;
};

inline Layout layout_of(int64_t T, int64_t cells) {
    Layout l;
    const int64_t longest = cells + 1 > T ? cells + 1 : T;
    l.rec = 0;
    l.flag = l.rec + (size_t)T * kRecWords * 8;
    l.start = l.flag + up16((size_t)T * 4);
    l.cursor = l.start + up16((size_t)(cells + 1) * 4);
    l.wide = l.cursor + up16((size_t)cells * 4);
    l.blocks = l.wide + (size_t)kMaxWide * 4;
    l.total = l.blocks + up16((size_t)scan_blocks(longest) * 8);
    return l;
}

struct Grid {
    double origin[3], h;
    int g[3];                                       // each <= 2^27
};

inline Grid grid_of(const double *origin, double h, int64_t gx, int64_t gy, int64_t gz) {
    Grid gr;
    for (int a = 0; a < 3; ++a) gr.origin[a] = origin[a];
    gr.h = h;
    gr.g[0] = (int)gx, gr.g[1] = (int)gy, gr.g[2] = (int)gz;
    return gr;
}

// ---- arithmetic -----------------------------------------------------------------------------------------------------------------
struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 sub(const V3 &a, const V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 &a, const V3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ bool finite(double x) { return fabs(x) < kInf; }      // (false for NaN)

struct Closest {
    double d2;
    V3 x, bary;
};

// the closest point of the segment a + t e, t in [0, 1]
__device__ __forceinline__ double seg(const V3 &p, const V3 &a, const V3 &e, double &t, V3 &x) {
    const double l = dot(e, e);
    t = dot(sub(p, a), e);
    t = l > 0.0 ? t / l : 0.0;
    t = t > 0.0 ? t : 0.0;                          // (min(max(t, 0), 1) with the sign of a zero fixed)
    t = t < 1.0 ? t : 1.0;
    x = {a.x + t * e.x, a.y + t * e.y, a.z + t * e.z};
    const V3 r = sub(p, x);
    return dot(r, r);
}

// The closest point of triangle (a, b, c) to p without a branch: the three edges, then the interior where the projection falls into
// it; the first candidate in that order wins a tie.  Every candidate is a point of the triangle, so a degenerate triangle gives the
// distance to its segment or point.  FULL: also the point and its barycentrics.
template <bool FULL>
__device__ __forceinline__ Closest closest_point(const V3 &p, const V3 &a, const V3 &b, const V3 &c) {
    const V3 ab = sub(b, a), bc = sub(c, b), ca = sub(a, c), ac = sub(c, a);
    double t0, t1, t2;
    V3 x0, x1, x2;
    const double d0 = seg(p, a, ab, t0, x0), d1 = seg(p, b, bc, t1, x1), d2 = seg(p, c, ca, t2, x2);
    const V3 n = cross(ab, ac);
    const double nn = dot(n, n);
    const V3 ap = sub(p, a);
    const double v = dot(cross(ap, ac), n) / nn, w = dot(cross(ab, ap), n) / nn;
    const bool inside = nn > 0.0 && finite(nn) && v >= 0.0 && w >= 0.0 && v + w <= 1.0;
    const V3 x3 = {a.x + (v * ab.x + w * ac.x), a.y + (v * ab.y + w * ac.y), a.z + (v * ab.z + w * ac.z)};
    const V3 r3 = sub(p, x3);
    const double d3 = inside ? dot(r3, r3) : kInf;
    Closest out;
    int win = 0;
    out.d2 = d0;
    if (d1 < out.d2) out.d2 = d1, win = 1;
    if (d2 < out.d2) out.d2 = d2, win = 2;
    if (d3 < out.d2) out.d2 = d3, win = 3;
    if (FULL) {
        out.x = win == 0 ? x0 : win == 1 ? x1 : win == 2 ? x2 : x3;
        const V3 e0 = {1.0 - t0, t0, 0.0}, e1 = {0.0, 1.0 - t1, t1}, e2 = {t2, 0.0, 1.0 - t2}, e3 = {(1.0 - v) - w, v, w};
        out.bary = win == 0 ? e0 : win == 1 ? e1 : win == 2 ? e2 : e3;
    }
    return out;
}

// ---- the mesh -------------------------------------------------------------------------------------------------------------------
struct MeshIn {
    const double *vertices;                         // (N,3) world
    const int *triangles;                           // (T,3)
    int64_t N, T;
    double origin[3];
};

// the corners of triangle t relative to the origin; 0: valid, otherwise the status bit (an index outside [0, N) is never dereferenced)
__device__ __forceinline__ int load_corners(const MeshIn &m, int64_t t, V3 (&p)[3]) {
    int iv[3];
    if (!load_indices(m.triangles, t, m.N, iv)) return kStatusIndex;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *vp = m.vertices + (int64_t)iv[k] * 3;
        const V3 v = {vp[0], vp[1], vp[2]};
        ok = ok && finite3(v.x, v.y, v.z);
        p[k] = {v.x - m.origin[0], v.y - m.origin[1], v.z - m.origin[2]};
    }
    return ok ? 0 : kStatusCorner;
}

// ---- areas ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dist_area(const MeshIn m, double unit, unsigned long long *__restrict__ prefix) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m.T) return;
    V3 p[3];
    unsigned long long a = 0;
    if (load_corners(m, t, p) == 0) {
        const V3 n = cross(sub(p[1], p[0]), sub(p[2], p[0]));
        const double q = (sqrt(dot(n, n)) / 2.0) / unit;
        if (q >= 0.0 && q < 2147483648.0) a = (unsigned long long)llrint(q);      // (a triangle inside the bounds stays below 0.87 * 2^30)
    }
    prefix[t] = a;
}

struct AreaIn {
    const unsigned long long *prefix;
    __device__ unsigned long long operator()(long i) const { return prefix[i]; }
};
struct AreaOut {
    unsigned long long *prefix;
    __device__ void operator()(long i, unsigned long long run, unsigned long long) const { prefix[i] = run; }
};

// ---- registration ---------------------------------------------------------------------------------------------------------------
struct Box {
    int lo[3], hi[3];
};

// the cells floor(min / h) .. floor(max / h) of a record, clamped to the grid (the host derives the extents so that nothing is cut)
__device__ __forceinline__ Box box_of(const Grid &gr, const V3 (&p)[3]) {
    Box b;
    const double lo[3] = {fmin(fmin(p[0].x, p[1].x), p[2].x), fmin(fmin(p[0].y, p[1].y), p[2].y), fmin(fmin(p[0].z, p[1].z), p[2].z)};
    const double hi[3] = {fmax(fmax(p[0].x, p[1].x), p[2].x), fmax(fmax(p[0].y, p[1].y), p[2].y), fmax(fmax(p[0].z, p[1].z), p[2].z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double top = (double)(gr.g[a] - 1);
        b.lo[a] = (int)fmin(fmax(floor(lo[a] / gr.h), 0.0), top);
        b.hi[a] = (int)fmin(fmax(floor(hi[a] / gr.h), 0.0), top);
    }
    return b;
}

__device__ __forceinline__ int64_t box_cells(const Box &b) {
    return ((int64_t)(b.hi[0] - b.lo[0] + 1) * (int64_t)(b.hi[1] - b.lo[1] + 1)) * (int64_t)(b.hi[2] - b.lo[2] + 1);      // (<= 2^27)
}

__device__ __forceinline__ int64_t key_of(const Grid &gr, int cx, int cy, int cz) { return ((int64_t)cz * gr.g[1] + cy) * gr.g[0] + cx; }

__device__ __forceinline__ void load_record(const double *__restrict__ rec, int64_t t, V3 (&p)[3]) {
    const double2 *r = reinterpret_cast<const double2 *>(rec + t * kRecWords);
    const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    p[0] = {r0.x, r0.y, r1.x}, p[1] = {r1.y, r2.x, r2.y}, p[2] = {r3.x, r3.y, r4.x};
}

__global__ __launch_bounds__(kThreads) void k_dist_records(const MeshIn m, const Grid gr, double *__restrict__ rec, int *__restrict__ flag,
                                                           unsigned *__restrict__ count, int *__restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m.T) return;
    V3 p[3];
    const int bad = load_corners(m, t, p);
    double *r = rec + t * kRecWords;
    if (bad) {
#pragma unroll
        for (int k = 0; k < kRecWords; ++k) r[k] = 0.0;
        flag[t] = 0;
        atomicOr(status, bad);
        return;
    }
    r[0] = p[0].x, r[1] = p[0].y, r[2] = p[0].z, r[3] = p[1].x, r[4] = p[1].y, r[5] = p[1].z, r[6] = p[2].x, r[7] = p[2].y, r[8] = p[2].z, r[9] = 0.0;
    const Box b = box_of(gr, p);
    if (box_cells(b) > kWideCells) {
        flag[t] = 2;
        return;
    }
    flag[t] = 1;
    for (int cz = b.lo[2]; cz <= b.hi[2]; ++cz)
        for (int cy = b.lo[1]; cy <= b.hi[1]; ++cy)
            for (int cx = b.lo[0]; cx <= b.hi[0]; ++cx) atomicAdd(count + key_of(gr, cx, cy, cz), 1u);
}

struct CellIn {
    const unsigned *start;
    __device__ unsigned long long operator()(long i) const { return (unsigned long long)start[i]; }
};
struct CellOut {
    unsigned *start;
    __device__ void operator()(long i, unsigned long long run, unsigned long long) const {
        start[i] = run < 0xffffffffull ? (unsigned)run : 0xffffffffu;      // (more than 2^31 references are refused before anything reads this)
    }
};
struct FlagIn {                                     // low half: wide, high half: valid
    const int *flag;
    __device__ unsigned long long operator()(long i) const {
        const int f = flag[i];
        return (f == 2 ? 1ull : 0ull) | (f != 0 ? 1ull << 32 : 0ull);
    }
};
struct WideOut {
    int *wide;
    __device__ void operator()(long i, unsigned long long run, unsigned long long v) const {
        const unsigned long long at = run & 0xffffffffull;
        if ((v & 1ull) && at < (unsigned long long)kMaxWide) wide[at] = (int)i;
    }
};

__global__ __launch_bounds__(kThreads) void k_dist_fill(const double *__restrict__ rec, const int *__restrict__ flag, int64_t T, const Grid gr,
                                                        const unsigned *__restrict__ start, unsigned *__restrict__ cursor, int *__restrict__ refs,
                                                        int64_t n_refs) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T || flag[t] != 1) return;
    V3 p[3];
    load_record(rec, t, p);
    const Box b = box_of(gr, p);
    for (int cz = b.lo[2]; cz <= b.hi[2]; ++cz)
        for (int cy = b.lo[1]; cy <= b.hi[1]; ++cy)
            for (int cx = b.lo[0]; cx <= b.hi[0]; ++cx) {
                const int64_t key = key_of(gr, cx, cy, cz);
                const int64_t at = (int64_t)start[key] + (int64_t)atomicAdd(cursor + key, 1u);
                if (at < n_refs) refs[at] = (int)t;      // (always: the counts are this loop's own)
            }
}

// ---- query ----------------------------------------------------------------------------------------------------------------------
struct QueryArgs {
    const double *points;                           // (Q,3) world
    const double *normals;                          // (Q,3) or NULL
    int64_t Q, T;
    Grid gr;
    const double *rec;
    const unsigned *start;
    const int *refs;
    int64_t n_refs;
    const int *wide;
    int n_wide;
    double max_distance;                            // +inf: none
    double *sqdist, *distance, *bary, *point, *normal_dot;
    int *triangle;
    int *status;
};

struct Best {
    double d2;
    int tri;
};

__device__ __forceinline__ void test_triangle(const QueryArgs &q, const V3 &p, int t, Best &best) {
    if (t < 0 || t >= q.T) return;                  // (cannot happen: the lists hold what k_dist_fill wrote)
    V3 c[3];
    load_record(q.rec, t, c);
    const double d2 = closest_point<false>(p, c[0], c[1], c[2]).d2;
    if (d2 < best.d2 || (d2 == best.d2 && t < best.tri)) best.d2 = d2, best.tri = t;
}

__device__ __forceinline__ void test_cells(const QueryArgs &q, const V3 &p, int64_t key0, int64_t key1, Best &best) {
    int64_t i = q.start[key0], end = q.start[key1 + 1];
    if (end > q.n_refs) end = q.n_refs;
    for (; i < end; ++i) test_triangle(q, p, q.refs[i], best);
}

__global__ __launch_bounds__(kThreads) void k_dist_query(const QueryArgs q) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.Q) return;
    const Grid &gr = q.gr;
    const V3 w = {q.points[i * 3], q.points[i * 3 + 1], q.points[i * 3 + 2]};
    const double nan = __builtin_nan("");
    if (!finite3(w.x, w.y, w.z)) {
        q.sqdist[i] = nan, q.distance[i] = nan, q.triangle[i] = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) q.bary[i * 3 + k] = nan, q.point[i * 3 + k] = nan;
        if (q.normal_dot) q.normal_dot[i] = nan;
        atomicOr(q.status, kStatusQuery);
        return;
    }
    const V3 p = {w.x - gr.origin[0], w.y - gr.origin[1], w.z - gr.origin[2]};
    const double pa[3] = {p.x, p.y, p.z};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = (int)fmin(fmax(floor(pa[a] / gr.h), 0.0), (double)(gr.g[a] - 1));
    Best best = {kInf, 0x7fffffff};
    for (int k = 0; k < q.n_wide; ++k) test_triangle(q, p, q.wide[k], best);
    const int rmax = max(max(gr.g[0], gr.g[1]), gr.g[2]);
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, gr.g[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, gr.g[1] - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, gr.g[0] - 1);
        for (int cz = z0; cz <= z1; ++cz)
            for (int cy = y0; cy <= y1; ++cy) {
                const int64_t row = key_of(gr, 0, cy, cz);
                if (cz == c[2] - r || cz == c[2] + r || cy == c[1] - r || cy == c[1] + r) {
                    test_cells(q, p, row + x0, row + x1, best);
                } else {
                    if (c[0] - r >= 0) test_cells(q, p, row + (c[0] - r), row + (c[0] - r), best);
                    if (c[0] + r <= gr.g[0] - 1) test_cells(q, p, row + (c[0] + r), row + (c[0] + r), best);
                }
            }
        double s = kInf;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) s = fmin(s, pa[a] - (double)(c[a] - r) * gr.h);
            if (c[a] + r < gr.g[a] - 1) s = fmin(s, (double)(c[a] + r + 1) * gr.h - pa[a]);
        }
        if (s == kInf) break;                       // no side counts: everything was visited
        const double sm = fmax(s - gr.h * kSlack, 0.0);
        if (best.d2 <= sm * sm || sm >= q.max_distance) break;
    }
    double dist = sqrt(best.d2);
    if (best.tri == 0x7fffffff || dist > q.max_distance) {
        q.sqdist[i] = kInf, q.distance[i] = kInf, q.triangle[i] = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) q.bary[i * 3 + k] = nan, q.point[i * 3 + k] = nan;
        if (q.normal_dot) q.normal_dot[i] = nan;
        return;
    }
    V3 t[3];
    load_record(q.rec, best.tri, t);
    const Closest hit = closest_point<true>(p, t[0], t[1], t[2]);
    q.sqdist[i] = hit.d2, q.distance[i] = sqrt(hit.d2), q.triangle[i] = best.tri;
    q.bary[i * 3] = hit.bary.x, q.bary[i * 3 + 1] = hit.bary.y, q.bary[i * 3 + 2] = hit.bary.z;
    q.point[i * 3] = hit.x.x + gr.origin[0], q.point[i * 3 + 1] = hit.x.y + gr.origin[1], q.point[i * 3 + 2] = hit.x.z + gr.origin[2];
    if (q.normals) {
        const V3 nq = {q.normals[i * 3], q.normals[i * 3 + 1], q.normals[i * 3 + 2]};
        const V3 n = cross(sub(t[1], t[0]), sub(t[2], t[0]));
        const double len = sqrt(dot(n, n));
        const bool ok = len > 0.0 && finite(len) && finite3(nq.x, nq.y, nq.z) && !(nq.x == 0.0 && nq.y == 0.0 && nq.z == 0.0);
        const V3 u = {n.x / len, n.y / len, n.z / len};
        q.normal_dot[i] = ok ? dot(nq, u) : nan;
    }
}

// ---- samples --------------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    MeshIn m;
    const unsigned long long *prefix;               // (T) exclusive
    unsigned long long total;
    int64_t S;
    unsigned long long seed;
    double *points, *bary, *normals;                // (S,3)
    int64_t *triangle;                              // (S)
};

__global__ __launch_bounds__(kThreads) void k_dist_sample(const SampleArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= a.S) return;
    unsigned long long k = (unsigned long long)floor((((double)s + 0.5) / (double)a.S) * (double)a.total);
    if (k > a.total - 1ull) k = a.total - 1ull;
    int64_t lo = 0, hi = a.m.T - 1;                 // the largest i with prefix[i] <= k (prefix[0] = 0)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (a.prefix[mid] <= k) lo = mid; else hi = mid - 1;
    }
    const unsigned long long mm = (a.seed << 32) + (unsigned long long)s + 1ull;
    double u1 = (double)((mm * 0xC13FA9A902A6328Full) >> 11) * 1.1102230246251565e-16;      // 2^-53
    double u2 = (double)((mm * 0x91E10DA5C79E7B1Dull) >> 11) * 1.1102230246251565e-16;
    if (u1 + u2 > 1.0) u1 = 1.0 - u1, u2 = 1.0 - u2;
    V3 p[3];
    const double nan = __builtin_nan("");
    if (load_corners(a.m, lo, p) != 0) {            // (cannot happen: an invalid triangle has area 0 and is never chosen)
        a.triangle[s] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.points[s * 3 + c] = nan, a.bary[s * 3 + c] = nan, a.normals[s * 3 + c] = nan;
        return;
    }
    const V3 ab = sub(p[1], p[0]), ac = sub(p[2], p[0]);
    const V3 x = {p[0].x + (u1 * ab.x + u2 * ac.x), p[0].y + (u1 * ab.y + u2 * ac.y), p[0].z + (u1 * ab.z + u2 * ac.z)};
    const V3 n = cross(ab, ac);
    const double len = sqrt(dot(n, n));
    a.triangle[s] = lo;
    a.points[s * 3] = x.x + a.m.origin[0], a.points[s * 3 + 1] = x.y + a.m.origin[1], a.points[s * 3 + 2] = x.z + a.m.origin[2];
    a.bary[s * 3] = (1.0 - u1) - u2, a.bary[s * 3 + 1] = u1, a.bary[s * 3 + 2] = u2;
    a.normals[s * 3] = n.x / len, a.normals[s * 3 + 1] = n.y / len, a.normals[s * 3 + 2] = n.z / len;
}

// ---- sums -----------------------------------------------------------------------------------------------------------------------
struct ReduceArgs {
    const double *distance, *sqdist, *normal_dot;   // (Q); normal_dot or NULL
    int64_t Q;
    int n_thresholds;
    double thresholds[kMaxThresholds];
};

// partial (blocks, kReduceWords); a query whose distance is not finite counts nowhere
__global__ __launch_bounds__(kThreads) void k_dist_reduce(const ReduceArgs a, double *__restrict__ partial) {
    __shared__ double sh[kThreads];
    double acc[kReduceWords];
#pragma unroll
    for (int k = 0; k < kReduceWords; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.Q; i += stride) {
        const double d = a.distance[i];
        if (!finite(d)) continue;
        acc[0] += d, acc[1] += a.sqdist[i], acc[4] = fmax(acc[4], d), acc[5] += 1.0;
        if (a.normal_dot) {
            const double nd = a.normal_dot[i];
            if (finite(nd)) acc[2] += nd, acc[3] += 1.0;
        }
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k)
            if (k < a.n_thresholds && d <= a.thresholds[k]) acc[8 + k] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < kReduceWords; ++k) {
        const double v = k == 4 ? block_reduce(acc[k], sh, Max()) : block_sum(acc[k], sh);
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * kReduceWords + k] = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_dist_reduce_finish(const double *__restrict__ partial, int blocks, double *__restrict__ out) {
    __shared__ double sh[kThreads];
#pragma unroll
    for (int k = 0; k < kReduceWords; ++k) {
        double v;
        if (k == 4) {
            double m = 0.0;
            for (int b = threadIdx.x; b < blocks; b += kThreads) m = fmax(m, partial[(int64_t)b * kReduceWords + k]);
            v = block_reduce(m, sh, Max());
        } else {
            v = strided_sum(partial + k, blocks, kReduceWords, sh);
        }
        if (threadIdx.x == 0) out[k] = v;
    }
}

inline MeshIn mesh_of(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *origin) {
    MeshIn m;
    m.vertices = vertices, m.triangles = triangles, m.N = N, m.T = T;
    for (int a = 0; a < 3; ++a) m.origin[a] = origin[a];
    return m;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

size_t hl_mesh_distance_scratch_bytes(int64_t T, int64_t gx, int64_t gy, int64_t gz) {
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    return count_ok(T) && cells ? layout_of(T, cells).total : 0;
}

int hl_mesh_distance_areas(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, double unit, int64_t *prefix,
                           int64_t *counts, void *blocks, size_t blocks_bytes, void *stream) {
    HL_REQUIRE(count_ok(N) && count_ok(T), "hl_mesh_distance_areas: bad sizes (N %lld, T %lld; both 1 .. 2^31 - 1)", (long long)N, (long long)T);
    HL_REQUIRE(origin_ok(h_origin), "hl_mesh_distance_areas: the origin must be finite");
    HL_REQUIRE(unit > 0.0 && finite_host(unit), "hl_mesh_distance_areas: the area unit must be positive and finite");
    HL_REQUIRE(vertices && triangles && prefix && counts && blocks, "hl_mesh_distance_areas: NULL argument");
    HL_REQUIRE(blocks_bytes >= (size_t)scan_blocks(T) * 8, "hl_mesh_distance_areas: block sums too small (%zu bytes, need %zu)", blocks_bytes,
               (size_t)scan_blocks(T) * 8);
    const hipStream_t st = (hipStream_t)stream;
    const MeshIn m = mesh_of(vertices, N, triangles, T, h_origin);
    unsigned long long *pre = reinterpret_cast<unsigned long long *>(prefix), *bl = static_cast<unsigned long long *>(blocks);
    hipLaunchKernelGGL(k_dist_area, dim3((unsigned)blocks_of(T)), dim3(kThreads), 0, st, m, unit, pre);
    int rc = check_launch("k_dist_area");
    if (rc != HL_OK) return rc;
    return scan_exclusive(AreaIn{pre}, AreaOut{pre}, (long)T, bl, counts, st, "hl_mesh_distance_areas: scan");
}

int hl_mesh_distance_count(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy,
                           int64_t gz, int64_t *counts, int32_t *status, void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(count_ok(N) && count_ok(T), "hl_mesh_distance_count: bad sizes (N %lld, T %lld; both 1 .. 2^31 - 1)", (long long)N, (long long)T);
    HL_REQUIRE(origin_ok(h_origin) && h > 0.0 && finite_host(h), "hl_mesh_distance_count: the cell must be positive and finite, the origin finite");
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    HL_REQUIRE(cells, "hl_mesh_distance_count: a grid of %lld x %lld x %lld cells (each >= 1, at most 2^27 in all: pass a larger cell)", (long long)gx,
               (long long)gy, (long long)gz);
    HL_REQUIRE(vertices && triangles && counts && status && scratch, "hl_mesh_distance_count: NULL argument");
    const Layout l = layout_of(T, cells);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_distance_count: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_distance_count: scratch must be 16-byte aligned");
    char *base = static_cast<char *>(scratch);
    double *rec = reinterpret_cast<double *>(base + l.rec);
    int *flag = reinterpret_cast<int *>(base + l.flag), *wide = reinterpret_cast<int *>(base + l.wide);
    unsigned *start = reinterpret_cast<unsigned *>(base + l.start);
    unsigned long long *bl = reinterpret_cast<unsigned long long *>(base + l.blocks);
    const hipStream_t st = (hipStream_t)stream;
    const MeshIn m = mesh_of(vertices, N, triangles, T, h_origin);
    const Grid gr = grid_of(h_origin, h, gx, gy, gz);
    HL_HIP(hipMemsetAsync(start, 0, (size_t)(cells + 1) * 4, st));
    HL_HIP(hipMemsetAsync(status, 0, 4, st));
    HL_HIP(hipMemsetAsync(counts, 0, 4 * 8, st));
    hipLaunchKernelGGL(k_dist_records, dim3((unsigned)blocks_of(T)), dim3(kThreads), 0, st, m, gr, rec, flag, start, status);
    int rc = check_launch("k_dist_records");
    if (rc != HL_OK) return rc;
    rc = scan_exclusive(CellIn{start}, CellOut{start}, (long)(cells + 1), bl, counts, st, "hl_mesh_distance_count: cell scan");
    if (rc != HL_OK) return rc;
    return scan_exclusive(FlagIn{flag}, WideOut{wide}, (long)T, bl, counts + 2, st, "hl_mesh_distance_count: triangle scan");
}

int hl_mesh_distance_fill(int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy, int64_t gz, int32_t *refs, int64_t n_refs, void *scratch,
                          size_t scratch_bytes, void *stream) {
    HL_REQUIRE(count_ok(T), "hl_mesh_distance_fill: bad triangle count %lld (1 .. 2^31 - 1)", (long long)T);
    HL_REQUIRE(origin_ok(h_origin) && h > 0.0 && finite_host(h), "hl_mesh_distance_fill: the cell must be positive and finite, the origin finite");
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    HL_REQUIRE(cells, "hl_mesh_distance_fill: a grid of %lld x %lld x %lld cells (each >= 1, at most 2^27 in all: pass a larger cell)", (long long)gx,
               (long long)gy, (long long)gz);
    HL_REQUIRE(n_refs >= 0 && n_refs <= kMaxRefs, "hl_mesh_distance_fill: %lld references, at most 2^31 (pass a larger cell)", (long long)n_refs);
    HL_REQUIRE(scratch && (refs || n_refs == 0), "hl_mesh_distance_fill: NULL argument");
    const Layout l = layout_of(T, cells);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_distance_fill: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_distance_fill: scratch must be 16-byte aligned");
    if (n_refs == 0) return HL_OK;                  // every valid triangle is wide
    char *base = static_cast<char *>(scratch);
    unsigned *cursor = reinterpret_cast<unsigned *>(base + l.cursor);
    const hipStream_t st = (hipStream_t)stream;
    HL_HIP(hipMemsetAsync(cursor, 0, (size_t)cells * 4, st));
    hipLaunchKernelGGL(k_dist_fill, dim3((unsigned)blocks_of(T)), dim3(kThreads), 0, st, (const double *)(base + l.rec), (const int *)(base + l.flag), T,
                       grid_of(h_origin, h, gx, gy, gz), (const unsigned *)(base + l.start), cursor, refs, n_refs);
    return check_launch("k_dist_fill");
}

int hl_mesh_distance_query(const double *points, const double *normals, int64_t Q, int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy,
                           int64_t gz, const int32_t *refs, int64_t n_refs, int64_t n_wide, double max_distance, double *sqdist, double *distance,
                           int32_t *triangle, double *barycentric, double *point, double *normal_dot, int32_t *status, const void *scratch,
                           size_t scratch_bytes, void *stream) {
    HL_REQUIRE(count_ok(Q) && count_ok(T), "hl_mesh_distance_query: bad sizes (Q %lld, T %lld; both 1 .. 2^31 - 1)", (long long)Q, (long long)T);
    HL_REQUIRE(origin_ok(h_origin) && h > 0.0 && finite_host(h), "hl_mesh_distance_query: the cell must be positive and finite, the origin finite");
    const int64_t cells = cells_of(gx, gy, gz, kMaxCells);
    HL_REQUIRE(cells, "hl_mesh_distance_query: a grid of %lld x %lld x %lld cells (each >= 1, at most 2^27 in all: pass a larger cell)", (long long)gx,
               (long long)gy, (long long)gz);
    HL_REQUIRE(n_refs >= 0 && n_refs <= kMaxRefs, "hl_mesh_distance_query: %lld references, at most 2^31 (pass a larger cell)", (long long)n_refs);
    HL_REQUIRE(n_wide >= 0 && n_wide <= kMaxWide, "hl_mesh_distance_query: %lld wide triangles, at most %lld (pass a larger cell)", (long long)n_wide,
               (long long)kMaxWide);
    HL_REQUIRE(max_distance >= 0.0, "hl_mesh_distance_query: max_distance must be >= 0 (+inf for none)");
    HL_REQUIRE(points && sqdist && distance && triangle && barycentric && point && status && scratch && (refs || n_refs == 0),
               "hl_mesh_distance_query: NULL argument");
    HL_REQUIRE((!normals) == (!normal_dot), "hl_mesh_distance_query: normals and normal_dot go together");
    const Layout l = layout_of(T, cells);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_distance_query: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_distance_query: scratch must be 16-byte aligned");
    const char *base = static_cast<const char *>(scratch);
    QueryArgs q;
    q.points = points, q.normals = normals, q.Q = Q, q.T = T, q.gr = grid_of(h_origin, h, gx, gy, gz);
    q.rec = reinterpret_cast<const double *>(base + l.rec), q.start = reinterpret_cast<const unsigned *>(base + l.start);
    q.refs = refs, q.n_refs = n_refs, q.wide = reinterpret_cast<const int *>(base + l.wide), q.n_wide = (int)n_wide;
    q.max_distance = max_distance;
    q.sqdist = sqdist, q.distance = distance, q.bary = barycentric, q.point = point, q.normal_dot = normal_dot, q.triangle = triangle, q.status = status;
    hipLaunchKernelGGL(k_dist_query, dim3((unsigned)blocks_of(Q)), dim3(kThreads), 0, (hipStream_t)stream, q);
    return check_launch("k_dist_query");
}

int hl_mesh_distance_sample(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, const int64_t *prefix,
                            int64_t total, int64_t S, uint64_t seed, double *points, int64_t *triangle, double *barycentric, double *normals, void *stream) {
    HL_REQUIRE(count_ok(N) && count_ok(T) && count_ok(S), "hl_mesh_distance_sample: bad sizes (N %lld, T %lld, S %lld; each 1 .. 2^31 - 1)", (long long)N,
               (long long)T, (long long)S);
    HL_REQUIRE(origin_ok(h_origin), "hl_mesh_distance_sample: the origin must be finite");
    HL_REQUIRE(total >= 1, "hl_mesh_distance_sample: the mesh has no area (total %lld)", (long long)total);
    HL_REQUIRE(vertices && triangles && prefix && points && triangle && barycentric && normals, "hl_mesh_distance_sample: NULL argument");
    SampleArgs a;
    a.m = mesh_of(vertices, N, triangles, T, h_origin);
    a.prefix = reinterpret_cast<const unsigned long long *>(prefix), a.total = (unsigned long long)total, a.S = S, a.seed = seed;
    a.points = points, a.bary = barycentric, a.normals = normals, a.triangle = triangle;
    hipLaunchKernelGGL(k_dist_sample, dim3((unsigned)blocks_of(S)), dim3(kThreads), 0, (hipStream_t)stream, a);
    return check_launch("k_dist_sample");
}

int hl_mesh_distance_reduce(const double *distance, const double *sqdist, const double *normal_dot, int64_t Q, const double *h_thresholds, int n_thresholds,
                            double *out, void *stream) {
    HL_REQUIRE(count_ok(Q), "hl_mesh_distance_reduce: bad query count %lld (1 .. 2^31 - 1)", (long long)Q);
    HL_REQUIRE(n_thresholds >= 0 && n_thresholds <= kMaxThresholds, "hl_mesh_distance_reduce: %d thresholds, at most 8", n_thresholds);
    HL_REQUIRE(distance && sqdist && out && (h_thresholds || n_thresholds == 0), "hl_mesh_distance_reduce: NULL argument");
    ReduceArgs a;
    a.distance = distance, a.sqdist = sqdist, a.normal_dot = normal_dot, a.Q = Q, a.n_thresholds = n_thresholds;
    for (int k = 0; k < kMaxThresholds; ++k) a.thresholds[k] = k < n_thresholds ? h_thresholds[k] : 0.0;
    const int blocks = (int)(blocks_of(Q) < kReduceBlocks ? blocks_of(Q) : kReduceBlocks);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dist_reduce, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, out + kReduceWords);
    const int rc = check_launch("k_dist_reduce");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_dist_reduce_finish, dim3(1), dim3(kThreads), 0, st, (const double *)(out + kReduceWords), blocks, out);
    return check_launch("k_dist_reduce_finish");
}

}  // extern "C"
