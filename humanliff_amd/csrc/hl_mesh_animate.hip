// Animating an extracted mesh, MI355X (gfx950): bind every mesh vertex to the K nearest vertices of a posed body once, then repose the
// mesh for any number of frames from the forward rows the skinning pass writes (hl_body.hip, big_out: R[9] t[3] pose_off[3] pad[1] per
// body vertex, of shape set 1 - the set the posed vertices come from; SMPL and SMPL-X run the same code).  Contract: DESIGN.md
// "Animating the mesh".  fp32 on the vector ALU, every sum in a fixed order, no atomics; frames are independent, so a frame has the
// same bits alone or inside a batch.  (-ffp-contract=off: a product and the sum it goes into are two roundings, so the place of every
// parenthesis below is part of the contract.)
//
// k_mesh_bind<KT>: a thread per mesh vertex.  q = (x - Th) R_w in deform_query's order; the body's SMPL-space vertices (verts4) go
//   through LDS in tiles of 2048 as in k_deform_points (one broadcast read serves the wave); d = (dx dx + dy dy) + dz dz; the running
//   KT best (d, index) stay sorted in registers: a candidate enters only with d < the worst kept, at the last slot, and moves up while
//   it is strictly nearer than the slot above - vertices are visited in index order, so among equal distances the lower index stays in
//   front: the order is (d, index) ascending.  KT in {1, 2, 4, 8} >= K; exactly K are used and stored.
//   w_k = 1 / (d_k + 1e-8f) over their sum (k ascending); M = sum_k w_k R_k, c = sum_k w_k (R_k po_k + t_k) (k ascending);
//   u = M^-1 ((q - transl) - c), the inverse by cofactors, every cofactor divided by the determinant, as the deformation table's Rinv
//   is made (transl: what SMPL-X added to the bind frame after skinning - verts4 holds it, the rows do not; NULL for SMPL);
//   the rest normal m = normalize(M^T (n R_w)), (0,0,0) for a zero or non-finite vector.
// k_mesh_repose<FC>: a thread per mesh vertex holds its ids, weights, u and m in registers and walks the FC frames of its chunk
//   (grid.y): per frame M and c as above from rows[f] - four 16-byte loads per neighbour; marching-cubes vertices come in lattice order,
//   so neighbouring threads gather neighbouring rows - y = M u + c (+ transl[f]), world = R_w y + Th as k_body_skin forms it; the normal
//   is normalize(cof(M) m) rotated by R_w: the cofactor matrix, so nothing is divided, and zero stays zero.  With bounds the workgroup
//   reduces its 256 world vertices to one min / max box per frame (the tree of hl_reduce.h) and writes it to the scratch.
// k_mesh_bounds: one workgroup per frame folds the boxes of that frame's workgroups (thread t takes t, t + 256, ..., then the tree) and
//   applies the margins with the body's two subtractions.  Min and max are exact in any order.
#include "hl_mesh.h"
#include "hl_reduce.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = kMeshThreads;
static_assert(kThreads == kReduceThreads, "block_reduce reduces a workgroup of kReduceThreads");
constexpr int kTile = 2048;                 // body vertices per LDS tile (32 KB)
constexpr int kMaxK = 8;
constexpr int kFrames = 8;                  // frames per workgroup of the repose pass
constexpr int kMaxGridY = 65535;

struct Row {                                // a forward row: y = R (x + po) + t
    float R[9], t[3], po[3];
};

__device__ __forceinline__ Row load_row(const float *__restrict__ rows, int64_t j) {
    const float4 *p = reinterpret_cast<const float4 *>(rows) + j * 4;
    const float4 a = p[0], b = p[1], c = p[2], d = p[3];
    Row r;
    r.R[0] = a.x, r.R[1] = a.y, r.R[2] = a.z, r.R[3] = a.w, r.R[4] = b.x, r.R[5] = b.y, r.R[6] = b.z, r.R[7] = b.w, r.R[8] = c.x;
    r.t[0] = c.y, r.t[1] = c.z, r.t[2] = c.w;
    r.po[0] = d.x, r.po[1] = d.y, r.po[2] = d.z;
    return r;
}

// M += w R, c += w (R po + t)
__device__ __forceinline__ void blend(const Row &r, float w, float (&M)[9], float (&c)[3]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] += w * r.R[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float o = ((r.R[3 * i] * r.po[0] + r.R[3 * i + 1] * r.po[1]) + r.R[3 * i + 2] * r.po[2]) + r.t[i];
        c[i] += w * o;
    }
}

// x / |x|, (0,0,0) for a zero or non-finite vector
__device__ __forceinline__ void normalize3(float (&v)[3]) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const bool ok = len > 0.f && len < INFINITY;          // (false for NaN)
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = ok ? v[i] / len : 0.f;
}

struct BindArgs {
    const float *pts, *nrm;                 // (N,3) world; nrm may be NULL
    int64_t N;
    const float4 *verts4;                   // (V) SMPL-space body vertices of the bind frame
    const float *rows, *rt;                 // (V,16); R | Th of the bind frame
    const float *transl;                    // (3) or NULL: what the bind frame's body had added after skinning
    int V, K;
    int *ids;                               // (N,K)
    float *weights, *rest, *rest_normals;   // (N,K), (N,3), (N,3) or NULL
};

template <int KT>
__global__ __launch_bounds__(kThreads) void k_mesh_bind(const BindArgs a) {
    __shared__ float4 sv[kTile];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.N;
    const int64_t ic = live ? i : a.N - 1;      // (all threads stage the tiles)
    const float *R = a.rt, *Th = a.rt + 9;
    const float wx = a.pts[ic * 3 + 0] - Th[0], wy = a.pts[ic * 3 + 1] - Th[1], wz = a.pts[ic * 3 + 2] - Th[2];
    const float qx = (wx * R[0] + wy * R[3]) + wz * R[6];
    const float qy = (wx * R[1] + wy * R[4]) + wz * R[7];
    const float qz = (wx * R[2] + wy * R[5]) + wz * R[8];
    float bd[KT];
    int bi[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) bd[k] = INFINITY, bi[k] = 0;      // (a slot never filled - NaN input - names vertex 0: in bounds)
    for (int v0 = 0; v0 < a.V; v0 += kTile) {
        const int n = min(kTile, a.V - v0);
        __syncthreads();
        for (int k = (int)threadIdx.x; k < n; k += kThreads) sv[k] = a.verts4[v0 + k];
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 v = sv[k];
            const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < bd[KT - 1]) {
                bd[KT - 1] = d, bi[KT - 1] = v0 + k;
#pragma unroll
                for (int s = KT - 1; s > 0; --s) {
                    const bool up = bd[s] < bd[s - 1];
                    const float td = bd[s - 1];
                    const int ti = bi[s - 1];
                    bd[s - 1] = up ? bd[s] : td, bi[s - 1] = up ? bi[s] : ti;
                    bd[s] = up ? td : bd[s], bi[s] = up ? ti : bi[s];
                }
            }
        }
    }
    if (!live) return;
    const int K = a.K;
    float w[KT], sum = 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        w[k] = k < K ? 1.f / (bd[k] + 1e-8f) : 0.f;
        if (k < K) sum += w[k];
    }
    float M[9], c[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < K) {
            w[k] = w[k] / sum;
            blend(load_row(a.rows, bi[k]), w[k], M, c);
            a.ids[i * K + k] = bi[k];
            a.weights[i * K + k] = w[k];
        }
    }
    // inverse of the blended 3x3 by cofactors
    const float m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const float c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
    const float det = (m00 * c00 + m01 * c01) + m02 * c02;
    const float i00 = c00 / det, i01 = (m02 * m21 - m01 * m22) / det, i02 = (m01 * m12 - m02 * m11) / det;
    const float i10 = c01 / det, i11 = (m00 * m22 - m02 * m20) / det, i12 = (m02 * m10 - m00 * m12) / det;
    const float i20 = c02 / det, i21 = (m01 * m20 - m00 * m21) / det, i22 = (m00 * m11 - m01 * m10) / det;
    // (repose forms (M u + c) + transl: the translation comes off first)
    const float px = a.transl ? qx - a.transl[0] : qx, py = a.transl ? qy - a.transl[1] : qy, pz = a.transl ? qz - a.transl[2] : qz;
    const float ex = px - c[0], ey = py - c[1], ez = pz - c[2];
    a.rest[i * 3 + 0] = (i00 * ex + i01 * ey) + i02 * ez;
    a.rest[i * 3 + 1] = (i10 * ex + i11 * ey) + i12 * ez;
    a.rest[i * 3 + 2] = (i20 * ex + i21 * ey) + i22 * ez;
    if (a.rest_normals) {
        float m[3] = {0.f, 0.f, 0.f};
        if (a.nrm) {
            const float nx = a.nrm[i * 3 + 0], ny = a.nrm[i * 3 + 1], nz = a.nrm[i * 3 + 2];
            const float sx = (nx * R[0] + ny * R[3]) + nz * R[6];
            const float sy = (nx * R[1] + ny * R[4]) + nz * R[7];
            const float sz = (nx * R[2] + ny * R[5]) + nz * R[8];
            m[0] = (m00 * sx + m10 * sy) + m20 * sz;
            m[1] = (m01 * sx + m11 * sy) + m21 * sz;
            m[2] = (m02 * sx + m12 * sy) + m22 * sz;
            normalize3(m);
        }
        a.rest_normals[i * 3 + 0] = m[0], a.rest_normals[i * 3 + 1] = m[1], a.rest_normals[i * 3 + 2] = m[2];
    }
}

struct Box {
    float lo[3], hi[3];
};
struct BoxUnion {
    __device__ __forceinline__ Box operator()(const Box &x, const Box &y) const {
        Box r;
#pragma unroll
        for (int c = 0; c < 3; ++c) r.lo[c] = fminf(x.lo[c], y.lo[c]), r.hi[c] = fmaxf(x.hi[c], y.hi[c]);
        return r;
    }
};

struct ReposeArgs {
    const int *ids;                         // (N,K)
    const float *weights, *rest, *rest_normals;
    int64_t N;
    int V, K, F;
    int f_begin;                            // first frame of this launch (frames beyond 65 535 chunks take further launches)
    const float *rows;                      // (F,V,16)
    const float *rt;                        // R | Th per frame
    int rt_stride;
    const float *transl;                    // (F,3) or NULL
    float *vertices, *normals;              // (F,N,3); normals may be NULL
    float *partials;                        // (F, blocks, 6) or NULL
};

template <int KT>
__global__ __launch_bounds__(kThreads) void k_mesh_repose(const ReposeArgs a) {
    __shared__ Box sh[kThreads];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.N;
    const int64_t ic = live ? i : a.N - 1;      // (all threads take part in the reductions)
    const int K = a.K;
    int id[KT];
    float w[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int j = k < K ? a.ids[ic * K + k] : 0;
        id[k] = j < 0 ? 0 : (j < a.V ? j : a.V - 1);       // (ids come from hl_mesh_bind; never index outside whatever they hold)
        w[k] = k < K ? a.weights[ic * K + k] : 0.f;
    }
    const float u0 = a.rest[ic * 3 + 0], u1 = a.rest[ic * 3 + 1], u2 = a.rest[ic * 3 + 2];
    const bool wn = a.normals != nullptr;
    const float n0 = wn && a.rest_normals ? a.rest_normals[ic * 3 + 0] : 0.f, n1 = wn && a.rest_normals ? a.rest_normals[ic * 3 + 1] : 0.f,
                n2 = wn && a.rest_normals ? a.rest_normals[ic * 3 + 2] : 0.f;
    const int64_t f0 = (int64_t)a.f_begin + (int64_t)blockIdx.y * kFrames;
    const int nf = a.F - f0 < kFrames ? (int)(a.F - f0) : kFrames;
    for (int fl = 0; fl < nf; ++fl) {
        const int64_t f = f0 + fl;
        const float *rows = a.rows + f * a.V * 16;
        float M[9], c[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) blend(load_row(rows, id[k]), w[k], M, c);
        float y[3], wv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) y[r] = ((M[3 * r] * u0 + M[3 * r + 1] * u1) + M[3 * r + 2] * u2) + c[r];
        if (a.transl) {
#pragma unroll
            for (int r = 0; r < 3; ++r) y[r] = y[r] + a.transl[f * 3 + r];
        }
        const float *R = a.rt + f * a.rt_stride, *Th = R + 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) wv[r] = ((y[0] * R[3 * r] + y[1] * R[3 * r + 1]) + y[2] * R[3 * r + 2]) + Th[r];
        const int64_t o = (f * a.N + i) * 3;
        if (live) a.vertices[o] = wv[0], a.vertices[o + 1] = wv[1], a.vertices[o + 2] = wv[2];
        if (wn) {
            // the cofactor matrix of M
            const float C[9] = {M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6],
                                M[2] * M[7] - M[1] * M[8], M[0] * M[8] - M[2] * M[6], M[1] * M[6] - M[0] * M[7],
                                M[1] * M[5] - M[2] * M[4], M[2] * M[3] - M[0] * M[5], M[0] * M[4] - M[1] * M[3]};
            float g[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) g[r] = (C[3 * r] * n0 + C[3 * r + 1] * n1) + C[3 * r + 2] * n2;
            normalize3(g);
            if (live) {
#pragma unroll
                for (int r = 0; r < 3; ++r) a.normals[o + r] = (g[0] * R[3 * r] + g[1] * R[3 * r + 1]) + g[2] * R[3 * r + 2];
            }
        }
        if (a.partials) {
            Box b;
#pragma unroll
            for (int r = 0; r < 3; ++r) b.lo[r] = live ? wv[r] : INFINITY, b.hi[r] = live ? wv[r] : -INFINITY;
            b = block_reduce(b, sh, BoxUnion());
            if (threadIdx.x == 0) {
                float *p = a.partials + (f * gridDim.x + blockIdx.x) * 6;
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = b.lo[r], p[3 + r] = b.hi[r];
            }
        }
    }
}

// one workgroup per frame: the boxes of the frame's `blocks` workgroups -> bounds (2,3) with the margins
__global__ __launch_bounds__(kThreads) void k_mesh_bounds(const float *__restrict__ partials, int64_t blocks, float margin, float y_margin,
                                                          float *__restrict__ bounds) {
    __shared__ Box sh[kThreads];
    const float *p = partials + (int64_t)blockIdx.x * blocks * 6;
    Box b;
#pragma unroll
    for (int c = 0; c < 3; ++c) b.lo[c] = INFINITY, b.hi[c] = -INFINITY;
    for (int64_t k = threadIdx.x; k < blocks; k += kThreads)
#pragma unroll
        for (int c = 0; c < 3; ++c) b.lo[c] = fminf(b.lo[c], p[k * 6 + c]), b.hi[c] = fmaxf(b.hi[c], p[k * 6 + 3 + c]);
    b = block_reduce(b, sh, BoxUnion());
    if (threadIdx.x == 0) {
        float *o = bounds + (int64_t)blockIdx.x * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float lo = b.lo[c] - margin, hi = b.hi[c] + margin;
            if (c == 1) lo = lo - y_margin, hi = hi + y_margin;
            o[c] = lo, o[3 + c] = hi;
        }
    }
}

// the sizes both entry points refuse; N == 0 is not among them
#define HL_MESH_SIZES(name, N, V, K)                                                                                               \
    do {                                                                                                                           \
        HL_REQUIRE((K) >= 1 && (K) <= kMaxK, "%s: K must be 1 .. %d (got %d)", name, kMaxK, (K));                                   \
        HL_REQUIRE((V) >= 1 && (K) <= (V), "%s: bad sizes (V %d, K %d; V >= 1, K <= V)", name, (V), (K));                           \
        HL_REQUIRE((N) >= 0 && blocks_of(N) <= 0x7fffffff, "%s: bad number of mesh vertices (%lld)", name, (long long)(N));        \
    } while (0)

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_mesh_bind(const float *points, const float *normals, int64_t N, const float *verts4, const float *rows, int V, const float *rt,
                 const float *transl, int K, int32_t *ids, float *weights, float *rest, float *rest_normals, void *stream) {
    HL_MESH_SIZES("hl_mesh_bind", N, V, K);
    if (N == 0) return HL_OK;
    HL_REQUIRE(points && verts4 && rows && rt && ids && weights && rest, "hl_mesh_bind: NULL argument");
    HL_REQUIRE(aligned16({verts4, rows}), "hl_mesh_bind: verts4 and rows must be 16-byte aligned");
    BindArgs a;
    a.pts = points, a.nrm = normals, a.N = N, a.verts4 = reinterpret_cast<const float4 *>(verts4), a.rows = rows, a.rt = rt, a.transl = transl, a.V = V, a.K = K;
    a.ids = ids, a.weights = weights, a.rest = rest, a.rest_normals = rest_normals;
    const dim3 grid((unsigned)blocks_of(N)), block(kThreads);
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1)
        hipLaunchKernelGGL(k_mesh_bind<1>, grid, block, 0, st, a);
    else if (K == 2)
        hipLaunchKernelGGL(k_mesh_bind<2>, grid, block, 0, st, a);
    else if (K <= 4)
        hipLaunchKernelGGL(k_mesh_bind<4>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_mesh_bind<8>, grid, block, 0, st, a);
    return check_launch("k_mesh_bind");
}

size_t hl_mesh_repose_scratch_bytes(int64_t N, int F) { return N < 1 || F < 1 ? 0 : (size_t)F * (size_t)blocks_of(N) * 6 * sizeof(float); }

int hl_mesh_repose(const int32_t *ids, const float *weights, const float *rest, const float *rest_normals, int64_t N, int K, const float *rows,
                   int V, int F, const float *rt, int rt_stride, const float *transl, float *vertices, float *normals, float *bounds,
                   float margin, float y_margin, void *scratch, size_t scratch_bytes, void *stream) {
    HL_MESH_SIZES("hl_mesh_repose", N, V, K);
    HL_REQUIRE(F >= 1, "hl_mesh_repose: F must be at least 1 (got %d)", F);
    HL_REQUIRE(rt_stride == 0 || rt_stride == 12, "hl_mesh_repose: rt_stride must be 0 or 12 (got %d)", rt_stride);
    HL_REQUIRE(margin >= 0.f && y_margin >= 0.f, "hl_mesh_repose: the bounds' margins must not be negative (got %g, %g)", (double)margin,
               (double)y_margin);
    if (N == 0) return HL_OK;
    HL_REQUIRE(ids && weights && rest && rows && rt && vertices, "hl_mesh_repose: NULL argument");
    HL_REQUIRE(!normals || rest_normals, "hl_mesh_repose: normals need the binding's rest normals");
    HL_REQUIRE(aligned16({rows}), "hl_mesh_repose: rows must be 16-byte aligned");
    const size_t need = bounds ? hl_mesh_repose_scratch_bytes(N, F) : 0;
    HL_REQUIRE(!bounds || (scratch && scratch_bytes >= need), "hl_mesh_repose: scratch too small (%zu bytes, need %zu)", scratch_bytes, need);
    ReposeArgs a;
    a.ids = ids, a.weights = weights, a.rest = rest, a.rest_normals = rest_normals, a.N = N, a.V = V, a.K = K, a.F = F;
    a.rows = rows, a.rt = rt, a.rt_stride = rt_stride, a.transl = transl, a.vertices = vertices, a.normals = normals;
    a.partials = bounds ? static_cast<float *>(scratch) : nullptr;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t chunks = ((int64_t)F + kFrames - 1) / kFrames;
    for (int64_t c0 = 0; c0 < chunks; c0 += kMaxGridY) {
        const int64_t nc = chunks - c0 < kMaxGridY ? chunks - c0 : kMaxGridY;
        a.f_begin = (int)(c0 * kFrames);
        const dim3 grid((unsigned)blocks_of(N), (unsigned)nc), block(kThreads);
        if (K == 1)
            hipLaunchKernelGGL(k_mesh_repose<1>, grid, block, 0, st, a);
        else if (K == 2)
            hipLaunchKernelGGL(k_mesh_repose<2>, grid, block, 0, st, a);
        else if (K <= 4)
            hipLaunchKernelGGL(k_mesh_repose<4>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_mesh_repose<8>, grid, block, 0, st, a);
        const int rc = check_launch("k_mesh_repose");
        if (rc != HL_OK) return rc;
    }
    if (!bounds) return HL_OK;
    hipLaunchKernelGGL(k_mesh_bounds, dim3((unsigned)F), dim3(kThreads), 0, st, a.partials, blocks_of(N), margin, y_margin, bounds);
    return check_launch("k_mesh_bounds");
}

}  // extern "C"
