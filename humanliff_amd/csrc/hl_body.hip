// Posing the body model on the device, MI355X (gfx950): linear blend skinning of an SMPL-style model for one frame or a sequence, the
// world bounds of every frame and the per-vertex tables hl_deform_points / hl_deform_rays consume (smpl/smpl_numpy.py SMPL.__call__,
// SynBodyView_datasets.py:141-182 prepare_input and NeRF/deform.py deform_tables of this package).  Contract: DESIGN.md "Body model".
// fp32 on the vector ALU, every sum in a fixed order, no float atomics; frames are independent, so a frame has the same bits alone or
// inside a batch.  (-ffp-contract=off: a product and the sum it goes into are two roundings everywhere below.)
//
// k_body_transpose (hl_body_kernels.h) / k_body_regress (hl_body_pack, once per model): posedirs (V,3,P) -> (P,3,V), shapedirs -> (Sp,3,V), weights (V,J)
//   -> (J,V), v_template -> (3,V): a thread per vertex then reads neighbouring addresses in neighbouring lanes.  The joint regressor
//   is applied to the template and to every shape direction once: (J,3) and (J,3,Sp).  One workgroup per output value; thread t adds
//   the float64 products of vertices t, t + 256, ... in order, then the fixed tree of hl_reduce.h; the sum is rounded to fp32 once.
// k_body_joints: one workgroup (one wave) per frame.  Rodrigues with the renderer's convention angle = |v + 1e-8| (a zero vector gives
//   the identity); rest joints = (J t)[j] + sum_s (J s)[j][s] beta[s], s ascending; the kinematic chain joint by joint in index order
//   (parent[i] < i), 16 lanes forming the 4x4 product G[parent] L[i] with k ascending; A = G with G [J; 0] taken off its last column.
// k_body_skin<FC>: a workgroup owns 256 vertices and FC frames.  The chunk's pose features, betas, joint transforms and R / Th sit in
//   LDS; one pass over the packed posedirs (the only large stream: 17 MB for SMPL) feeds FC accumulator triples per thread, feature
//   index ascending.  Then per frame: shape_off (s ascending), T = sum_j w[v][j] A_j (j ascending), v_smpl = T [(v_t + shape_off) +
//   pose_off; 1], world = v_smpl R^T + Th, verts4 = (world - Th) R from the rounded world vertex, Rinv by cofactors, the table row.
//   FC = 8 (kChunk) for a sequence - 24 accumulators, the features of a chunk are 6.6 KB of LDS for SMPL - and FC = 1 for one frame.
// k_body_bounds (hl_body_kernels.h): one workgroup per frame: min / max of the frame's vertices (thread t takes t, t + 256, ..., then the tree), - / +
//   `margin`, y once more by `y_margin`: two fp32 subtractions, as SynBodyView_datasets.py:174-179 does them with 0.05f and 0.05f
//   (hl_body_pose) and TightCap_dataset.py:165-168 of the reference with 0.05f and 0.1f (hl_pose_body_margins).
#include "hl_body_kernels.h"

namespace hl {
namespace {

constexpr int kChunk = 8;                   // frames per workgroup of the skinning pass
constexpr int kMaxJ = 64, kMaxS = 16;

struct Packed {                             // offsets (floats) into the packed model
    int64_t pd, sd, wt, vt, jt, js, total;
};
inline Packed layout(int V, int J, int Sp) {
    Packed p;
    const int64_t P = 9 * (int64_t)(J - 1);
    p.pd = 0;
    p.sd = p.pd + P * 3 * V;
    p.wt = p.sd + (int64_t)Sp * 3 * V;
    p.vt = p.wt + (int64_t)J * V;
    p.jt = p.vt + 3 * (int64_t)V;
    p.js = p.jt + 3 * J;
    p.total = p.js + 3 * (int64_t)J * Sp;
    return p;
}

// workgroup o = (j 3 + c) (1 + Sp) + q: q = 0 the template, q >= 1 shape direction q - 1
__global__ __launch_bounds__(kThreads) void k_body_regress(const float *__restrict__ jreg, const float *__restrict__ vt,
                                                           const float *__restrict__ sd, int sd_cols, int V, int Sp,
                                                           float *__restrict__ jt, float *__restrict__ js) {
    __shared__ double sh[kThreads];
    const int o = (int)blockIdx.x, q = o % (1 + Sp), jc = o / (1 + Sp), j = jc / 3, c = jc - 3 * j;
    const float *row = jreg + (int64_t)j * V;
    double acc = 0.0;
    for (int v = (int)threadIdx.x; v < V; v += kThreads) {
        const float x = q == 0 ? vt[3 * (int64_t)v + c] : sd[(3 * (int64_t)v + c) * sd_cols + (q - 1)];
        acc += (double)row[v] * (double)x;
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if (q == 0)
            jt[jc] = (float)tot;
        else
            js[(int64_t)jc * Sp + (q - 1)] = (float)tot;
    }
}

struct PoseArgs {
    const float *pd, *sd, *wt, *vt, *jt, *js;      // the packed model
    const int *parents;
    int V, J, P, Sp, S, F;
    const float *poses, *shapes, *rt, *big;
    int shapes_stride, rt_stride;
    float *A, *feat;                               // workspace: (F,J,16), (F,P)
    float *vertices, *joints, *bounds, *verts4, *table, *big_out;
};

__global__ __launch_bounds__(64) void k_body_joints(PoseArgs a) {
    __shared__ float rot[kMaxJ][9], jr[kMaxJ * 3], L[kMaxJ][16], G[kMaxJ][16];
    __shared__ int par[kMaxJ];
    const int64_t f = blockIdx.x;
    const int t = (int)threadIdx.x, J = a.J;
    const float *beta = a.shapes + f * a.shapes_stride;
    if (t < J) {
        const float *pv = a.poses + (f * J + t) * 3;
        const float x = pv[0], y = pv[1], z = pv[2];
        const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
        const float angle = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float kx = x / angle, ky = y / angle, kz = z / angle;
        const float K[9] = {0.f, -kz, ky, kz, 0.f, -kx, -ky, kx, 0.f};
        const float s = sinf(angle), c1 = 1.f - cosf(angle);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float kk = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
                const float v = ((r == c ? 1.f : 0.f) + s * K[3 * r + c]) + c1 * kk;
                rot[t][3 * r + c] = v;
                if (t >= 1) a.feat[f * a.P + (t - 1) * 9 + 3 * r + c] = v - (r == c ? 1.f : 0.f);
            }
        const int p = t == 0 ? 0 : a.parents[t];
        par[t] = p < 0 ? 0 : (p > t - 1 ? (t == 0 ? 0 : t - 1) : p);      // (the loader refuses such parents; never index outside)
    }
    for (int i = t; i < 3 * J; i += 64) {
        float v = a.jt[i];
        for (int s = 0; s < a.S; ++s) v += a.js[i * a.Sp + s] * beta[s];
        jr[i] = v;
    }
    __syncthreads();
    if (t < J) {
        const int p = par[t];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) L[t][4 * r + c] = rot[t][3 * r + c];
            L[t][4 * r + 3] = t == 0 ? jr[r] : jr[3 * t + r] - jr[3 * p + r];
        }
        L[t][12] = 0.f, L[t][13] = 0.f, L[t][14] = 0.f, L[t][15] = 1.f;
    }
    __syncthreads();
    if (t < 16) G[0][t] = L[0][t];
    for (int i = 1; i < J; ++i) {
        __syncthreads();
        if (t < 16) {
            const int r = t >> 2, c = t & 3, p = par[i];
            G[i][t] = ((G[p][4 * r] * L[i][c] + G[p][4 * r + 1] * L[i][4 + c]) + G[p][4 * r + 2] * L[i][8 + c]) + G[p][4 * r + 3] * L[i][12 + c];
        }
    }
    __syncthreads();
    if (t < J) {
        const float *g = G[t];
        if (a.joints) {
            const float *rt = a.rt + f * a.rt_stride;
            float *o = a.joints + (f * J + t) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = ((g[3] * rt[3 * i] + g[7] * rt[3 * i + 1]) + g[11] * rt[3 * i + 2]) + rt[9 + i];
        }
        float *o = a.A + (f * J + t) * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[4 * r] = g[4 * r], o[4 * r + 1] = g[4 * r + 1], o[4 * r + 2] = g[4 * r + 2];
            o[4 * r + 3] = g[4 * r + 3] - ((g[4 * r] * jr[3 * t] + g[4 * r + 1] * jr[3 * t + 1]) + g[4 * r + 2] * jr[3 * t + 2]);
        }
    }
}

inline size_t skin_lds_floats(int FC, int J, int S) { return (size_t)FC * ((size_t)J * 12 + 9 * (size_t)(J - 1) + S + 12); }

template <int FC>
__global__ __launch_bounds__(kThreads) void k_body_skin(PoseArgs a) {
    extern __shared__ float lds[];
    const int J = a.J, P = a.P, S = a.S, V = a.V, tid = (int)threadIdx.x;
    float *sA = lds;                        // [FC][J][12]: rows 0..2 of A
    float *sF = sA + FC * J * 12;           // [P][FC]
    float *sB = sF + P * FC;                // [S][FC]
    float *sRT = sB + S * FC;               // [FC][12]
    const int64_t f0 = (int64_t)blockIdx.y * FC;
    const int nf = a.F - f0 < FC ? (int)(a.F - f0) : FC;
    // (a chunk's missing frames are staged as copies of its last one: computed, never stored)
    for (int i = tid; i < FC * J * 12; i += kThreads) {
        const int fl = i / (J * 12), r = i - fl * (J * 12), f = fl < nf ? fl : nf - 1;
        sA[i] = a.A[(f0 + f) * J * 16 + (r / 12) * 16 + r % 12];
    }
    for (int i = tid; i < P * FC; i += kThreads) {
        const int k = i / FC, fl = i - k * FC, f = fl < nf ? fl : nf - 1;
        sF[i] = a.feat[(f0 + f) * P + k];
    }
    for (int i = tid; i < S * FC; i += kThreads) {
        const int s = i / FC, fl = i - s * FC, f = fl < nf ? fl : nf - 1;
        sB[i] = a.shapes[(f0 + f) * a.shapes_stride + s];
    }
    for (int i = tid; i < FC * 12; i += kThreads) {
        const int fl = i / 12, f = fl < nf ? fl : nf - 1;
        sRT[i] = a.rt[(f0 + f) * a.rt_stride + (i - fl * 12)];
    }
    __syncthreads();
    const int v = (int)blockIdx.x * kThreads + tid;
    if (v >= V) return;

    float po[FC][3];
#pragma unroll
    for (int f = 0; f < FC; ++f) po[f][0] = po[f][1] = po[f][2] = 0.f;
    const float *pd = a.pd + v;
#pragma unroll 4
    for (int k = 0; k < P; ++k) {
        const float x = pd[(int64_t)(3 * k) * V], y = pd[(int64_t)(3 * k + 1) * V], z = pd[(int64_t)(3 * k + 2) * V];
#pragma unroll
        for (int f = 0; f < FC; ++f) {
            const float w = sF[k * FC + f];
            po[f][0] += x * w;
            po[f][1] += y * w;
            po[f][2] += z * w;
        }
    }
    const float vt0 = a.vt[v], vt1 = a.vt[(int64_t)V + v], vt2 = a.vt[2 * (int64_t)V + v];
#pragma unroll
    for (int f = 0; f < FC; ++f) {
        if (f >= nf) break;
        const int64_t row = (f0 + f) * V + v;
        float so[3] = {0.f, 0.f, 0.f};
        for (int s = 0; s < S; ++s) {
            const float b = sB[s * FC + f];
            so[0] += a.sd[(int64_t)(3 * s) * V + v] * b;
            so[1] += a.sd[(int64_t)(3 * s + 1) * V + v] * b;
            so[2] += a.sd[(int64_t)(3 * s + 2) * V + v] * b;
        }
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
        const float *Af = sA + f * J * 12;
        for (int j = 0; j < J; ++j) {
            const float w = a.wt[(int64_t)j * V + v];
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] += w * Af[j * 12 + e];
        }
        const float x = (vt0 + so[0]) + po[f][0], y = (vt1 + so[1]) + po[f][1], z = (vt2 + so[2]) + po[f][2];
        float vs[3], wv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) vs[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
        const float *R = sRT + f * 12, *Th = R + 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) wv[i] = ((vs[0] * R[3 * i] + vs[1] * R[3 * i + 1]) + vs[2] * R[3 * i + 2]) + Th[i];
        if (a.vertices) {
            float *o = a.vertices + row * 3;
            o[0] = wv[0], o[1] = wv[1], o[2] = wv[2];
        }
        if (a.verts4) {
            const float d0 = wv[0] - Th[0], d1 = wv[1] - Th[1], d2 = wv[2] - Th[2];
            float4 q;
            q.x = (d0 * R[0] + d1 * R[3]) + d2 * R[6];
            q.y = (d0 * R[1] + d1 * R[4]) + d2 * R[7];
            q.z = (d0 * R[2] + d1 * R[5]) + d2 * R[8];
            q.w = 0.f;
            reinterpret_cast<float4 *>(a.verts4)[row] = q;
        }
        if (a.big_out) {
            float4 *o = reinterpret_cast<float4 *>(a.big_out) + row * 4;
            o[0] = make_float4(T[0], T[1], T[2], T[4]);
            o[1] = make_float4(T[5], T[6], T[8], T[9]);
            o[2] = make_float4(T[10], T[3], T[7], T[11]);
            o[3] = make_float4(po[f][0], po[f][1], po[f][2], 0.f);
        }
        if (a.table) {
            // inverse of the blended 3x3 by cofactors
            const float m00 = T[0], m01 = T[1], m02 = T[2], m10 = T[4], m11 = T[5], m12 = T[6], m20 = T[8], m21 = T[9], m22 = T[10];
            const float c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
            const float det = (m00 * c00 + m01 * c01) + m02 * c02;
            const float i00 = c00 / det, i01 = (m02 * m21 - m01 * m22) / det, i02 = (m01 * m12 - m02 * m11) / det;
            const float i10 = c01 / det, i11 = (m00 * m22 - m02 * m20) / det, i12 = (m02 * m10 - m00 * m12) / det;
            const float i20 = c02 / det, i21 = (m01 * m20 - m00 * m21) / det, i22 = (m00 * m11 - m01 * m10) / det;
            const float4 *b = reinterpret_cast<const float4 *>(a.big) + (int64_t)v * 4;
            const float4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];      // Rbig[9] tbig[3] pose_off_big[3]
            float4 *o = reinterpret_cast<float4 *>(a.table) + row * 9;
            o[0] = make_float4(T[3], T[7], T[11], i00);
            o[1] = make_float4(i01, i02, i10, i11);
            o[2] = make_float4(i12, i20, i21, i22);
            o[3] = make_float4(po[f][0], po[f][1], po[f][2], so[0]);
            o[4] = make_float4(so[1], so[2], b3.x, b3.y);
            o[5] = make_float4(b3.z, b0.x, b0.y, b0.z);
            o[6] = make_float4(b0.w, b1.x, b1.y, b1.z);
            o[7] = make_float4(b1.w, b2.x, b2.y, b2.z);
            o[8] = make_float4(b2.w, 0.f, 0.f, 0.f);
        }
    }
}

inline bool sizes_ok(int V, int J, int Sp) { return V > 0 && J >= 1 && J <= kMaxJ && Sp >= 1 && Sp <= kMaxS; }

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

size_t hl_body_packed_bytes(int V, int J, int Sp) { return sizes_ok(V, J, Sp) ? (size_t)layout(V, J, Sp).total * sizeof(float) : 0; }

int hl_body_pack(const float *v_template, const float *shapedirs, int sd_cols, const float *posedirs, const float *J_regressor,
                 const float *weights, int V, int J, int Sp, float *packed, void *stream) {
    HL_REQUIRE(v_template && shapedirs && posedirs && J_regressor && weights && packed, "hl_body_pack: NULL argument");
    HL_REQUIRE(sizes_ok(V, J, Sp) && J >= 2, "hl_body_pack: bad sizes (V %d, J %d, Sp %d; V > 0, 2 <= J <= %d, 1 <= Sp <= %d)", V, J, Sp, kMaxJ, kMaxS);
    HL_REQUIRE(sd_cols >= Sp, "hl_body_pack: shapedirs has %d columns, fewer than Sp = %d", sd_cols, Sp);
    const Packed p = layout(V, J, Sp);
    const int P = 9 * (J - 1);
    const hipStream_t st = (hipStream_t)stream;
    struct { const float *in; int C, cols, K; int64_t off; } jobs[4] = {
        {posedirs, 3, P, P, p.pd}, {shapedirs, 3, sd_cols, Sp, p.sd}, {weights, 1, J, J, p.wt}, {v_template, 1, 3, 3, p.vt}};
    for (const auto &j : jobs) {
        const int64_t n = (int64_t)j.K * j.C * V;
        HL_REQUIRE((n + kThreads - 1) / kThreads <= 0x7fffffff, "hl_body_pack: model too large");
        hipLaunchKernelGGL(k_body_transpose, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, j.in, V, j.C, j.cols, j.K,
                           packed + j.off);
        const int rc = check_launch("k_body_transpose");
        if (rc != HL_OK) return rc;
    }
    hipLaunchKernelGGL(k_body_regress, dim3(3 * J * (1 + Sp)), dim3(kThreads), 0, st, J_regressor, v_template, shapedirs, sd_cols, V, Sp,
                       packed + p.jt, packed + p.js);
    return check_launch("k_body_regress");
}

int hl_body_chunk_frames(void) { return kChunk; }

size_t hl_body_pose_workspace_bytes(int J, int F) {
    if (J < 2 || J > kMaxJ || F < 1) return 0;
    return (size_t)F * ((size_t)J * 16 + 9 * (size_t)(J - 1)) * sizeof(float);
}

int hl_body_pose(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                 int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                 float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, void *stream) {
    return hl_pose_body_margins(packed, parents, V, J, Sp, S, F, poses, shapes, shapes_stride, rt, rt_stride, big, vertices, joints, bounds, verts4,
                                table, big_out, workspace, workspace_bytes, 0.05f, 0.05f, stream);
}

int hl_pose_body_margins(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                         int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                         float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin, float y_margin,
                         void *stream) {
    HL_REQUIRE(margin >= 0.f && y_margin >= 0.f, "hl_body_pose: the bounds' margins must not be negative (got %g, %g)", (double)margin, (double)y_margin);
    HL_REQUIRE(packed && parents && poses && shapes && rt, "hl_body_pose: NULL argument");
    HL_REQUIRE(sizes_ok(V, J, Sp) && J >= 2 && S >= 1 && S <= Sp && F >= 1,
               "hl_body_pose: bad sizes (V %d, J %d, Sp %d, S %d, F %d; V > 0, 2 <= J <= %d, 1 <= S <= Sp <= %d, F >= 1)", V, J, Sp, S, F, kMaxJ, kMaxS);
    HL_REQUIRE(shapes_stride == 0 || shapes_stride == S, "hl_body_pose: shapes_stride must be 0 or S (got %d)", shapes_stride);
    HL_REQUIRE(rt_stride == 0 || rt_stride == 12, "hl_body_pose: rt_stride must be 0 or 12 (got %d)", rt_stride);
    HL_REQUIRE(!table || big, "hl_body_pose: the table needs the big-pose rows (big)");
    HL_REQUIRE(!bounds || vertices, "hl_body_pose: the bounds are taken over `vertices`, which is NULL");
    HL_REQUIRE(aligned16({verts4, table, big_out, big}), "hl_body_pose: verts4, table, big and big_out must be 16-byte aligned");
    const size_t need = hl_body_pose_workspace_bytes(J, F);
    HL_REQUIRE(workspace && workspace_bytes >= need, "hl_body_pose: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    const int chunks = F == 1 ? 1 : (F + kChunk - 1) / kChunk;
    HL_REQUIRE(chunks <= 65535, "hl_body_pose: at most %d frames per call (got %d)", 65535 * kChunk, F);
    const Packed p = layout(V, J, Sp);
    PoseArgs a;
    a.pd = packed + p.pd, a.sd = packed + p.sd, a.wt = packed + p.wt, a.vt = packed + p.vt, a.jt = packed + p.jt, a.js = packed + p.js;
    a.parents = parents;
    a.V = V, a.J = J, a.P = 9 * (J - 1), a.Sp = Sp, a.S = S, a.F = F;
    a.poses = poses, a.shapes = shapes, a.rt = rt, a.big = big;
    a.shapes_stride = shapes_stride, a.rt_stride = rt_stride;
    a.A = static_cast<float *>(workspace);
    a.feat = a.A + (size_t)F * J * 16;
    a.vertices = vertices, a.joints = joints, a.bounds = bounds, a.verts4 = verts4, a.table = table, a.big_out = big_out;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_body_joints, dim3(F), dim3(64), 0, st, a);
    int rc = check_launch("k_body_joints");
    if (rc != HL_OK) return rc;
    if (vertices || verts4 || table || big_out) {
        const dim3 grid((V + kThreads - 1) / kThreads, chunks);
        if (F == 1)
            hipLaunchKernelGGL(k_body_skin<1>, grid, dim3(kThreads), skin_lds_floats(1, J, S) * sizeof(float), st, a);
        else
            hipLaunchKernelGGL(k_body_skin<kChunk>, grid, dim3(kThreads), skin_lds_floats(kChunk, J, S) * sizeof(float), st, a);
        rc = check_launch("k_body_skin");
        if (rc != HL_OK) return rc;
    }
    if (bounds) {
        hipLaunchKernelGGL(k_body_bounds, dim3(F), dim3(kThreads), 0, st, vertices, V, margin, y_margin, bounds);
        rc = check_launch("k_body_bounds");
    }
    return rc;
}

}  // extern "C"
