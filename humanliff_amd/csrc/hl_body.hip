// Posing a body model on the device, MI355X (gfx950): linear blend skinning of an SMPL-style model for one frame or a sequence, the
// world bounds of every frame and the per-vertex tables hl_deform_points / hl_deform_rays consume.  Two models, one set of kernels:
//   SMPL   (hl_body_*, hl_pose_body_margins): smpl/smpl_numpy.py SMPL.__call__, SynBodyView_datasets.py:141-182 prepare_input and
//          NeRF/deform.py deform_tables of this package.  Contract: DESIGN.md 4h.  The X = false instantiations below.
//   SMPL-X (hl_smplx_*): SMPLX.forward + lbs of the smplx package as the reference's SynBody flows run it (recon_NeRF/smplx/
//          body_models.py:1188-1242, smplx/lbs.py; SynBody_dataset.py:158-194).  Contract: DESIGN.md 4k.  X = true.
// fp32 on the vector ALU, every sum in a fixed order, no float atomics; frames are independent, so a frame has the same bits alone or
// inside a batch.  (-ffp-contract=off: a product and the sum it goes into are two roundings everywhere below, so the place of every
// parenthesis is part of the contract.)
//
// What SMPL-X adds (all of it behind X, a compile-time flag: a runtime one would carry set 2's accumulators, its LDS region and its
// staging loop into the SMPL kernels):
//   - `poses` is the full pose (global | body 21 | jaw | leye | reye | left hand 15 | right hand 15, pose_mean added by the caller),
//     `shapes` is betas || expression per frame, and `transl` is added to the skinned vertices and joints before R / Th.
//   - TWO sets of shape directions.  Set 1 - columns [0, nb) || [e0, e0 + ne) of the file - shapes the body: vertices, joints, bounds.
//     Set 2 - the first nb + ne RAW columns - is what the renderer's canonical-space tables are built from (renderer.py:87, 364 cut
//     shapedirs to shapes.shape[-1] columns and know nothing of expression columns or of transl).  With a 400-column file the sets differ
//     (e0 = 300), with a 20-column file they coincide (`two_sets` = 0).  The table follows the renderer, quirk included.
//   - The joint rotations do not depend on the set, so the blended 3x3 is shared; set 2 only has rest joints of its own, i.e. another
//     translation column of every joint transform: the second chain carries 3 values per joint, not 16.
//
// k_body_transpose / k_body_regress (pack, once per model): posedirs (V,3,P) -> (P,3,V), shapedirs -> (S,3,V), weights (V,J) -> (J,V),
//   v_template -> (3,V): a thread per vertex then reads neighbouring addresses in neighbouring lanes.  The joint regressor is applied
//   to the template and to every kept shape direction once, from the arrays just transposed: (J,3) and (J,3,S), set 2 after set 1.
//   One workgroup per output value; thread t adds the float64 products of vertices t, t + 256, ... in order, then the fixed tree of
//   hl_reduce.h; the sum is rounded to fp32 once.
// k_body_joints<X>: one workgroup (one wave) per frame.  Rodrigues with the renderer's convention angle = |v + 1e-8| (a zero vector gives
//   the identity); rest joints = (J t)[j] + sum_s (J s)[j][s] beta[s], s ascending; the kinematic chain joint by joint in index order
//   (parent[i] < i), 16 lanes forming the 4x4 product G[parent] L[i] with k ascending; A = G with G [J; 0] taken off its last column.
//   X: lanes 16-18 form the translation column of set 2 (only when a table is asked for and the sets differ).
// k_body_skin<FC, X>: a workgroup owns 256 vertices and FC frames.  The chunk's pose features, coefficients, joint transforms and R / Th
//   sit in LDS; one pass over the packed posedirs (the only large stream: 17 MB for SMPL, 61 MB for SMPL-X) feeds FC accumulator triples
//   per thread, feature index ascending.  Then per frame: shape_off (s ascending), T = sum_j w[v][j] A_j (j ascending), v_smpl =
//   T [(v_t + shape_off) + pose_off; 1] (X: + transl), world = v_smpl R^T + Th, verts4 = (world - Th) R from the rounded world vertex,
//   Rinv by cofactors, the table row.  FC = 8 (kChunk) for a sequence - 24 accumulators - and FC = 1 for one frame.
//   LDS per staged frame, floats: 12 J (rows 0..2 of A) + 9 (J - 1) (pose features) + S (coefficients) + 12 (R | Th), 16.5 KB per
//   chunk for SMPL; X: + 3 J (the set-2 translations) and 16 for R | Th | transl | pad: FC = 8, J = 55, S = 20: 43 104 bytes; at the
//   limits J = 64, S = 32: 50 400 bytes - every accepted size fits the 64 KB default (the static_assert below), so no limit is raised.
// k_body_bounds: one workgroup per frame: min / max of the frame's vertices (thread t takes t, t + 256, ..., then the tree), - / +
//   `margin`, y once more by `y_margin`: two fp32 subtractions, as SynBodyView_datasets.py:174-179 does them with 0.05f and 0.05f
//   (hl_body_pose) and TightCap_dataset.py:165-168 of the reference with 0.05f and 0.1f (hl_pose_body_margins).
#include "hl_reduce.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kReduceThreads, "block_reduce reduces a workgroup of kReduceThreads");
constexpr int kChunk = 8;                   // frames per workgroup of the skinning pass
constexpr int kMaxJ = 64, kMaxSmplS = 16, kMaxSmplxS = 32;
constexpr size_t kLdsDefault = 64 * 1024;

struct Packed {                             // offsets (floats) into the packed model
    int64_t pd, sd, wt, vt, jt, js, sd2, js2, total;
};
// S shape columns; two: set 2 is stored behind set 1 (SMPL: two = 0, and sd2 = js2 = total)
inline Packed layout(int V, int J, int S, int two) {
    Packed p;
    const int64_t P = 9 * (int64_t)(J - 1);
    p.pd = 0;
    p.sd = p.pd + P * 3 * V;
    p.wt = p.sd + (int64_t)S * 3 * V;
    p.vt = p.wt + (int64_t)J * V;
    p.jt = p.vt + 3 * (int64_t)V;
    p.js = p.jt + 3 * J;
    p.sd2 = p.js + 3 * (int64_t)J * S;
    p.js2 = p.sd2 + (two ? (int64_t)S * 3 * V : 0);
    p.total = p.js2 + (two ? 3 * (int64_t)J * S : 0);
    return p;
}

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

// workgroup o = (j 3 + c) (1 + S) + q: q = 0 the template, q >= 1 direction q - 1, read from the transposed arrays vt (3,V), sd (S,3,V).
// Thread t adds the float64 products of vertices t, t + 256, ... in order, then the fixed tree; the sum is rounded to fp32 once.
// jt may be NULL: the template's product is then left as it is.
__global__ __launch_bounds__(kThreads) void k_body_regress(const float *__restrict__ jreg, const float *__restrict__ vt,
                                                           const float *__restrict__ sd, int V, int S, float *__restrict__ jt,
                                                           float *__restrict__ js) {
    __shared__ double sh[kThreads];
    const int o = (int)blockIdx.x, q = o % (1 + S), jc = o / (1 + S), j = jc / 3, c = jc - 3 * j;
    const float *row = jreg + (int64_t)j * V;
    const float *x = q == 0 ? vt + (int64_t)c * V : sd + ((int64_t)(q - 1) * 3 + c) * V;
    double acc = 0.0;
    for (int v = (int)threadIdx.x; v < V; v += kThreads) acc += (double)row[v] * (double)x[v];
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if (q == 0) {
            if (jt) jt[jc] = (float)tot;
        } else {
            js[(int64_t)jc * S + (q - 1)] = (float)tot;
        }
    }
}

struct PoseArgs {
    const float *pd, *sd, *wt, *vt, *jt, *js;      // the packed model
    const int *parents;
    int V, J, P, Sp, S, F;                         // Sp: the packed stride of js (SMPL poses with S <= Sp columns; SMPL-X: Sp = S)
    const float *poses, *shapes, *rt, *big;
    int shapes_stride, rt_stride;                  // shapes_stride 0 (SMPL only: one row for all frames) or S
    float *A, *feat;                               // workspace: (F,J,16), (F,P)
    float *vertices, *joints, *bounds, *verts4, *table, *big_out;
    // read under X only (behind the rest: the kernels' schedules, k_body_skin<8, false>'s registers among them, follow this order)
    const float *sd2, *js2, *transl;               // sd2 / js2: set 2, or set 1 again
    float *t2;                                     // workspace, between A and feat: (F,J,4)
    int second;                                    // a table is asked for and set 2 differs from set 1
};

// Rodrigues with the convention of smplx/lbs.py and of the renderer, angle = |v + 1e-8| (a zero vector gives the identity), K K and
// I + sin K + (1 - cos) K K term by term: rot, row-major 3x3
__device__ __forceinline__ void rodrigues(float x, float y, float z, float rot[9]) {
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
            rot[3 * r + c] = ((r == c ? 1.f : 0.f) + s * K[3 * r + c]) + c1 * kk;
        }
}

template <bool X>
__global__ __launch_bounds__(64) void k_body_joints(PoseArgs a) {
    __shared__ float rot[kMaxJ][9], jr[kMaxJ * 3], L[kMaxJ][16], G[kMaxJ][16];
    __shared__ float jr2[kMaxJ * 3], l2[kMaxJ][3], g2[kMaxJ][3];      // set 2: touched under X only, so the SMPL kernel has none of it
    __shared__ int par[kMaxJ];
    const int64_t f = blockIdx.x;
    const int t = (int)threadIdx.x, J = a.J, S = a.S;
    const float *beta = a.shapes + f * a.shapes_stride;
    if (t < J) {
        const float *pv = a.poses + (f * J + t) * 3;
        float rv[9];
        rodrigues(pv[0], pv[1], pv[2], rv);
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            rot[t][e] = rv[e];
            if (t >= 1) a.feat[f * a.P + (t - 1) * 9 + e] = rv[e] - (e % 4 == 0 ? 1.f : 0.f);
        }
        const int p = t == 0 ? 0 : a.parents[t];
        par[t] = p < 0 ? 0 : (p > t - 1 ? (t == 0 ? 0 : t - 1) : p);      // (the loader refuses such parents; never index outside)
    }
    for (int i = t; i < 3 * J; i += 64) {
        float v = a.jt[i];
        for (int s = 0; s < S; ++s) v += a.js[i * a.Sp + s] * beta[s];
        jr[i] = v;
        if constexpr (X) {
            if (a.second) {
                float w = a.jt[i];
                for (int s = 0; s < S; ++s) w += a.js2[i * a.Sp + s] * beta[s];
                jr2[i] = w;
            }
        }
    }
    __syncthreads();
    if (t < J) {
        const int p = par[t];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) L[t][4 * r + c] = rot[t][3 * r + c];
            L[t][4 * r + 3] = t == 0 ? jr[r] : jr[3 * t + r] - jr[3 * p + r];
            if constexpr (X) {
                if (a.second) l2[t][r] = t == 0 ? jr2[r] : jr2[3 * t + r] - jr2[3 * p + r];
            }
        }
        L[t][12] = 0.f, L[t][13] = 0.f, L[t][14] = 0.f, L[t][15] = 1.f;
    }
    __syncthreads();
    if (t < 16) G[0][t] = L[0][t];
    if constexpr (X) {
        if (a.second && t >= 16 && t < 19) g2[0][t - 16] = l2[0][t - 16];
    }
    for (int i = 1; i < J; ++i) {
        __syncthreads();
        const int p = par[i];
        if (t < 16) {
            const int r = t >> 2, c = t & 3;
            G[i][t] = ((G[p][4 * r] * L[i][c] + G[p][4 * r + 1] * L[i][4 + c]) + G[p][4 * r + 2] * L[i][8 + c]) + G[p][4 * r + 3] * L[i][12 + c];
        } else if constexpr (X) {
            if (a.second && t < 19) {
                const int r = t - 16;   // the same product for column 3 of set 2: the rotation of G[p] is shared, L[i][15] = 1
                g2[i][r] = ((G[p][4 * r] * l2[i][0] + G[p][4 * r + 1] * l2[i][1]) + G[p][4 * r + 2] * l2[i][2]) + g2[p][r] * 1.f;
            }
        }
    }
    __syncthreads();
    if (t < J) {
        const float *g = G[t];
        if (a.joints) {
            const float *rt = a.rt + f * a.rt_stride;
            float q[3] = {g[3], g[7], g[11]};
            if constexpr (X) {
                if (a.transl) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) q[i] = q[i] + a.transl[f * 3 + i];
                }
            }
            float *o = a.joints + (f * J + t) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = ((q[0] * rt[3 * i] + q[1] * rt[3 * i + 1]) + q[2] * rt[3 * i + 2]) + rt[9 + i];
        }
        float *o = a.A + (f * J + t) * 16;
        float *o2 = a.t2 + (f * J + t) * 4;         // X only
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[4 * r] = g[4 * r], o[4 * r + 1] = g[4 * r + 1], o[4 * r + 2] = g[4 * r + 2];
            o[4 * r + 3] = g[4 * r + 3] - ((g[4 * r] * jr[3 * t] + g[4 * r + 1] * jr[3 * t + 1]) + g[4 * r + 2] * jr[3 * t + 2]);
            if constexpr (X) {
                if (r < 3)
                    o2[r] = a.second ? g2[t][r] - ((g[4 * r] * jr2[3 * t] + g[4 * r + 1] * jr2[3 * t + 1]) + g[4 * r + 2] * jr2[3 * t + 2]) : o[4 * r + 3];
            }
        }
        if constexpr (X) o2[3] = 0.f;
    }
}

// floats of a frame in the workspace / staged in LDS by the skinning pass
constexpr size_t ws_floats(bool X, int J) { return (size_t)J * (X ? 20 : 16) + 9 * (size_t)(J - 1); }
constexpr size_t skin_lds_floats(bool X, int FC, int J, int S) {
    return (size_t)FC * ((size_t)J * (X ? 15 : 12) + 9 * (size_t)(J - 1) + S + (X ? 16 : 12));
}
static_assert(skin_lds_floats(true, kChunk, kMaxJ, kMaxSmplxS) * sizeof(float) <= kLdsDefault, "every accepted (J, S) must fit the default dynamic LDS");

template <int FC, bool X>
__global__ __launch_bounds__(kThreads) void k_body_skin(PoseArgs a) {
    extern __shared__ float lds[];
    constexpr int RT = X ? 16 : 12;         // R | Th, X: | transl | pad
    const int J = a.J, P = a.P, S = a.S, V = a.V, tid = (int)threadIdx.x;
    float *sA = lds;                        // [FC][J][12]: rows 0..2 of A (set 1)
    float *sT2 = sA + FC * J * 12;          // X: [FC][J][3]: the translation column of set 2
    float *sF = sT2 + (X ? FC * J * 3 : 0); // [P][FC]
    float *sB = sF + P * FC;                // [S][FC]
    float *sRT = sB + S * FC;               // [FC][RT]
    const int64_t f0 = (int64_t)blockIdx.y * FC;
    const int nf = a.F - f0 < FC ? (int)(a.F - f0) : FC;
    // (a chunk's missing frames are staged as copies of its last one: computed, never stored)
    for (int i = tid; i < FC * J * 12; i += kThreads) {
        const int fl = i / (J * 12), r = i - fl * (J * 12), f = fl < nf ? fl : nf - 1;
        sA[i] = a.A[(f0 + f) * J * 16 + (r / 12) * 16 + r % 12];
    }
    if constexpr (X) {
        for (int i = tid; i < FC * J * 3; i += kThreads) {
            const int fl = i / (J * 3), r = i - fl * (J * 3), f = fl < nf ? fl : nf - 1;
            sT2[i] = a.t2[(f0 + f) * J * 4 + (r / 3) * 4 + r % 3];
        }
    }
    for (int i = tid; i < P * FC; i += kThreads) {
        const int k = i / FC, fl = i - k * FC, f = fl < nf ? fl : nf - 1;
        sF[i] = a.feat[(f0 + f) * P + k];
    }
    for (int i = tid; i < S * FC; i += kThreads) {
        const int s = i / FC, fl = i - s * FC, f = fl < nf ? fl : nf - 1;
        sB[i] = a.shapes[(f0 + f) * a.shapes_stride + s];
    }
    for (int i = tid; i < FC * RT; i += kThreads) {
        const int fl = i / RT, e = i - fl * RT, f = fl < nf ? fl : nf - 1;
        if constexpr (X)
            sRT[i] = e < 12 ? a.rt[(f0 + f) * a.rt_stride + e] : (e < 15 && a.transl ? a.transl[(f0 + f) * 3 + (e - 12)] : 0.f);
        else
            sRT[i] = a.rt[(f0 + f) * a.rt_stride + e];
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
        float T[12], t2[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
        const float *Af = sA + f * J * 12, *Tf = sT2 + f * J * 3;
        for (int j = 0; j < J; ++j) {
            const float w = a.wt[(int64_t)j * V + v];
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] += w * Af[j * 12 + e];
            if constexpr (X) {
#pragma unroll
                for (int e = 0; e < 3; ++e) t2[e] += w * Tf[j * 3 + e];
            }
        }
        const float x = (vt0 + so[0]) + po[f][0], y = (vt1 + so[1]) + po[f][1], z = (vt2 + so[2]) + po[f][2];
        float vs[3], wv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) vs[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
        const float *R = sRT + f * RT, *Th = R + 9;
        if constexpr (X) {
            if (a.transl) {
#pragma unroll
                for (int r = 0; r < 3; ++r) vs[r] = vs[r] + R[12 + r];
            }
        }
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
            const float tx = X ? t2[0] : T[3], ty = X ? t2[1] : T[7], tz = X ? t2[2] : T[11];      // one set: the blend's last column
            float s2[3] = {so[0], so[1], so[2]};
            if constexpr (X) {
                if (a.second) {         // the renderer's shape offset: the first S raw columns
                    s2[0] = s2[1] = s2[2] = 0.f;
                    for (int s = 0; s < S; ++s) {
                        const float b = sB[s * FC + f];
                        s2[0] += a.sd2[(int64_t)(3 * s) * V + v] * b;
                        s2[1] += a.sd2[(int64_t)(3 * s + 1) * V + v] * b;
                        s2[2] += a.sd2[(int64_t)(3 * s + 2) * V + v] * b;
                    }
                }
            }
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
            o[0] = make_float4(tx, ty, tz, i00);
            o[1] = make_float4(i01, i02, i10, i11);
            o[2] = make_float4(i12, i20, i21, i22);
            o[3] = make_float4(po[f][0], po[f][1], po[f][2], s2[0]);
            o[4] = make_float4(s2[1], s2[2], b3.x, b3.y);
            o[5] = make_float4(b3.z, b0.x, b0.y, b0.z);
            o[6] = make_float4(b0.w, b1.x, b1.y, b1.z);
            o[7] = make_float4(b1.w, b2.x, b2.y, b2.z);
            o[8] = make_float4(b2.w, 0.f, 0.f, 0.f);
        }
    }
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

inline bool sizes_ok(int V, int J, int S, int maxS) { return V > 0 && J >= 2 && J <= kMaxJ && S >= 1 && S <= maxS; }

struct TransposeJob {                       // columns [0, K) of in (V,C,cols) -> packed + off, (K,C,V)
    const float *in;
    int C, cols, K;
    int64_t off;
};

// The transposes, then J_regressor applied to the template and to the S directions of set 1 (and of set 2 when `two`), once, in
// float64, from the arrays just transposed.
int pack(const char *name, std::initializer_list<TransposeJob> jobs, const float *J_regressor, int V, int J, int S, int two, float *packed,
         hipStream_t st) {
    for (const TransposeJob &j : jobs) {
        const int64_t n = (int64_t)j.K * j.C * V;
        if (n == 0) continue;
        HL_REQUIRE((n + kThreads - 1) / kThreads <= 0x7fffffff, "%s: model too large", name);
        hipLaunchKernelGGL(k_body_transpose, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, j.in, V, j.C, j.cols, j.K,
                           packed + j.off);
        const int rc = check_launch("k_body_transpose");
        if (rc != HL_OK) return rc;
    }
    const Packed p = layout(V, J, S, two);
    hipLaunchKernelGGL(k_body_regress, dim3(3 * J * (1 + S)), dim3(kThreads), 0, st, J_regressor, packed + p.vt, packed + p.sd, V, S, packed + p.jt,
                       packed + p.js);
    const int rc = check_launch("k_body_regress");
    if (rc != HL_OK || !two) return rc;
    hipLaunchKernelGGL(k_body_regress, dim3(3 * J * (1 + S)), dim3(kThreads), 0, st, J_regressor, packed + p.vt, packed + p.sd2, V, S,
                       (float *)nullptr, packed + p.js2);
    return check_launch("k_body_regress");
}

// What the three pose entry points do, under the name of the one that was called.  X = false: the packed model holds Sp >= S columns
// of one set, shapes_stride is 0 or S, transl is NULL; X = true: Sp = S, shapes_stride = S.
template <bool X>
int pose(const char *name, const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int two, int F, const float *poses,
         const float *shapes, int shapes_stride, const float *transl, const float *rt, int rt_stride, const float *big, float *vertices,
         float *joints, float *bounds, float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin,
         float y_margin, void *stream) {
    constexpr int maxS = X ? kMaxSmplxS : kMaxSmplS;
    HL_REQUIRE(margin >= 0.f && y_margin >= 0.f, "%s: the bounds' margins must not be negative (got %g, %g)", name, (double)margin, (double)y_margin);
    HL_REQUIRE(packed && parents && poses && shapes && rt, "%s: NULL argument", name);
    HL_REQUIRE(sizes_ok(V, J, Sp, maxS) && S >= 1 && S <= Sp && F >= 1,
               "%s: bad sizes (V %d, J %d, Sp %d, S %d, F %d; V > 0, 2 <= J <= %d, 1 <= S <= Sp <= %d, F >= 1)", name, V, J, Sp, S, F, kMaxJ, maxS);
    HL_REQUIRE(shapes_stride == S || (!X && shapes_stride == 0), "%s: shapes_stride must be 0 or S (got %d)", name, shapes_stride);
    HL_REQUIRE(rt_stride == 0 || rt_stride == 12, "%s: rt_stride must be 0 or 12 (got %d)", name, rt_stride);
    HL_REQUIRE(!table || big, "%s: the table needs the big-pose rows (big)", name);
    HL_REQUIRE(!bounds || vertices, "%s: the bounds are taken over `vertices`, which is NULL", name);
    HL_REQUIRE(aligned16({verts4, table, big_out, big}), "%s: verts4, table, big and big_out must be 16-byte aligned", name);
    const size_t need = (size_t)F * ws_floats(X, J) * sizeof(float);
    HL_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", name, workspace_bytes, need);
    const int FC = F == 1 ? 1 : kChunk;
    const int chunks = (F + FC - 1) / FC;
    HL_REQUIRE(chunks <= 65535, "%s: at most %d frames per call (got %d)", name, 65535 * kChunk, F);
    const size_t lds = skin_lds_floats(X, FC, J, S) * sizeof(float);
    HL_REQUIRE(lds <= kLdsDefault, "%s: %d frames of J %d, S %d need %zu bytes of LDS, a workgroup may ask for %zu", name, FC, J, S, lds, kLdsDefault);
    const Packed p = layout(V, J, Sp, two);
    PoseArgs a;
    a.pd = packed + p.pd, a.sd = packed + p.sd, a.wt = packed + p.wt, a.vt = packed + p.vt, a.jt = packed + p.jt, a.js = packed + p.js;
    a.sd2 = two ? packed + p.sd2 : a.sd, a.js2 = two ? packed + p.js2 : a.js;
    a.parents = parents;
    a.V = V, a.J = J, a.P = 9 * (J - 1), a.Sp = Sp, a.S = S, a.F = F, a.second = two && table;
    a.poses = poses, a.shapes = shapes, a.transl = transl, a.rt = rt, a.big = big;
    a.shapes_stride = shapes_stride, a.rt_stride = rt_stride;
    a.A = static_cast<float *>(workspace);
    a.t2 = a.A + (size_t)F * J * 16;
    a.feat = a.t2 + (X ? (size_t)F * J * 4 : 0);
    a.vertices = vertices, a.joints = joints, a.bounds = bounds, a.verts4 = verts4, a.table = table, a.big_out = big_out;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_body_joints<X>, dim3(F), dim3(64), 0, st, a);
    int rc = check_launch("k_body_joints");
    if (rc != HL_OK) return rc;
    if (vertices || verts4 || table || big_out) {
        const dim3 grid((V + kThreads - 1) / kThreads, chunks);
        if (F == 1)
            hipLaunchKernelGGL((k_body_skin<1, X>), grid, dim3(kThreads), lds, st, a);
        else
            hipLaunchKernelGGL((k_body_skin<kChunk, X>), grid, dim3(kThreads), lds, st, a);
        rc = check_launch("k_body_skin");
        if (rc != HL_OK) return rc;
    }
    if (bounds) {
        hipLaunchKernelGGL(k_body_bounds, dim3(F), dim3(kThreads), 0, st, vertices, V, margin, y_margin, bounds);
        rc = check_launch("k_body_bounds");
    }
    return rc;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

// ---- SMPL ----------------------------------------------------------------------------------------------------------------------------
size_t hl_body_packed_bytes(int V, int J, int Sp) {
    return V > 0 && J >= 1 && J <= kMaxJ && Sp >= 1 && Sp <= kMaxSmplS ? (size_t)layout(V, J, Sp, 0).total * sizeof(float) : 0;
}

int hl_body_pack(const float *v_template, const float *shapedirs, int sd_cols, const float *posedirs, const float *J_regressor,
                 const float *weights, int V, int J, int Sp, float *packed, void *stream) {
    HL_REQUIRE(v_template && shapedirs && posedirs && J_regressor && weights && packed, "hl_body_pack: NULL argument");
    HL_REQUIRE(sizes_ok(V, J, Sp, kMaxSmplS), "hl_body_pack: bad sizes (V %d, J %d, Sp %d; V > 0, 2 <= J <= %d, 1 <= Sp <= %d)", V, J, Sp, kMaxJ, kMaxSmplS);
    HL_REQUIRE(sd_cols >= Sp, "hl_body_pack: shapedirs has %d columns, fewer than Sp = %d", sd_cols, Sp);
    const Packed p = layout(V, J, Sp, 0);
    const int P = 9 * (J - 1);
    return pack("hl_body_pack", {{posedirs, 3, P, P, p.pd}, {shapedirs, 3, sd_cols, Sp, p.sd}, {weights, 1, J, J, p.wt}, {v_template, 1, 3, 3, p.vt}},
                J_regressor, V, J, Sp, 0, packed, (hipStream_t)stream);
}

int hl_body_chunk_frames(void) { return kChunk; }

size_t hl_body_pose_workspace_bytes(int J, int F) { return J < 2 || J > kMaxJ || F < 1 ? 0 : (size_t)F * ws_floats(false, J) * sizeof(float); }

int hl_body_pose(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                 int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                 float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, void *stream) {
    return pose<false>("hl_body_pose", packed, parents, V, J, Sp, S, 0, F, poses, shapes, shapes_stride, nullptr, rt, rt_stride, big, vertices, joints,
                       bounds, verts4, table, big_out, workspace, workspace_bytes, 0.05f, 0.05f, stream);
}

int hl_pose_body_margins(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                         int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                         float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin, float y_margin,
                         void *stream) {
    return pose<false>("hl_body_pose", packed, parents, V, J, Sp, S, 0, F, poses, shapes, shapes_stride, nullptr, rt, rt_stride, big, vertices, joints,
                       bounds, verts4, table, big_out, workspace, workspace_bytes, margin, y_margin, stream);
}

// ---- SMPL-X --------------------------------------------------------------------------------------------------------------------------
size_t hl_smplx_packed_bytes(int V, int J, int S, int two_sets) {
    return sizes_ok(V, J, S, kMaxSmplxS) ? (size_t)layout(V, J, S, two_sets != 0).total * sizeof(float) : 0;
}

int hl_smplx_pack(const float *v_template, const float *shapedirs, int sd_cols, int num_betas, int expr_start, int num_expr,
                  const float *posedirs, const float *J_regressor, const float *weights, int V, int J, float *packed, void *stream) {
    HL_REQUIRE(v_template && shapedirs && posedirs && J_regressor && weights && packed, "hl_smplx_pack: NULL argument");
    HL_REQUIRE(num_betas >= 0 && num_expr >= 0 && num_betas + num_expr >= 1, "hl_smplx_pack: bad coefficient counts (betas %d, expression %d)",
               num_betas, num_expr);
    const int S = num_betas + num_expr;
    HL_REQUIRE(sizes_ok(V, J, S, kMaxSmplxS),
               "hl_smplx_pack: bad sizes (V %d, J %d, betas + expression %d; V > 0, 2 <= J <= %d, 1 <= betas + expression <= %d - beyond these "
               "the skinning pass's staged frames would not fit the %zu bytes of LDS a workgroup may ask for)", V, J, S, kMaxJ, kMaxSmplxS, kLdsDefault);
    HL_REQUIRE(expr_start >= num_betas && sd_cols >= S && (num_expr == 0 || expr_start + num_expr <= sd_cols),
               "hl_smplx_pack: shapedirs has %d columns; betas [0, %d) and expression [%d, %d) do not fit", sd_cols, num_betas, expr_start,
               expr_start + num_expr);
    const int two = num_expr > 0 && expr_start != num_betas;
    const Packed p = layout(V, J, S, two);
    const int P = 9 * (J - 1);
    return pack("hl_smplx_pack",
                {{posedirs, 3, P, P, p.pd}, {weights, 1, J, J, p.wt}, {v_template, 1, 3, 3, p.vt}, {shapedirs, 3, sd_cols, num_betas, p.sd},
                 {shapedirs + expr_start, 3, sd_cols, num_expr, p.sd + (int64_t)num_betas * 3 * V}, {shapedirs, 3, sd_cols, two ? S : 0, p.sd2}},
                J_regressor, V, J, S, two, packed, (hipStream_t)stream);
}

int hl_smplx_chunk_frames(void) { return kChunk; }

size_t hl_smplx_pose_workspace_bytes(int J, int F) { return J < 2 || J > kMaxJ || F < 1 ? 0 : (size_t)F * ws_floats(true, J) * sizeof(float); }

int hl_smplx_pose(const float *packed, const int32_t *parents, int V, int J, int S, int two_sets, int F, const float *poses, const float *coef,
                  const float *transl, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                  float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin, float y_margin,
                  void *stream) {
    return pose<true>("hl_smplx_pose", packed, parents, V, J, S, S, two_sets != 0, F, poses, coef, S, transl, rt, rt_stride, big, vertices, joints, bounds,
                      verts4, table, big_out, workspace, workspace_bytes, margin, y_margin, stream);
}

}  // extern "C"
