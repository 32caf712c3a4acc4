// Backward of QKVAttention (improved_diffusion/unet.py:255-274) for the HIP training path - hand-written, fp32, deterministic, flash-style
// (probabilities recomputed, never stored).  Replaces the five torch.bmm (rocBLAS) of round 3's _Attention.backward.
//
// Per (sample, head):  S = (s q)(s k)^T with s = ch^-1/4 on q AND k,  P = softmax_rows(S),  O = P v.   Given dO:
//   dV = P^T dO      dP = dO V^T      D_i = sum_j P_ij dP_ij  (= dO_i . O_i)      dS = P o (dP - D)      dQ = s dS (s k)      dK = s dS^T (s q)
// D is formed as sum_j P_ij dP_ij from the SAME P and dP the dS of the query kernel is formed from, not as dO_i . O_i: the two agree to fp32 rounding only, and
// dQ multiplies dP - D by k.  On a saturated row (one key holds all the probability) the exact dS is 0; with D = dP_top bit for bit it is 0 here too, where
// dO . O left |dO| |v| 2^-24 sqrt(ch) times |k| in dQ.
//
// Two kernels, both in the register-resident transposed style of k_attention / k_march (v_mfma_f32_32x32x2_f32; an accumulator tile IS
// the next product's B operand):
//   k_attn_bwd_q   one wave = 32 queries.  Pass A over the key tiles: row maximum, sum (the forward kernels do not emit them) and D, online.  Pass B:
//                  S^T -> P^T, dP^T = V dO^T, dS^T in registers, dQ^T += K^T dS^T.  Writes dQ and per query (max, 1/sum, D) for the second kernel.
//   k_attn_bwd_kv  one wave = 32 keys, loop over the query tiles: S -> P, dP = dO V^T, dS; dV^T += dO^T P, dK^T += Q^T dS.
// Every output element is owned by one wave and summed in a fixed order: run-to-run identical bits.
// Head sizes that are not a multiple of 32 (the tiny test networks: 8, 16) take a plain two-kernel path that materialises P and dS per head
// in caller scratch.
#include "hl_reduce.h"
#include "hl_unet_kernels.h"

namespace hl {
namespace {

// KS waves of a workgroup share ONE 32-row tile and split the other dimension (every KS-th key tile / query tile each, wave-private LDS
// tiles, no workgroup barrier inside the loops); their partial sums meet in LDS and are added in a fixed order.  The UNet's attention levels
// have 32 / 8 / 2 tiles per head and 8 (sample, head) pairs at microbatch 2: one wave per tile pair left three quarters of the SIMDs idle and
// ran a 1024-key loop serially (565 + 350 us per layer at T = 1024; with the split 1/KS of that).
template <int CH, int KS_>
__global__ __launch_bounds__(KS_ * 64, 1) void k_attn_bwd_q(const float *__restrict__ qkv, const float *__restrict__ out, const float *__restrict__ dout,
                                                            int T, int C, int heads, float *__restrict__ dqkv, float *__restrict__ stat) {
    constexpr int CT = CH / 32, KS = CH / 2, LDK = CH + 1, TILE = 32 * LDK;
    extern __shared__ float lds_q[];                    // per wave: K tile, V tile (2 x 32 x LDK); reused for the partial dQ tiles at the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    float *sK = lds_q + wave * 2 * TILE, *sV = sK + TILE;
    __shared__ float sML[KS_ * 3 * 32];
    const int nh = blockIdx.y, n = nh / heads, head = nh % heads;
    const int q0 = blockIdx.x * 32;
    const float scale = 1.f / sqrtf(sqrtf((float)CH));
    const long pitch = 3L * C;
    const float *base = qkv + (long)n * T * pitch + (long)head * 3 * CH;
    const int qi = q0 + (lane & 31), qj = min(qi, T - 1);
    float qreg[KS], doreg[KS];
    {
        const float *drow = dout + ((long)n * T + qj) * C + head * CH;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            qreg[s] = base[(long)qj * pitch + 2 * s + half] * scale;
            doreg[s] = drow[2 * s + half];
        }
    }
    (void)out;                                          // (the forward's output is not needed: D comes from P and dP, see the head of the file)
    auto load_tile = [&](int k0, bool with_v) {   // wave-private: the wave's own LDS reads of the previous tile are behind it in program order
        for (int e = lane; e < 32 * (CH / 4); e += 64) {
            const int key = e / (CH / 4), c = (e - key * (CH / 4)) * 4;
            const int kk = min(k0 + key, T - 1);
            const f32x4 kv = *reinterpret_cast<const f32x4 *>(base + (long)kk * pitch + CH + c);
            float *dk = sK + key * LDK + c;
            dk[0] = kv[0] * scale; dk[1] = kv[1] * scale; dk[2] = kv[2] * scale; dk[3] = kv[3] * scale;
            if (with_v) {
                const f32x4 vv = *reinterpret_cast<const f32x4 *>(base + (long)kk * pitch + 2 * CH + c);
                float *dv = sV + key * LDK + c;
                dv[0] = vv[0]; dv[1] = vv[1]; dv[2] = vv[2]; dv[3] = vv[3];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto scores = [&](int k0) -> f32x16 {   // st[r] = S(key = k0 + (r&3) + 8 (r>>2) + 4 half, query = lane & 31); keys beyond T masked
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[(lane & 31) * LDK + 2 * s + half], qreg[s], st, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (k0 + (r & 3) + 8 * (r >> 2) + 4 * half >= T) st[r] = -3.0e38f;
        return st;
    };
    auto dprobs = [&]() -> f32x16 {   // dP^T = V dO^T of the staged tile, the layout of scores()
        f32x16 dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[(lane & 31) * LDK + 2 * s + half], doreg[s], dp, 0, 0, 0);
        return dp;
    };
    // pass A: row maximum, sum and sum_j exp(S_ij - max) dP_ij over this wave's key tiles (online, rescaled when the maximum moves), then over the waves
    float mrun = -3.0e38f, lrun = 0.f, drun = 0.f;
    for (int k0 = wave * 32; k0 < T; k0 += 32 * KS_) {
        load_tile(k0, true);
        const f32x16 st = scores(k0);
        const f32x16 dp = dprobs();
        float mx = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mnew = fmaxf(mrun, mx);
        float psum = 0.f, dsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __expf(st[r] - mnew);     // masked keys: 0 (their dP is that of the clamped key: finite)
            psum += e;
            dsum += e * dp[r];
        }
        psum += __shfl_xor(psum, 32);
        dsum += __shfl_xor(dsum, 32);
        const float alpha = __expf(mrun - mnew);
        lrun = lrun * alpha + psum;
        drun = drun * alpha + dsum;
        mrun = mnew;
        __builtin_amdgcn_wave_barrier();
    }
    if (half == 0) { sML[(wave * 3) * 32 + lane] = mrun; sML[(wave * 3 + 1) * 32 + lane] = lrun; sML[(wave * 3 + 2) * 32 + lane] = drun; }
    __syncthreads();
    {
        float m = -3.0e38f, l = 0.f, d = 0.f;
#pragma unroll
        for (int w = 0; w < KS_; ++w) m = fmaxf(m, sML[(w * 3) * 32 + (lane & 31)]);
#pragma unroll
        for (int w = 0; w < KS_; ++w) {
            const float a = __expf(sML[(w * 3) * 32 + (lane & 31)] - m);     // waves without keys: l = d = 0
            l += sML[(w * 3 + 1) * 32 + (lane & 31)] * a;
            d += sML[(w * 3 + 2) * 32 + (lane & 31)] * a;
        }
        mrun = m; lrun = l; drun = d;
    }
    const float invl = 1.f / lrun;
    const float D = drun * invl;
    if (wave == 0 && half == 0 && qi < T) {
        float *sp = stat + ((long)nh * T + qi) * 3;
        sp[0] = mrun; sp[1] = invl; sp[2] = D;
    }
    // pass B: dQ^T[c][q] += K^T[c][key] dS^T[key][q] over this wave's key tiles
    f32x16 o[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[c][r] = 0.f;
    for (int k0 = wave * 32; k0 < T; k0 += 32 * KS_) {
        load_tile(k0, true);
        f32x16 st = scores(k0);
        const f32x16 dp = dprobs();
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = __expf(st[r] - mrun) * invl * (dp[r] - D);    // masked keys: exp(-inf) = 0
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int key = (s & 3) + 8 * (s >> 2) + 4 * half;
                o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[key * LDK + c * 32 + (lane & 31)], st[s], o[c], 0, 0, 0);
            }
        __builtin_amdgcn_wave_barrier();
    }
    // the waves' partial dQ tiles meet in LDS ([wave][CT * 16][64 lanes], inside the wave's own tile space) and are added in wave order
    __syncthreads();
    float *part = lds_q + wave * 2 * TILE;
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[(c * 16 + r) * 64 + lane] = o[c][r];
    __syncthreads();
    if (qi < T) {
        float *dst = dqkv + ((long)n * T + qi) * pitch + (long)head * 3 * CH;
        for (int e = wave; e < CT * 16; e += KS_) {      // register rows split over the waves
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < KS_; ++w) v += lds_q[w * 2 * TILE + e * 64 + lane];
            const int c = e >> 4, r = e & 15;
            dst[c * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = v * scale;
        }
    }
}

template <int CH, int KS_>
__global__ __launch_bounds__(KS_ * 64, 1) void k_attn_bwd_kv(const float *__restrict__ qkv, const float *__restrict__ dout, const float *__restrict__ stat,
                                                             int T, int C, int heads, float *__restrict__ dqkv) {
    constexpr int CT = CH / 32, KS = CH / 2, LDK = CH + 1, TILE = 32 * LDK;
    extern __shared__ float lds_k[];                    // per wave: Q tile, dO tile, 96 floats of (max, 1/sum, D); reused for the partial dK / dV tiles
    constexpr int WSZ = 2 * TILE + 96 + ((2 * TILE + 96) & 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    float *sQ = lds_k + wave * WSZ, *sD = sQ + TILE, *sS = sD + TILE;
    const int nh = blockIdx.y, n = nh / heads, head = nh % heads;
    const int k0 = blockIdx.x * 32;
    const float scale = 1.f / sqrtf(sqrtf((float)CH));
    const long pitch = 3L * C;
    const float *base = qkv + (long)n * T * pitch + (long)head * 3 * CH;
    const int ki = k0 + (lane & 31), kj = min(ki, T - 1);
    float kreg[KS], vreg[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        kreg[s] = base[(long)kj * pitch + CH + 2 * s + half] * scale;
        vreg[s] = base[(long)kj * pitch + 2 * CH + 2 * s + half];
    }
    f32x16 dk[CT], dv[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[c][r] = 0.f; dv[c][r] = 0.f; }
    for (int q0 = wave * 32; q0 < T; q0 += 32 * KS_) {
        for (int e = lane; e < 32 * (CH / 4); e += 64) {
            const int q = e / (CH / 4), c = (e - q * (CH / 4)) * 4;
            const int qq = min(q0 + q, T - 1);
            const f32x4 qv = *reinterpret_cast<const f32x4 *>(base + (long)qq * pitch + c);
            const f32x4 dd = *reinterpret_cast<const f32x4 *>(dout + ((long)n * T + qq) * C + head * CH + c);
            float *a = sQ + q * LDK + c, *b = sD + q * LDK + c;
            a[0] = qv[0] * scale; a[1] = qv[1] * scale; a[2] = qv[2] * scale; a[3] = qv[3] * scale;
            b[0] = dd[0]; b[1] = dd[1]; b[2] = dd[2]; b[3] = dd[3];
        }
        for (int e = lane; e < 96; e += 64) {
            const int q = e / 3, j = e - q * 3;
            sS[e] = q0 + q < T ? stat[((long)nh * T + q0 + q) * 3 + j] : (j == 0 ? 3.0e38f : 0.f);   // queries beyond T: max = +huge, 1/sum = 0 -> P = 0
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(sQ[(lane & 31) * LDK + 2 * s + half], kreg[s], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sD[(lane & 31) * LDK + 2 * s + half], vreg[s], dp, 0, 0, 0);
        }
        // st[r] = S(query = q0 + (r&3) + 8 (r>>2) + 4 half, key = lane & 31)
        f32x16 ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float p = __expf(st[r] - sS[q * 3]) * sS[q * 3 + 1];
            st[r] = p;
            ds[r] = p * (dp[r] - sS[q * 3 + 2]);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int q = (s & 3) + 8 * (s >> 2) + 4 * half;
                dv[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sD[q * LDK + c * 32 + (lane & 31)], st[s], dv[c], 0, 0, 0);
                dk[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sQ[q * LDK + c * 32 + (lane & 31)], ds[s], dk[c], 0, 0, 0);
            }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    float *part = lds_k + wave * WSZ;                    // [2 CT * 16][64]: 2 * CT * 1024 floats <= 2 * TILE
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) { part[(c * 16 + r) * 64 + lane] = dk[c][r]; part[((CT + c) * 16 + r) * 64 + lane] = dv[c][r]; }
    __syncthreads();
    if (ki < T) {
        float *dst = dqkv + ((long)n * T + ki) * pitch + (long)head * 3 * CH;
        for (int e = wave; e < 2 * CT * 16; e += KS_) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < KS_; ++w) v += lds_k[w * WSZ + e * 64 + lane];
            const int isv = e >= CT * 16, ee = isv ? e - CT * 16 : e, c = ee >> 4, r = ee & 15;
            const int cc = c * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (isv) dst[2 * CH + cc] = v; else dst[CH + cc] = v * scale;
        }
    }
}

// ---- any head size: P and dS rows materialised in scratch ([nh][T][T] each), then three plain products ----
__global__ void k_attn_bwd_rows(const float *__restrict__ qkv, const float *__restrict__ out, const float *__restrict__ dout, int T, int C, int heads,
                                int ch, float *__restrict__ P, float *__restrict__ dS) {
    // one 64-lane block per (query, sample-head)
    const int q = blockIdx.x, nh = blockIdx.y, n = nh / heads, head = nh % heads, lane = threadIdx.x;
    const float s2 = 1.f / sqrtf((float)ch);
    const long pitch = 3L * C;
    const float *base = qkv + (long)n * T * pitch + (long)head * 3 * ch;
    const float *qr = base + (long)q * pitch, *orow = out + ((long)n * T + q) * C + head * ch, *drow = dout + ((long)n * T + q) * C + head * ch;
    float *prow = P + ((long)nh * T + q) * T, *srow = dS + ((long)nh * T + q) * T;
    float mx = -3.0e38f;
    for (int j = lane; j < T; j += 64) {
        const float *kr = base + (long)j * pitch + ch;
        float s = 0.f;
        for (int c = 0; c < ch; ++c) s = fmaf(qr[c], kr[c], s);
        s *= s2;
        prow[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_xor_max(mx);
    float sum = 0.f;
    for (int j = lane; j < T; j += 64) { const float e = __expf(prow[j] - mx); prow[j] = e; sum += e; }
    sum = wave_xor_sum(sum);
    (void)orow;                                         // (D = sum_j P_ij dP_ij from the same P and dP as dS below, not dO . O: see the head of the file)
    const float inv = 1.f / sum;
    float D = 0.f;
    for (int j = lane; j < T; j += 64) {
        const float *vr = base + (long)j * pitch + 2 * ch;
        float dp = 0.f;
        for (int c = 0; c < ch; ++c) dp = fmaf(drow[c], vr[c], dp);
        const float p = prow[j] * inv;
        prow[j] = p;
        srow[j] = dp;
        D = fmaf(p, dp, D);
    }
    D = wave_xor_sum(D);
    for (int j = lane; j < T; j += 64) srow[j] = prow[j] * (srow[j] - D);
}
__global__ void k_attn_bwd_products(const float *__restrict__ qkv, const float *__restrict__ dout, const float *__restrict__ P, const float *__restrict__ dS,
                                    int N, int T, int C, int heads, int ch, float *__restrict__ dqkv) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per element of dqkv
    if (i >= (long)N * T * 3 * C) return;
    const int cc = (int)(i % (3L * C));
    const long nt = i / (3L * C);
    const int t = (int)(nt % T), n = (int)(nt / T);
    const int head = cc / (3 * ch), part = (cc - head * 3 * ch) / ch, c = cc - head * 3 * ch - part * ch;
    const long nh = (long)n * heads + head, pitch = 3L * C;
    const float *base = qkv + (long)n * T * pitch + (long)head * 3 * ch;
    const float s2 = 1.f / sqrtf((float)ch);
    float acc = 0.f;
    if (part == 0) {          // dQ[t][c] = s2 sum_j dS[t][j] k[j][c]
        const float *r = dS + (nh * T + t) * T;
        for (int j = 0; j < T; ++j) acc = fmaf(r[j], base[(long)j * pitch + ch + c], acc);
        acc *= s2;
    } else if (part == 1) {   // dK[t][c] = s2 sum_i dS[i][t] q[i][c]
        for (int q = 0; q < T; ++q) acc = fmaf(dS[(nh * T + q) * T + t], base[(long)q * pitch + c], acc);
        acc *= s2;
    } else {                  // dV[t][c] = sum_i P[i][t] dO[i][c]
        for (int q = 0; q < T; ++q) acc = fmaf(P[(nh * T + q) * T + t], dout[((long)n * T + q) * C + head * ch + c], acc);
    }
    dqkv[i] = acc;
}

}  // namespace

// head sizes with a register-resident kernel pair (HL_ATTB below); every other size takes the row kernels, whose scratch holds P and dS.
// ONE predicate for the scratch size and for the dispatch (round-4 advisor: 160 was sized as fast and dispatched as generic).
static bool attn_bwd_fast(int C, int ch) {
    return (3L * C) % 4 == 0 && (ch == 32 || ch == 64 || ch == 96 || ch == 128 || ch == 192);
}

size_t attention_backward_scratch_bytes(int N, int T, int C, int heads) {
    const int ch = heads > 0 ? C / heads : 0;
    if (attn_bwd_fast(C, ch)) return (size_t)N * heads * T * 3 * sizeof(float) + 256;
    return (size_t)2 * N * heads * T * T * sizeof(float) + 256;
}

int attention_backward(const float *qkv, const float *out, const float *dout, int N, int T, int C, int heads, float *dqkv, void *scratch,
                       size_t scratch_bytes, hipStream_t st) {
    HL_REQUIRE(qkv && out && dout && dqkv && scratch && heads > 0 && C % heads == 0 && N > 0 && T > 0, "attention_backward: bad argument");
    HL_REQUIRE(scratch_bytes >= attention_backward_scratch_bytes(N, T, C, heads), "attention_backward: scratch too small");
    const int ch = C / heads;
    float *sc = (float *)scratch;
    const int tiles = (T + 31) / 32;
    const dim3 grid(tiles, N * heads);
    // waves per workgroup = how many ways the other dimension is split: 4 while the wave-private tiles fit LDS (head sizes <= 96), else 2
#define HL_ATTB(CH_)                                                                                                                       \
    do {                                                                                                                                   \
        constexpr int KS_ = CH_ <= 96 ? 4 : 2;                                                                                             \
        constexpr size_t lq = (size_t)KS_ * 2 * 32 * (CH_ + 1) * sizeof(float), lk = (size_t)KS_ * (2 * 32 * (CH_ + 1) + 96) * sizeof(float);  \
        int rc_ = launch_lds<k_attn_bwd_q<CH_, KS_>>("k_attn_bwd_q", lq, grid, dim3(KS_ * 64), lq, st, qkv, out, dout, T, C, heads, dqkv, sc);   \
        if (rc_) return rc_;                                                                                                               \
        return launch_lds<k_attn_bwd_kv<CH_, KS_>>("k_attn_bwd_kv", lk, grid, dim3(KS_ * 64), lk, st, qkv, dout, sc, T, C, heads, dqkv);     \
    } while (0)
    switch (attn_bwd_fast(C, ch) ? ch : -1) {
        case 32: HL_ATTB(32); break;
        case 64: HL_ATTB(64); break;
        case 96: HL_ATTB(96); break;
        case 128: HL_ATTB(128); break;
        case 192: HL_ATTB(192); break;
        default: {
            float *P = sc, *dS = sc + (size_t)N * heads * T * T;
            hipLaunchKernelGGL(k_attn_bwd_rows, dim3(T, N * heads), dim3(64), 0, st, qkv, out, dout, T, C, heads, ch, P, dS);
            const long total = (long)N * T * 3 * C;
            hipLaunchKernelGGL(k_attn_bwd_products, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, qkv, dout, P, dS, N, T, C, heads, ch, dqkv);
        }
    }
#undef HL_ATTB
    return check_launch("attention_backward");
}

}  // namespace hl
