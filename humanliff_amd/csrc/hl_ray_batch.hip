// Training ray batches drawn on the device from resident views, MI355X (gfx950): the split == 'train' half of sample_ray_batch
// (recon_NeRF/lib/if_nerf_data_utils.py:87-170 of the reference) without its per-call host work.  Contract: DESIGN.md 4g.
//
// Once per stored view (hl_ray_views_prepare):
// k_view_classes: grid (V * H), one workgroup per image row, one wave per 64-pixel word.  bound_mask (get_bound_2d_mask :36-47) is the
//   union of six quads of the 8 projected box corners, which the host rounds to integers exactly as the reference does; a pixel is in a
//   quad when it lies inside or on the boundary of the closed polygon, decided in 64-bit integer arithmetic (even-odd crossings plus
//   on-segment).  Class 0 = bound & body (msk * bound_mask == 1, :97 / :120), class 1 = bound & ~body (:130).  One __ballot per class
//   is one word of the class's bitmap; the row's popcounts go to the row table.
// k_view_row_prefix: grid (V * 2).  Exclusive prefix of a class's row counts, in place, the total at [H].
//   The k-th pixel of a class in np.argwhere order = binary search of the row table, then a popcount select across the row's words.
//
// Once per batch (hl_ray_batch):
// k_ray_batch: grid (bs), one workgroup per batch entry, the loop of :115-161.  Round r with m rays missing: n_body = (int)(m * ratio)
//   candidates of class 0, then m - n_body of class 1, each the pick-th pixel of its class (picks injected, or a Philox4x32-10 draw
//   keyed by (seed, step) with counter (slot, entry, 2 round + class), x -> mulhi(x, count)).  The candidate's ray is camera_ray_pixel
//   (csrc/hl_camera.h), the function k_camera_rays runs, in its train-split arithmetic (the box test on the float64 rays, as
//   :146-149 does); candidates that cross the padded box exactly twice are appended in candidate order: ballot within the wave, wave
//   offsets through LDS.  Rows still missing after max_rounds are zeros with near 0 / far 1.
// Plain vector stores only, no atomics: the same inputs give the same bits.
#include "hl_camera.h"

#include <cstdint>

namespace hl {
namespace {

constexpr int kPrepThreads = 256;            // 4 waves: 4 words of a row per pass
constexpr int kBatchThreads = 1024;          // 16 waves: a 2048-ray round is two passes
constexpr int kBatchWaves = kBatchThreads / 64;

typedef unsigned long long u64;

// (x, y) inside or on the boundary of the closed quad q[0..3] (a bow-tie counts by the even-odd rule).  |coordinates| < 2^30, so every
// product below stays inside int64.
__device__ __forceinline__ bool in_closed_quad(const int (&qx)[4], const int (&qy)[4], long long x, long long y) {
    bool inside = false, edge = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long ax = qx[i], ay = qy[i], bx = qx[(i + 1) & 3], by = qy[(i + 1) & 3];
        const long long cross = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
        const long long x0 = ax < bx ? ax : bx, x1 = ax < bx ? bx : ax, y0 = ay < by ? ay : by, y1 = ay < by ? by : ay;
        edge |= cross == 0 && x >= x0 && x <= x1 && y >= y0 && y <= y1;
        if ((ay > y) != (by > y)) {                                   // half-open: a vertex counts for the edge it is the lower end of
            const long long t = (x - ax) * (by - ay) - (y - ay) * (bx - ax);
            inside ^= by > ay ? t < 0 : t > 0;
        }
    }
    return inside || edge;
}

__global__ __launch_bounds__(kPrepThreads) void k_view_classes(const int *__restrict__ corners, const unsigned char *__restrict__ body,
                                                               int H, int W, int nw, u64 *__restrict__ bitmaps,
                                                               int *__restrict__ row_table) {
    __shared__ int sh[kPrepThreads / 64][2];
    const long long row = blockIdx.x;                                 // v * H + y
    const long long v = row / H;
    const int y = (int)(row - v * H);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int cx[8], cy[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        cx[i] = corners[(v * 8 + i) * 2];
        cy[i] = corners[(v * 8 + i) * 2 + 1];
    }
    constexpr int Q[6][4] = {{0, 1, 3, 2}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 3, 7, 5}};   // get_bound_2d_mask :41-46
    int n0 = 0, n1 = 0;
    for (int w = wave; w < nw; w += kPrepThreads / 64) {
        const int x = w * 64 + lane;
        bool bound = false;
        if (x < W) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int qx[4] = {cx[Q[q][0]], cx[Q[q][1]], cx[Q[q][2]], cx[Q[q][3]]};
                const int qy[4] = {cy[Q[q][0]], cy[Q[q][1]], cy[Q[q][2]], cy[Q[q][3]]};
                bound |= in_closed_quad(qx, qy, x, y);
            }
        }
        const bool is_body = x < W && body[row * W + x] != 0;
        const u64 b0 = __ballot(bound && is_body), b1 = __ballot(bound && !is_body);
        if (lane == 0) {
            bitmaps[((v * 2 + 0) * H + y) * nw + w] = b0;
            bitmaps[((v * 2 + 1) * H + y) * nw + w] = b1;
        }
        n0 += __builtin_popcountll(b0);
        n1 += __builtin_popcountll(b1);
    }
    if (lane == 0) {
        sh[wave][0] = n0;
        sh[wave][1] = n1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < kPrepThreads / 64; ++i) tot += sh[i][threadIdx.x];
        row_table[(v * 2 + threadIdx.x) * (H + 1) + y] = tot;
    }
}

// counts [0, H) -> exclusive prefix [0, H], in place: thread t owns one contiguous piece
__global__ __launch_bounds__(kPrepThreads) void k_view_row_prefix(int *__restrict__ row_table, int H) {
    __shared__ int sh[kPrepThreads];
    int *p = row_table + (long long)blockIdx.x * (H + 1);
    const int t = (int)threadIdx.x, piece = (H + kPrepThreads - 1) / kPrepThreads;
    const int s = t * piece < H ? t * piece : H, e = s + piece < H ? s + piece : H;
    int sum = 0;
    for (int i = s; i < e; ++i) sum += p[i];
    sh[t] = sum;
    __syncthreads();
    int run = 0;
    for (int i = 0; i < t; ++i) run += sh[i];
    for (int i = s; i < e; ++i) {
        const int c = p[i];
        p[i] = run;
        run += c;
    }
    if (t == kPrepThreads - 1) p[H] = run;                            // (the last thread's running sum is the total)
}

// position of the k-th (from 0) set bit of w; k < popcount(w)
__device__ __forceinline__ int select_bit(u64 w, int k) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const int c = __builtin_popcountll((w >> pos) & ((1ull << width) - 1ull));
        if (k >= c) {
            k -= c;
            pos += width;
        }
    }
    return pos;
}

// Philox4x32-10 (Salmon et al., SC'11), first output word
__device__ __forceinline__ unsigned philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

struct BatchArgs {
    const int64_t *image_idx;
    const void *images;
    const u64 *bitmaps;
    const int *row_table;
    const CamView *cameras;
    const int *picks;
    long long V;
    int H, W, nw, n, max_rounds, images_u8;
    double ratio;
    unsigned key0, key1, step;
    float *rgb, *ray_o, *ray_d, *near, *far, *bkgd;
    unsigned char *mask;
    int *coord, *n_valid;
};

__global__ __launch_bounds__(kBatchThreads) void k_ray_batch(const BatchArgs a) {
    __shared__ int sh_wave[kBatchWaves];
    __shared__ int sh_bad;
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, H = a.H, W = a.W;
    const long long out0 = (long long)e * n;
    const long long v = a.image_idx[e];
    if (tid == 0) sh_bad = v < 0 || v >= a.V;
    __syncthreads();
    int filled = 0;
    if (v >= 0 && v < a.V) {                                          // (uniform over the workgroup)
        const CamView cam = a.cameras[v];
        const int *pre[2] = {a.row_table + (v * 2 + 0) * (H + 1), a.row_table + (v * 2 + 1) * (H + 1)};
        const int count[2] = {pre[0][H], pre[1][H]};
        for (int r = 0; r < a.max_rounds && filled < n; ++r) {
            const int m = n - filled;
            int n_body = (int)((double)m * a.ratio);                  // :116, in double as Python evaluates it
            n_body = n_body < 0 ? 0 : n_body > m ? m : n_body;
            for (int base = 0; base < m; base += kBatchThreads) {
                const int s = base + tid;
                bool keep = false;
                int px = 0, py = 0, c = 0;
                float of[3], df[3], near = 0.f, far = 1.f;
                if (s < m) {
                    c = s < n_body ? 0 : 1;
                    const int slot = c ? s - n_body : s;
                    long long k;
                    if (a.picks) k = a.picks[(((long long)e * a.max_rounds + r) * 2 + c) * n + slot];
                    else k = __umulhi(philox((unsigned)slot, (unsigned)e, (unsigned)(2 * r + c), a.step, a.key0, a.key1), (unsigned)count[c]);
                    if (k < 0 || k >= count[c]) {
                        sh_bad = 1;                                   // an index np.argwhere's list does not have (an empty class included)
                    } else {
                        const int *p = pre[c];
                        int lo = 0, hi = H;                           // p[lo] <= k < p[hi]
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (p[mid] <= k) lo = mid;
                            else hi = mid;
                        }
                        py = lo;
                        int kk = (int)k - p[lo];
                        const u64 *words = a.bitmaps + ((v * 2 + c) * H + py) * a.nw;
                        for (int w = 0; w < a.nw; ++w) {
                            const u64 word = words[w];
                            const int pc = __builtin_popcountll(word);
                            if (kk < pc) {
                                px = w * 64 + select_bit(word, kk);
                                break;
                            }
                            kk -= pc;
                        }
                        keep = camera_ray_pixel<true>(cam, px, py, of, df, near, far);
                    }
                }
                const u64 bal = __ballot(keep);
                if (lane == 0) sh_wave[wave] = __builtin_popcountll(bal);
                __syncthreads();
                int off = 0, tot = 0;
#pragma unroll
                for (int w = 0; w < kBatchWaves; ++w) {
                    const int cw = sh_wave[w];
                    off += w < wave ? cw : 0;
                    tot += cw;
                }
                __syncthreads();                                      // (sh_wave is rewritten by the next pass)
                if (keep) {
                    const long long row = out0 + filled + off + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                    const long long pix = (v * H + py) * W + px;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        a.rgb[row * 3 + ch] = a.images_u8 ? (float)static_cast<const unsigned char *>(a.images)[pix * 3 + ch] / 255.0f
                                                          : static_cast<const float *>(a.images)[pix * 3 + ch];
                        a.ray_o[row * 3 + ch] = of[ch];
                        a.ray_d[row * 3 + ch] = df[ch];
                    }
                    a.near[row] = near;
                    a.far[row] = far;
                    a.bkgd[row] = c == 0 ? 1.f : 0.f;
                    a.mask[row] = 1;
                    a.coord[row * 2] = py;
                    a.coord[row * 2 + 1] = px;
                }
                filled += tot;
            }
        }
    }
    for (int i = filled + tid; i < n; i += kBatchThreads) {           // rows the loop did not reach
        const long long row = out0 + i;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            a.rgb[row * 3 + ch] = 0.f;
            a.ray_o[row * 3 + ch] = 0.f;
            a.ray_d[row * 3 + ch] = 0.f;
        }
        a.near[row] = 0.f;
        a.far[row] = 1.f;
        a.bkgd[row] = 0.f;
        a.mask[row] = 0;
        a.coord[row * 2] = 0;
        a.coord[row * 2 + 1] = 0;
    }
    __syncthreads();
    if (tid == 0) a.n_valid[e] = sh_bad ? -1 : filled;
}

inline bool view_shape_ok(long long V, int H, int W) {
    return V > 0 && H > 0 && W > 0 && V * H <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL / 3;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_camera_table_row(const double *h_Kinv, const double *h_R, const double *h_T, const double *h_bounds, double *h_row) {
    HL_REQUIRE(h_Kinv && h_R && h_T && h_bounds && h_row, "hl_camera_table_row: NULL argument");
    CamView c;
    cam_view_fill(h_Kinv, h_R, h_T, h_bounds, c);
    memcpy(h_row, &c, sizeof(c));
    return HL_OK;
}

int hl_ray_views_prepare(const int32_t *corners, const unsigned char *body, int64_t V, int H, int W, uint64_t *bitmaps, int32_t *row_table,
                         void *stream) {
    HL_REQUIRE(corners && body && bitmaps && row_table, "hl_ray_views_prepare: NULL argument");
    HL_REQUIRE(view_shape_ok(V, H, W), "hl_ray_views_prepare: bad shape (%lld views of %d x %d; V H < 2^31, 3 H W < 2^31)", (long long)V, H, W);
    const int nw = (W + 63) / 64;
    hipLaunchKernelGGL(k_view_classes, dim3((unsigned)(V * H)), dim3(kPrepThreads), 0, (hipStream_t)stream, corners, body, H, W, nw,
                       reinterpret_cast<u64 *>(bitmaps), row_table);
    int rc = check_launch("k_view_classes");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_view_row_prefix, dim3((unsigned)(V * 2)), dim3(kPrepThreads), 0, (hipStream_t)stream, row_table, H);
    return check_launch("k_view_row_prefix");
}

int hl_ray_batch(const int64_t *image_idx, int bs, const void *images, int images_u8, const uint64_t *bitmaps, const int32_t *row_table,
                 const double *cameras, int64_t V, int H, int W, int n_rays, double ratio, const int32_t *picks, uint64_t seed, uint64_t step,
                 int max_rounds, float *rgb, float *ray_o, float *ray_d, float *near, float *far, float *bkgd_msk,
                 unsigned char *mask_at_box, int32_t *coord, int32_t *n_valid, void *stream) {
    HL_REQUIRE(image_idx && images && bitmaps && row_table && cameras && rgb && ray_o && ray_d && near && far && bkgd_msk && mask_at_box &&
                   coord && n_valid, "hl_ray_batch: NULL argument");
    HL_REQUIRE(view_shape_ok(V, H, W), "hl_ray_batch: bad shape (%lld views of %d x %d)", (long long)V, H, W);
    HL_REQUIRE(bs > 0 && n_rays > 0 && max_rounds > 0 && (long long)bs * n_rays <= 0x7fffffffLL / 3,
               "hl_ray_batch: bad sizes (bs %d, n_rays %d, max_rounds %d)", bs, n_rays, max_rounds);
    HL_REQUIRE(ratio >= 0.0 && ratio <= 1.0, "hl_ray_batch: ratio must be in [0, 1] (got %g)", ratio);
    BatchArgs a{};
    a.image_idx = image_idx; a.images = images; a.bitmaps = reinterpret_cast<const u64 *>(bitmaps); a.row_table = row_table;
    a.cameras = reinterpret_cast<const CamView *>(cameras); a.picks = picks;
    a.V = V; a.H = H; a.W = W; a.nw = (W + 63) / 64; a.n = n_rays; a.max_rounds = max_rounds; a.images_u8 = images_u8 ? 1 : 0;
    a.ratio = ratio;
    a.key0 = (unsigned)seed; a.key1 = (unsigned)(seed >> 32) ^ (unsigned)(step >> 32); a.step = (unsigned)step;
    a.rgb = rgb; a.ray_o = ray_o; a.ray_d = ray_d; a.near = near; a.far = far; a.bkgd = bkgd_msk; a.mask = mask_at_box;
    a.coord = coord; a.n_valid = n_valid;
    hipLaunchKernelGGL(k_ray_batch, dim3((unsigned)bs), dim3(kBatchThreads), 0, (hipStream_t)stream, a);
    return check_launch("k_ray_batch");
}

}  // extern "C"
