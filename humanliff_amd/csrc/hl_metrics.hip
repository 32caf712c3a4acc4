// Held-out view scores on the device, MI355X (gfx950): masked MSE / PSNR, the mask's bounding rectangle and skimage's SSIM on the crop
// (recon_NeRF/lib/all_test.py:19-42, 175-188 of the reference: psnr_metric, ssim_metric, to8b).  Contract: DESIGN.md "Evaluation".
// Four small launches per call, every sum in float64 and in a fixed order (no float atomics), nothing read back by the host:
//
// k_metrics_pixels: grid (chunks, V).  A workgroup owns kPixChunk pixels of one view: the fp32 difference of every masked value, its
//   float64 square, the count and the smallest / largest masked column and row; optionally the two uint8 images (to8b of the masked
//   prediction and of the unmasked ground truth).  One partial per workgroup.
// k_metrics_box: grid (V).  Adds / min-maxes a view's partials in a fixed order and writes mse, psnr, count and the box of its record.
// k_metrics_ssim: grid (tiles of the worst case (W-6) x (H-6), V).  Reads the view's box from its record; tile (bx, by) owns the 16 x 16
//   window origins (box.x + 16 bx + i, box.y + 16 by + j) - aligned to the crop, so the same crop gives the same sums wherever it
//   sits in the image.  The 22 x 22 masked pixels it needs are staged in LDS as fp32 (exact), then per channel a row pass (7-sums of
//   x, y, xx, yy, xy in float64) and a column pass (7-sums of those) give the 49-sums of every window; S follows skimage's
//   expression order.  One partial of three channel sums per workgroup; a workgroup outside the crop's interior writes zeros.
// k_metrics_ssim_finish: grid (V).  Adds the tiles' partials in a fixed order (hl_reduce.h), the channels' means, their mean -> ssim of the record.
#include "hl_reduce.h"

#include <climits>
#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kThreads = 256;
constexpr int kPixChunk = 4096;             // pixels of a view per workgroup (k_metrics_pixels)
constexpr int kTile = 16;                   // window origins per tile side
constexpr int kWin = 7;                     // skimage's default win_size
constexpr int kHalo = kTile + kWin - 1;     // 22 pixels per tile side
static_assert(kTile * kTile == kThreads, "one thread per window origin of a tile");
static_assert(kThreads == kReduceThreads, "block_reduce / strided_sum reduce a workgroup of kReduceThreads");

struct PixPartial {
    double sse;
    int count, x0, x1, y0, y1, pad;         // x0 / y0: smallest masked column / row (INT_MAX if none), x1 / y1: largest (-1 if none)
};
static_assert(sizeof(PixPartial) == 32, "workspace layout");
static_assert(sizeof(hl_metrics_record) == 48, "record layout (humanliff_amd/metrics.py reads it as 6 float64 / 12 int32)");

__device__ __forceinline__ unsigned char to8b(float x) {      // (255 * np.clip(x, 0, 1)).astype(np.uint8); NaN -> 0
    const float c = fminf(fmaxf(x, 0.f), 1.f);
    return (unsigned char)(int)(255.f * c);
}

__global__ __launch_bounds__(kThreads) void k_metrics_pixels(const float *__restrict__ pred, const float *__restrict__ gt,
                                                             const unsigned char *__restrict__ mask, int H, int W,
                                                             unsigned char *__restrict__ pred_u8, unsigned char *__restrict__ gt_u8,
                                                             PixPartial *__restrict__ partial) {
    __shared__ double shd[kThreads];
    __shared__ int shi[kThreads];
    const int HW = H * W;                   // (3 HW < 2^31: the host refuses larger views)
    const int64_t v = blockIdx.y;
    const int s = (int)blockIdx.x * kPixChunk, e = HW - s > kPixChunk ? s + kPixChunk : HW;
    const float *p = pred + v * 3 * HW, *g = gt + v * 3 * HW;
    const unsigned char *m = mask + v * HW;
    double sse = 0.0;
    int count = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    for (int i = s + (int)threadIdx.x; i < e; i += kThreads) {
        const bool in = m[i] != 0;
        const float p0 = p[3 * i], p1 = p[3 * i + 1], p2 = p[3 * i + 2];
        const float g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
        if (in) {
            const double d0 = (double)(p0 - g0), d1 = (double)(p1 - g1), d2 = (double)(p2 - g2);
            sse += d0 * d0;
            sse += d1 * d1;
            sse += d2 * d2;
            const int y = (int)((unsigned)i / (unsigned)W), x = i - y * W;
            ++count;
            x0 = x < x0 ? x : x0;
            x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0;
            y1 = y > y1 ? y : y1;
        }
        if (pred_u8) {
            unsigned char *o = pred_u8 + (v * HW + i) * 3;
            o[0] = in ? to8b(p0) : 0;
            o[1] = in ? to8b(p1) : 0;
            o[2] = in ? to8b(p2) : 0;
        }
        if (gt_u8) {
            unsigned char *o = gt_u8 + (v * HW + i) * 3;
            o[0] = to8b(g0);
            o[1] = to8b(g1);
            o[2] = to8b(g2);
        }
    }
    PixPartial out;
    out.sse = block_sum(sse, shd);
    out.count = block_sum(count, shi);
    out.x0 = block_reduce(x0, shi, Min());
    out.x1 = block_reduce(x1, shi, Max());
    out.y0 = block_reduce(y0, shi, Min());
    out.y1 = block_reduce(y1, shi, Max());
    out.pad = 0;
    if (threadIdx.x == 0) partial[v * gridDim.x + blockIdx.x] = out;
}

// one workgroup per view: thread t takes partials t, t + 256, ... in order, then the fixed tree (strided_sum for the squared error)
__global__ __launch_bounds__(kThreads) void k_metrics_box(const PixPartial *__restrict__ partial, int chunks,
                                                          hl_metrics_record *__restrict__ rec) {
    __shared__ double shd[kThreads];
    __shared__ int shi[kThreads];
    const int64_t v = blockIdx.x;
    const double sse = strided_sum(&partial[v * chunks].sse, chunks, sizeof(PixPartial) / sizeof(double), shd);
    int count = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    for (int i = (int)threadIdx.x; i < chunks; i += kThreads) {      // (integers: any order gives the same result)
        const PixPartial q = partial[v * chunks + i];
        count += q.count;
        x0 = q.x0 < x0 ? q.x0 : x0;
        x1 = q.x1 > x1 ? q.x1 : x1;
        y0 = q.y0 < y0 ? q.y0 : y0;
        y1 = q.y1 > y1 ? q.y1 : y1;
    }
    count = block_sum(count, shi);
    x0 = block_reduce(x0, shi, Min());
    x1 = block_reduce(x1, shi, Max());
    y0 = block_reduce(y0, shi, Min());
    y1 = block_reduce(y1, shi, Max());
    if (threadIdx.x == 0) {
        hl_metrics_record r;
        r.mse = sse / (3.0 * (double)count);                  // (an empty mask: 0 / 0 = NaN, like np.mean of nothing)
        r.psnr = -10.0 * log(r.mse) / log(10.0);              // psnr_metric's expression
        r.ssim = NAN;                                         // (k_metrics_ssim_finish overwrites it)
        r.count = count;
        r.x = count ? x0 : 0;                                 // cv2.boundingRect of an empty mask is (0, 0, 0, 0)
        r.y = count ? y0 : 0;
        r.w = count ? x1 - x0 + 1 : 0;
        r.h = count ? y1 - y0 + 1 : 0;
        r.reserved = 0;
        rec[v] = r;
    }
}

__global__ __launch_bounds__(kThreads) void k_metrics_ssim(const float *__restrict__ pred, const float *__restrict__ gt,
                                                           const unsigned char *__restrict__ mask, int H, int W, double c1, double c2,
                                                           const hl_metrics_record *__restrict__ rec, double *__restrict__ partial) {
    __shared__ float sx[3][kHalo][kHalo], sy[3][kHalo][kHalo];     // masked prediction / ground truth, fp32 as given
    __shared__ double row[5][kHalo][kTile];                        // 7-sums along x of x, y, xx, yy, xy
    __shared__ double shd[kThreads];
    const int64_t v = blockIdx.z;
    const int tid = (int)threadIdx.x;
    const int bx = rec[v].x, by = rec[v].y, bw = rec[v].w, bh = rec[v].h;
    const int iw = bw - (kWin - 1), ih = bh - (kWin - 1);          // window origins of the crop's interior
    const int ox = (int)blockIdx.x * kTile, oy = (int)blockIdx.y * kTile;
    double *out = partial + 3 * ((v * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
    if (iw <= 0 || ih <= 0 || ox >= iw || oy >= ih) {              // (uniform over the workgroup)
        if (tid < 3) out[tid] = 0.0;
        return;
    }
    const int HW = H * W;
    for (int i = tid; i < kHalo * kHalo; i += kThreads) {
        const int ly = i / kHalo, lx = i - ly * kHalo;
        const int y = by + oy + ly, x = bx + ox + lx;
        // beyond the crop: only windows outside the interior read it, and those are not counted
        const bool in = y < by + bh && x < bx + bw && y < H && x < W && mask[v * HW + y * W + x] != 0;
        const int64_t o = (v * HW + (in ? y * W + x : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sx[c][ly][lx] = in ? pred[o + c] : 0.f;
            sy[c][ly][lx] = in ? gt[o + c] : 0.f;
        }
    }
    __syncthreads();
    const int ty = tid / kTile, tx = tid - ty * kTile;
    const bool counted = ox + tx < iw && oy + ty < ih;
    const double cov_norm = 49.0 / 48.0;                           // use_sample_covariance=True: NP / (NP - 1)
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < kHalo * kTile; i += kThreads) {
            const int ly = i / kTile, j = i - ly * kTile;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const double xv = (double)sx[c][ly][j + k], yv = (double)sy[c][ly][j + k];
                a += xv;
                b += yv;
                aa += xv * xv;
                bb += yv * yv;
                ab += xv * yv;
            }
            row[0][ly][j] = a;
            row[1][ly][j] = b;
            row[2][ly][j] = aa;
            row[3][ly][j] = bb;
            row[4][ly][j] = ab;
        }
        __syncthreads();
        double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            a += row[0][ty + k][tx];
            b += row[1][ty + k][tx];
            aa += row[2][ty + k][tx];
            bb += row[3][ty + k][tx];
            ab += row[4][ty + k][tx];
        }
        // skimage.metrics.structural_similarity, in its order
        const double ux = a / 49.0, uy = b / 49.0, uxx = aa / 49.0, uyy = bb / 49.0, uxy = ab / 49.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + c1, A2 = 2.0 * vxy + c2, B1 = ux * ux + uy * uy + c1, B2 = vx + vy + c2;
        const double D = B1 * B2;
        const double S = (A1 * A2) / D;
        const double tot = block_sum(counted ? S : 0.0, shd);      // (its barriers also free `row` for the next channel)
        if (tid == 0) out[c] = tot;
    }
}

__global__ __launch_bounds__(kThreads) void k_metrics_ssim_finish(const double *__restrict__ partial, int tiles,
                                                                  hl_metrics_record *__restrict__ rec) {
    __shared__ double shd[kThreads];
    const int64_t v = blockIdx.x;
    const int iw = rec[v].w - (kWin - 1), ih = rec[v].h - (kWin - 1);
    double ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ch[c] = strided_sum(partial + 3 * v * tiles + c, tiles, 3, shd) / ((double)iw * (double)ih);
    // a crop smaller than the window has no interior: skimage raises, the record says NaN
    if (threadIdx.x == 0) rec[v].ssim = iw > 0 && ih > 0 ? (ch[0] + ch[1] + ch[2]) / 3.0 : NAN;
}

struct Plan {
    int chunks, tx, ty;
    size_t pix_bytes, ssim_bytes;
};

inline bool plan(int V, int H, int W, Plan &p) {
    if (V <= 0 || V > 65535 || H <= 0 || W <= 0 || (int64_t)H * W * 3 > (int64_t)0x7fffffff - 3 * kPixChunk) return false;
    p.chunks = (int)(((int64_t)H * W + kPixChunk - 1) / kPixChunk);
    p.tx = W >= kWin ? (W - kWin + kTile) / kTile : 1;            // ceil((W - 6) / 16), at least one tile so every partial exists
    p.ty = H >= kWin ? (H - kWin + kTile) / kTile : 1;
    if (p.ty > 65535) return false;
    p.pix_bytes = (size_t)V * p.chunks * sizeof(PixPartial);
    p.ssim_bytes = (size_t)V * p.tx * p.ty * 3 * sizeof(double);
    return true;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

size_t hl_image_metrics_workspace_bytes(int V, int H, int W) {
    Plan p;
    return plan(V, H, W, p) ? p.pix_bytes + p.ssim_bytes : 0;
}

int hl_image_metrics(const float *pred, const float *gt, const unsigned char *mask, int V, int H, int W, double data_range, unsigned flags,
                     unsigned char *pred_u8, unsigned char *gt_u8, hl_metrics_record *results, void *workspace, size_t workspace_bytes,
                     void *stream) {
    Plan p;
    HL_REQUIRE(pred && gt && mask && results, "hl_image_metrics: NULL argument");
    HL_REQUIRE(plan(V, H, W, p), "hl_image_metrics: bad shape (%d views of %d x %d; 1..65535 views, 3 H W < 2^31)", V, H, W);
    HL_REQUIRE(flags == 0, "hl_image_metrics: flags must be 0 (got %u)", flags);
    HL_REQUIRE(data_range > 0.0, "hl_image_metrics: data_range must be positive (got %g)", data_range);
    HL_REQUIRE(workspace && workspace_bytes >= p.pix_bytes + p.ssim_bytes, "hl_image_metrics: workspace too small (%zu bytes, need %zu)",
               workspace_bytes, p.pix_bytes + p.ssim_bytes);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    PixPartial *pix = static_cast<PixPartial *>(workspace);
    double *tiles = reinterpret_cast<double *>(static_cast<char *>(workspace) + p.pix_bytes);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(kThreads);
    hipLaunchKernelGGL(k_metrics_pixels, dim3(p.chunks, V), block, 0, st, pred, gt, mask, H, W, pred_u8, gt_u8, pix);
    int rc = check_launch("k_metrics_pixels");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_metrics_box, dim3(V), block, 0, st, pix, p.chunks, results);
    rc = check_launch("k_metrics_box");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_metrics_ssim, dim3(p.tx, p.ty, V), block, 0, st, pred, gt, mask, H, W, c1, c2, results, tiles);
    rc = check_launch("k_metrics_ssim");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_metrics_ssim_finish, dim3(V), block, 0, st, tiles, p.tx * p.ty, results);
    return check_launch("k_metrics_ssim_finish");
}

}  // extern "C"
