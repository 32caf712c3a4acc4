// Raw dataset views -> the float image and body mask a ViewStore holds, MI355X (gfx950): the image half of SynBodyDatasetBatch.__getitem__
// (recon_NeRF/lib/SynBody_dataset.py:266-278 of the reference) without cv2.  Contract: DESIGN.md 4i.
//
// Host (no device work): hl_area_taps / hl_nearest_taps build one axis of the resize rule in float64, hl_view_ingest_table packs them
//   into the int32 words the kernel reads: count[dst] | nearest[dst] | idx[dst][T] | weight bits[dst][T], T = hl_area_max_taps(src, dst).
//
// k_view_ingest: grid (ceil(W / 256), H, V), one workgroup per 256 output pixels of one output row; lane i owns output column x0 + i, so the
//   source windows of a wave are one contiguous run of every source row.  That run - image bytes and mask bytes - is staged in LDS with
//   16-byte loads from the 16-byte boundary below it (the chunk that would cross the end of the array is read bytewise), as many source
//   rows per pass as fit 32 KiB.  Each lane then sums its window: per source row s = sum_k alpha_k * value in table order, where
//   value = mask ? (float)u8 / 255.0f : 0.0f (the mask applied at source resolution, :268), and acc += beta * s over the rows in table
//   order.  The body byte is the nearest source mask pixel.  Every index read from a table is clamped into the source before use: a wrong
//   table gives wrong pixels, never an access outside the arrays.
// k_view_convert: H == Hs and W == Ws, a flat pass, four pixels per thread (three dword loads, three 16-byte stores).
// k_layers_ingest / k_layers_convert: the same two passes for the layered views of TightCap (TightCap_dataset.py:233-298, contract: DESIGN.md
//   4j): the source pixel is composed from the photograph and up to five mask planes per view - zero, the byte / 255 or a fixed skin colour -
//   while it is staged (a code byte in LDS where k_view_ingest keeps the mask byte) or in registers; no composed image goes through HBM.
// Plain vector stores, no atomics, nothing depends on V: a view's bits are the same alone or in a batch.  -ffp-contract=off (build.py).
#include "hl_common.h"

#include <cmath>
#include <cstdint>

namespace hl {
namespace {

constexpr int kTile = 256;                   // output pixels (threads) per workgroup
constexpr int kStageBytes = 32 * 1024;       // LDS a pass stages
constexpr int kMaxLds = 64 * 1024;

struct IngestArgs {
    const unsigned char *img, *msk;
    const int *xtab, *ytab;
    float *out;
    unsigned char *body;
    long long img_bytes, msk_bytes;
    int Hs, Ws, H, W, Tx, Ty, cap, istride, mstride, rows_per_pass;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// 16 bytes of `p` at byte offset `off` (a multiple of 16, p 16-byte aligned); bytes at or beyond `total` read as zero
__device__ __forceinline__ uint4 load16(const unsigned char *p, long long off, long long total) {
    if (off + 16 <= total) return *reinterpret_cast<const uint4 *>(p + off);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (off + b < total) w[b >> 2] |= (unsigned)p[off + b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kTile) void k_view_ingest(const IngestArgs a) {
    extern __shared__ uint4 lds4[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds4);
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kTile, dy = (int)blockIdx.y;
    const long long v = blockIdx.z;
    const int dx = x0 + tid, xl = (x0 + kTile < a.W ? x0 + kTile : a.W) - 1;
    const bool live = dx < a.W;
    const int Tx = a.Tx, Ty = a.Ty, Hs = a.Hs, Ws = a.Ws;
    const int *xi = a.xtab + 2 * a.W, *xw = xi + (long long)a.W * Tx;
    const int *yi = a.ytab + 2 * a.H + (long long)dy * Ty, *yw = yi + (long long)a.H * Ty;
    // the tile's run of source columns [c0, c0 + span): first tap of its first column .. last tap of its last
    const int c0 = clampi(xi[(long long)x0 * Tx], 0, Ws - 1);
    const int nl = clampi(a.xtab[xl], 0, Tx);
    const int c1 = (nl ? clampi(xi[(long long)xl * Tx + nl - 1], 0, Ws - 1) : c0) + 1;
    const int span = clampi(c1 - c0, 0, a.cap);
    const int ny = clampi(a.ytab[dy], 0, Ty);
    const int nx = live ? clampi(a.xtab[dx], 0, Tx) : 0;
    const int ich = a.istride >> 4, mch = a.mstride >> 4, rowbytes = a.istride + a.mstride;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int j0 = 0; j0 < ny; j0 += a.rows_per_pass) {
        const int nr = ny - j0 < a.rows_per_pass ? ny - j0 : a.rows_per_pass;
        __syncthreads();                                              // (the previous pass has been read)
        for (int it = tid; it < nr * (ich + mch); it += kTile) {
            const int jr = it / (ich + mch), i = it - jr * (ich + mch);
            const long long row = v * Hs + clampi(yi[j0 + jr], 0, Hs - 1);
            const long long m0 = row * Ws + c0;                       // first mask byte of the run; the image's is 3 m0
            uint4 *dst = reinterpret_cast<uint4 *>(lds + (long long)jr * rowbytes);
            if (i < ich) {
                const long long a0 = 3 * m0, al = a0 & ~15LL;
                if (i < (int)((a0 - al + 3LL * span + 15) >> 4)) dst[i] = load16(a.img, al + 16LL * i, a.img_bytes);
            } else {
                const long long al = m0 & ~15LL;
                const int k = i - ich;
                if (k < (int)((m0 - al + span + 15) >> 4)) dst[ich + k] = load16(a.msk, al + 16LL * k, a.msk_bytes);
            }
        }
        __syncthreads();
        for (int jr = 0; jr < nr; ++jr) {
            const long long m0 = (v * Hs + clampi(yi[j0 + jr], 0, Hs - 1)) * Ws + c0;
            const unsigned char *li = lds + (long long)jr * rowbytes + (int)((3 * m0) & 15);
            const unsigned char *lm = lds + (long long)jr * rowbytes + a.istride + (int)(m0 & 15);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int k = 0; k < nx; ++k) {
                const int off = clampi(xi[(long long)dx * Tx + k], 0, Ws - 1) - c0;
                if ((unsigned)off < (unsigned)span) {
                    const float al = __int_as_float(xw[(long long)dx * Tx + k]);
                    const bool on = lm[off] != 0;                     // img[msk == 0] = 0 at source resolution (:268)
                    const float p0 = on ? (float)li[3 * off] / 255.0f : 0.f;
                    const float p1 = on ? (float)li[3 * off + 1] / 255.0f : 0.f;
                    const float p2 = on ? (float)li[3 * off + 2] / 255.0f : 0.f;
                    s0 += al * p0;
                    s1 += al * p1;
                    s2 += al * p2;
                }
            }
            const float be = __int_as_float(yw[j0 + jr]);
            acc0 += be * s0;
            acc1 += be * s1;
            acc2 += be * s2;
        }
    }
    if (live) {
        const long long pix = (v * a.H + dy) * a.W + dx;
        a.out[pix * 3] = acc0;
        a.out[pix * 3 + 1] = acc1;
        a.out[pix * 3 + 2] = acc2;
        const int sy = clampi(a.ytab[a.H + dy], 0, Hs - 1), sx = clampi(a.xtab[a.W + dx], 0, Ws - 1);
        a.body[pix] = a.msk[(v * Hs + sy) * Ws + sx] != 0 ? 1 : 0;
    }
}

__device__ __forceinline__ float4 unit4(unsigned char b0, unsigned char b1, unsigned char b2, unsigned char b3) {
    return make_float4((float)b0 / 255.0f, (float)b1 / 255.0f, (float)b2 / 255.0f, (float)b3 / 255.0f);
}

// n pixels; img, msk, out, body 16-byte aligned, so a thread's four pixels are three aligned dwords of image and one of mask
__global__ __launch_bounds__(256) void k_view_convert(const unsigned char *__restrict__ img, const unsigned char *__restrict__ msk, long long n,
                                                      float *__restrict__ out, unsigned char *__restrict__ body) {
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p + 4 <= n) {
        const unsigned *src = reinterpret_cast<const unsigned *>(img + p * 3);
        unsigned w0 = src[0], w1 = src[1], w2 = src[2];
        const unsigned m = *reinterpret_cast<const unsigned *>(msk + p);
        const bool on0 = (m & 0xffu) != 0, on1 = (m & 0xff00u) != 0, on2 = (m & 0xff0000u) != 0, on3 = (m & 0xff000000u) != 0;
        // bytes 0..11 are pixels 0 0 0 1 | 1 1 2 2 | 2 3 3 3
        w0 &= (on0 ? 0x00ffffffu : 0u) | (on1 ? 0xff000000u : 0u);
        w1 &= (on1 ? 0x0000ffffu : 0u) | (on2 ? 0xffff0000u : 0u);
        w2 &= (on2 ? 0x000000ffu : 0u) | (on3 ? 0xffffff00u : 0u);
        float4 *dst = reinterpret_cast<float4 *>(out + p * 3);
        dst[0] = unit4(w0 & 0xff, (w0 >> 8) & 0xff, (w0 >> 16) & 0xff, w0 >> 24);
        dst[1] = unit4(w1 & 0xff, (w1 >> 8) & 0xff, (w1 >> 16) & 0xff, w1 >> 24);
        dst[2] = unit4(w2 & 0xff, (w2 >> 8) & 0xff, (w2 >> 16) & 0xff, w2 >> 24);
        *reinterpret_cast<unsigned *>(body + p) = (on0 ? 1u : 0u) | (on1 ? 0x100u : 0u) | (on2 ? 0x10000u : 0u) | (on3 ? 0x1000000u : 0u);
    } else {
        for (long long q = p; q < n; ++q) {
            const bool on = msk[q] != 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[q * 3 + ch] = on ? (float)img[q * 3 + ch] / 255.0f : 0.f;
            body[q] = on ? 1 : 0;
        }
    }
}

// ---- layered views: the photograph and five binary masks of a TightCap view -> the image of cloth layer L ----
// One code per source pixel; the first matching row decides (s = person + the garments layer L wears):
//   full == 0 -> zero | L == 3 -> keep, mask on | s >= 2 -> skin | person == 0 and s == 1 -> zero | otherwise keep (mask on where a byte is non-zero)
constexpr unsigned kZero = 0, kKeep = 1, kKeepOn = 2, kSkin = 3;

struct LayerPlanes {
    const unsigned char *img, *full, *person, *top, *bottom, *shoes;
    const int *layers;
};

struct LayerArgs {
    LayerPlanes pl;
    const int *xtab, *ytab;
    float *out;
    unsigned char *body;
    long long msk_bytes;                     // V Hs Ws; the image has three times as many
    int Hs, Ws, H, W, Tx, Ty, cap, istride, mstride, rows_per_pass;
};

__device__ __forceinline__ float skin(int ch) { return ch == 0 ? 0.607186f : ch == 1 ? 0.49289057f : 0.43795943f; }

// the planes layer L reads besides `full`; a plane the caller left NULL reads as zero
struct LayerReads {
    bool person, top, bottom, shoes;
    unsigned keep;
};

__device__ __forceinline__ LayerReads layer_reads(const LayerPlanes &pl, int L) {
    LayerReads r;
    r.person = L < 3 && pl.person;
    r.top = L < 2 && pl.top;
    r.bottom = L < 1 && pl.bottom;
    r.shoes = L < 3 && pl.shoes;
    r.keep = L < 3 ? kKeep : kKeepOn;
    return r;
}

// per byte of w: 1 where it is non-zero
__device__ __forceinline__ unsigned nz01(unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

// the codes of four pixels from their 0 / 1 bytes of full (f) and person (p) and their garment counts g (0 .. 3 per byte)
__device__ __forceinline__ unsigned codes4(unsigned f, unsigned p, unsigned g, unsigned keep) {
    const unsigned ge2 = ((p + g + 0x7e7e7e7eu) >> 7) & 0x01010101u;                 // s >= 2
    const unsigned lone = g & ~p & ~ge2 & 0x01010101u;                               // one garment and no body under it
    return (f & ge2) * kSkin + (f & ~ge2 & ~lone) * keep;
}

__device__ __forceinline__ unsigned pixel_code(const LayerPlanes &pl, const LayerReads &r, long long q) {
    if (pl.full[q] == 0) return kZero;
    const unsigned p = r.person && pl.person[q] != 0 ? 1u : 0u;
    const unsigned g = (r.top && pl.top[q] != 0 ? 1u : 0u) + (r.bottom && pl.bottom[q] != 0 ? 1u : 0u) + (r.shoes && pl.shoes[q] != 0 ? 1u : 0u);
    if (p + g >= 2) return kSkin;
    if (p == 0 && g == 1) return kZero;
    return r.keep;
}

// the body bit of a composed pixel: any channel non-zero (img.sum(-1) != 0 of non-negative values)
__device__ __forceinline__ unsigned code_body(unsigned code, unsigned b0, unsigned b1, unsigned b2) {
    return code == kKeep ? ((b0 | b1 | b2) != 0 ? 1u : 0u) : code != kZero ? 1u : 0u;
}

__device__ __forceinline__ float code_value(unsigned code, unsigned char b, int ch) {
    return code == kSkin ? skin(ch) : code != kZero ? (float)b / 255.0f : 0.f;
}

// k_view_ingest with the composition fused: where that kernel stages the mask byte this one stages the pixel's code, combined bytewise in
// registers from the 16-byte chunks of up to five planes (every plane is (V, Hs, Ws), so one offset and one alignment serve them all)
__global__ __launch_bounds__(kTile) void k_layers_ingest(const LayerArgs a) {
    extern __shared__ uint4 lds4[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds4);
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kTile, dy = (int)blockIdx.y;
    const long long v = blockIdx.z;
    const int dx = x0 + tid, xl = (x0 + kTile < a.W ? x0 + kTile : a.W) - 1;
    const bool live = dx < a.W;
    const int Tx = a.Tx, Ty = a.Ty, Hs = a.Hs, Ws = a.Ws;
    const LayerReads rd = layer_reads(a.pl, clampi(a.pl.layers[v], 0, 3));
    const int *xi = a.xtab + 2 * a.W, *xw = xi + (long long)a.W * Tx;
    const int *yi = a.ytab + 2 * a.H + (long long)dy * Ty, *yw = yi + (long long)a.H * Ty;
    const int c0 = clampi(xi[(long long)x0 * Tx], 0, Ws - 1);
    const int nl = clampi(a.xtab[xl], 0, Tx);
    const int c1 = (nl ? clampi(xi[(long long)xl * Tx + nl - 1], 0, Ws - 1) : c0) + 1;
    const int span = clampi(c1 - c0, 0, a.cap);
    const int ny = clampi(a.ytab[dy], 0, Ty);
    const int nx = live ? clampi(a.xtab[dx], 0, Tx) : 0;
    const int ich = a.istride >> 4, mch = a.mstride >> 4, rowbytes = a.istride + a.mstride;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int j0 = 0; j0 < ny; j0 += a.rows_per_pass) {
        const int nr = ny - j0 < a.rows_per_pass ? ny - j0 : a.rows_per_pass;
        __syncthreads();                                              // (the previous pass has been read)
        for (int it = tid; it < nr * (ich + mch); it += kTile) {
            const int jr = it / (ich + mch), i = it - jr * (ich + mch);
            const long long row = v * Hs + clampi(yi[j0 + jr], 0, Hs - 1);
            const long long m0 = row * Ws + c0;                       // first mask byte of the run; the image's is 3 m0
            uint4 *dst = reinterpret_cast<uint4 *>(lds + (long long)jr * rowbytes);
            if (i < ich) {
                const long long a0 = 3 * m0, al = a0 & ~15LL;
                if (i < (int)((a0 - al + 3LL * span + 15) >> 4)) dst[i] = load16(a.pl.img, al + 16LL * i, 3 * a.msk_bytes);
            } else {
                const long long al = m0 & ~15LL;
                const int k = i - ich;
                if (k < (int)((m0 - al + span + 15) >> 4)) {
                    const long long off = al + 16LL * k;
                    if (off + 16 <= a.msk_bytes) {
                        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                        const uint4 f = *reinterpret_cast<const uint4 *>(a.pl.full + off);
                        const uint4 p = rd.person ? *reinterpret_cast<const uint4 *>(a.pl.person + off) : z;
                        const uint4 t = rd.top ? *reinterpret_cast<const uint4 *>(a.pl.top + off) : z;
                        const uint4 b = rd.bottom ? *reinterpret_cast<const uint4 *>(a.pl.bottom + off) : z;
                        const uint4 s = rd.shoes ? *reinterpret_cast<const uint4 *>(a.pl.shoes + off) : z;
                        dst[ich + k] = make_uint4(codes4(nz01(f.x), nz01(p.x), nz01(t.x) + nz01(b.x) + nz01(s.x), rd.keep),
                                                  codes4(nz01(f.y), nz01(p.y), nz01(t.y) + nz01(b.y) + nz01(s.y), rd.keep),
                                                  codes4(nz01(f.z), nz01(p.z), nz01(t.z) + nz01(b.z) + nz01(s.z), rd.keep),
                                                  codes4(nz01(f.w), nz01(p.w), nz01(t.w) + nz01(b.w) + nz01(s.w), rd.keep));
                    } else {                                          // the chunk that would cross the end of the planes: bytewise
                        unsigned char *cb = reinterpret_cast<unsigned char *>(dst + ich + k);
                        for (int b = 0; b < 16; ++b) cb[b] = off + b < a.msk_bytes ? (unsigned char)pixel_code(a.pl, rd, off + b) : (unsigned char)kZero;
                    }
                }
            }
        }
        __syncthreads();
        for (int jr = 0; jr < nr; ++jr) {
            const long long m0 = (v * Hs + clampi(yi[j0 + jr], 0, Hs - 1)) * Ws + c0;
            const unsigned char *li = lds + (long long)jr * rowbytes + (int)((3 * m0) & 15);
            const unsigned char *lm = lds + (long long)jr * rowbytes + a.istride + (int)(m0 & 15);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int k = 0; k < nx; ++k) {
                const int off = clampi(xi[(long long)dx * Tx + k], 0, Ws - 1) - c0;
                if ((unsigned)off < (unsigned)span) {
                    const float al = __int_as_float(xw[(long long)dx * Tx + k]);
                    const unsigned code = lm[off];
                    const float p0 = code_value(code, li[3 * off], 0);
                    const float p1 = code_value(code, li[3 * off + 1], 1);
                    const float p2 = code_value(code, li[3 * off + 2], 2);
                    s0 += al * p0;
                    s1 += al * p1;
                    s2 += al * p2;
                }
            }
            const float be = __int_as_float(yw[j0 + jr]);
            acc0 += be * s0;
            acc1 += be * s1;
            acc2 += be * s2;
        }
    }
    if (live) {
        const long long pix = (v * a.H + dy) * a.W + dx;
        a.out[pix * 3] = acc0;
        a.out[pix * 3 + 1] = acc1;
        a.out[pix * 3 + 2] = acc2;
        const int sy = clampi(a.ytab[a.H + dy], 0, Hs - 1), sx = clampi(a.xtab[a.W + dx], 0, Ws - 1);
        const long long q = (v * Hs + sy) * Ws + sx;                  // the one nearest source pixel, composed from global memory
        a.body[pix] = (unsigned char)code_body(pixel_code(a.pl, rd, q), a.pl.img[3 * q], a.pl.img[3 * q + 1], a.pl.img[3 * q + 2]);
    }
}

// n = V hw pixels, every array 16-byte aligned: k_view_convert with the composition.  A thread's four pixels are three aligned dwords of
// image and one of each plane its layer reads; the four that straddle two views (hw % 4 != 0) and the array's tail go bytewise.
__global__ __launch_bounds__(256) void k_layers_convert(const LayerPlanes pl, long long n, long long hw, int V, float *__restrict__ out,
                                                        unsigned char *__restrict__ body) {
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n) return;
    const long long v0 = p / hw;
    if (p + 4 <= n && p + 3 - v0 * hw < hw) {
        const LayerReads rd = layer_reads(pl, clampi(pl.layers[v0], 0, 3));
        const unsigned *src = reinterpret_cast<const unsigned *>(pl.img + p * 3);
        const unsigned w[3] = {src[0], src[1], src[2]};
        const unsigned f = nz01(*reinterpret_cast<const unsigned *>(pl.full + p));
        const unsigned pe = rd.person ? nz01(*reinterpret_cast<const unsigned *>(pl.person + p)) : 0u;
        const unsigned g = (rd.top ? nz01(*reinterpret_cast<const unsigned *>(pl.top + p)) : 0u) +
                           (rd.bottom ? nz01(*reinterpret_cast<const unsigned *>(pl.bottom + p)) : 0u) +
                           (rd.shoes ? nz01(*reinterpret_cast<const unsigned *>(pl.shoes + p)) : 0u);
        const unsigned codes = codes4(f, pe, g, rd.keep);
        float o[12];
        unsigned on = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned code = (codes >> (8 * i)) & 0xffu;
            unsigned b[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int j = 3 * i + ch;                             // bytes 0..11 are pixels 0 0 0 1 | 1 1 2 2 | 2 3 3 3
                b[ch] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                o[j] = code_value(code, (unsigned char)b[ch], ch);
            }
            on |= code_body(code, b[0], b[1], b[2]) << (8 * i);
        }
        float4 *dst = reinterpret_cast<float4 *>(out + p * 3);
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        dst[1] = make_float4(o[4], o[5], o[6], o[7]);
        dst[2] = make_float4(o[8], o[9], o[10], o[11]);
        *reinterpret_cast<unsigned *>(body + p) = on;
    } else {
        for (long long q = p; q < p + 4 && q < n; ++q) {
            const long long vq = q / hw;
            const LayerReads rd = layer_reads(pl, clampi(pl.layers[vq < V ? vq : V - 1], 0, 3));
            const unsigned code = pixel_code(pl, rd, q);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[q * 3 + ch] = code_value(code, pl.img[q * 3 + ch], ch);
            body[q] = (unsigned char)code_body(code, pl.img[q * 3], pl.img[q * 3 + 1], pl.img[q * 3 + 2]);
        }
    }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round16(long long v) { return (int)((v + 15) & ~15LL); }

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_area_max_taps(int src, int dst) {
    if (src <= 0 || dst <= 0 || dst > src) return 0;
    return ceil_div(src, dst) + 1;                                    // ceil(scale) full cells and one partial beside them
}

int hl_area_taps(int src, int dst, int max_taps, int32_t *idx_out, float *w_out, int32_t *count_out) {
    HL_REQUIRE(idx_out && w_out && count_out, "hl_area_taps: NULL argument");
    HL_REQUIRE(src > 0 && dst > 0 && dst <= src, "hl_area_taps: %d -> %d is not a reduction (the area rule covers dst <= src only)", src, dst);
    HL_REQUIRE(max_taps > 0, "hl_area_taps: max_taps %d", max_taps);
    const double scale = (double)src / (double)dst;
    for (int dx = 0; dx < dst; ++dx) {
        int32_t *idx = idx_out + (long long)dx * max_taps;
        float *w = w_out + (long long)dx * max_taps;
        for (int k = 0; k < max_taps; ++k) {
            idx[k] = 0;
            w[k] = 0.f;
        }
        const double f1 = dx * scale, f2 = f1 + scale;
        const double cell = std::fmin(scale, (double)src - f1);
        int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
        s2 = s2 < src - 1 ? s2 : src - 1;
        s1 = s1 < s2 ? s1 : s2;
        int n = 0;
        auto put = [&](int s, double weight) {
            if (n < max_taps) {
                idx[n] = s;
                w[n] = (float)weight;
            }
            ++n;
        };
        if (s1 - f1 > 1e-3) put(s1 - 1, (s1 - f1) / cell);
        for (int s = s1; s < s2; ++s) put(s, 1.0 / cell);
        if (f2 - s2 > 1e-3) put(s2, std::fmin(std::fmin(f2 - s2, 1.0), cell) / cell);
        HL_REQUIRE(n <= max_taps, "hl_area_taps: column %d of %d -> %d has %d taps, max_taps is %d", dx, src, dst, n, max_taps);
        for (int k = 0; k < n; ++k) HL_REQUIRE(idx[k] >= 0 && idx[k] < src, "hl_area_taps: tap %d of column %d is outside the source", idx[k], dx);
        count_out[dx] = n;
    }
    return HL_OK;
}

int hl_nearest_taps(int src, int dst, int32_t *idx_out) {
    HL_REQUIRE(idx_out, "hl_nearest_taps: NULL argument");
    HL_REQUIRE(src > 0 && dst > 0, "hl_nearest_taps: bad sizes %d -> %d", src, dst);
    const double scale = (double)src / (double)dst;
    for (int dx = 0; dx < dst; ++dx) {
        const int s = (int)std::floor(dx * scale);
        idx_out[dx] = s < src - 1 ? s : src - 1;
    }
    return HL_OK;
}

size_t hl_view_ingest_table_words(int src, int dst) {
    const int T = hl_area_max_taps(src, dst);
    return T ? (size_t)dst * (2 + 2 * (size_t)T) : 0;
}

int hl_view_ingest_table(int src, int dst, int32_t *h_table) {
    HL_REQUIRE(h_table, "hl_view_ingest_table: NULL argument");
    const int T = hl_area_max_taps(src, dst);
    HL_REQUIRE(T > 0, "hl_view_ingest_table: %d -> %d is not a reduction", src, dst);
    static_assert(sizeof(float) == sizeof(int32_t), "weights are stored as their bits");
    int rc = hl_area_taps(src, dst, T, h_table + 2 * (size_t)dst, reinterpret_cast<float *>(h_table + (2 + (size_t)T) * dst), h_table);
    if (rc != HL_OK) return rc;
    return hl_nearest_taps(src, dst, h_table + dst);
}

int hl_view_ingest(const unsigned char *img_u8, const unsigned char *msk_u8, int V, int Hs, int Ws, int H, int W, const int32_t *xtab,
                   const int32_t *ytab, float *out_image, unsigned char *out_body, void *stream) {
    HL_REQUIRE(img_u8 && msk_u8 && out_image && out_body, "hl_view_ingest: NULL argument");
    HL_REQUIRE(V > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "hl_view_ingest: bad shape (%d views of %d x %d -> %d x %d)", V, Hs, Ws, H, W);
    HL_REQUIRE(H <= Hs && W <= Ws, "hl_view_ingest: %d x %d -> %d x %d enlarges an axis (the area rule covers reductions only)", Hs, Ws, H, W);
    HL_REQUIRE((long long)V * Hs * Ws <= 0x7fffffffffffLL / 3 && (long long)Hs * Ws <= 0x7fffffffLL, "hl_view_ingest: views too large");
    HL_REQUIRE(aligned16({img_u8, msk_u8, out_image, out_body}), "hl_view_ingest: img_u8, msk_u8, out_image and out_body must be 16-byte aligned");
    if (H == Hs && W == Ws) {
        const long long n = (long long)V * H * W, blocks = (n + 1023) / 1024;
        HL_REQUIRE(blocks <= 0x7fffffffLL, "hl_view_ingest: too many pixels for one launch");
        hipLaunchKernelGGL(k_view_convert, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img_u8, msk_u8, n, out_image, out_body);
        return check_launch("k_view_convert");
    }
    HL_REQUIRE(xtab && ytab, "hl_view_ingest: NULL tap table");
    HL_REQUIRE(H <= 65535 && V <= 65535, "hl_view_ingest: at most 65535 output rows and 65535 views per call (got %d, %d)", H, V);
    IngestArgs a{};
    a.img = img_u8; a.msk = msk_u8; a.xtab = xtab; a.ytab = ytab; a.out = out_image; a.body = out_body;
    a.img_bytes = 3LL * V * Hs * Ws; a.msk_bytes = (long long)V * Hs * Ws;
    a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.Tx = hl_area_max_taps(Ws, W); a.Ty = hl_area_max_taps(Hs, H);
    const long long cap = (long long)std::ceil(kTile * ((double)Ws / (double)W)) + 2;      // source columns under kTile output columns
    a.cap = (int)(cap < Ws ? cap : Ws);
    a.istride = round16(3LL * a.cap + 15);
    a.mstride = round16((long long)a.cap + 15);
    HL_REQUIRE(a.istride + a.mstride <= kMaxLds, "hl_view_ingest: a reduction of %d -> %d columns needs %d bytes of LDS per source row (limit %d)",
               Ws, W, a.istride + a.mstride, kMaxLds);
    a.rows_per_pass = kStageBytes / (a.istride + a.mstride);
    a.rows_per_pass = a.rows_per_pass < 1 ? 1 : a.rows_per_pass > a.Ty ? a.Ty : a.rows_per_pass;
    const size_t lds = (size_t)a.rows_per_pass * (a.istride + a.mstride);
    hipLaunchKernelGGL(k_view_ingest, dim3((unsigned)ceil_div(W, kTile), (unsigned)H, (unsigned)V), dim3(kTile), lds, (hipStream_t)stream, a);
    return check_launch("k_view_ingest");
}

int hl_view_ingest_layers(const unsigned char *img_u8, const unsigned char *full, const unsigned char *person, const unsigned char *top,
                          const unsigned char *bottom, const unsigned char *shoes, const int32_t *layers, int V, int Hs, int Ws, int H, int W,
                          const int32_t *xtab, const int32_t *ytab, float *out_image, unsigned char *out_body, void *stream) {
    HL_REQUIRE(img_u8 && full && layers && out_image && out_body, "hl_view_ingest_layers: NULL argument");
    HL_REQUIRE(V > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "hl_view_ingest_layers: bad shape (%d views of %d x %d -> %d x %d)", V, Hs, Ws, H, W);
    HL_REQUIRE(H <= Hs && W <= Ws, "hl_view_ingest_layers: %d x %d -> %d x %d enlarges an axis (the area rule covers reductions only)", Hs, Ws, H, W);
    HL_REQUIRE((long long)V * Hs * Ws <= 0x7fffffffffffLL / 3 && (long long)Hs * Ws <= 0x7fffffffLL, "hl_view_ingest_layers: views too large");
    HL_REQUIRE(aligned16({img_u8, full, person, top, bottom, shoes, out_image, out_body}),
               "hl_view_ingest_layers: img_u8, the five planes, out_image and out_body must be 16-byte aligned");
    const LayerPlanes pl{img_u8, full, person, top, bottom, shoes, layers};
    if (H == Hs && W == Ws) {
        const long long hw = (long long)H * W, n = V * hw, blocks = (n + 1023) / 1024;
        HL_REQUIRE(blocks <= 0x7fffffffLL, "hl_view_ingest_layers: too many pixels for one launch");
        hipLaunchKernelGGL(k_layers_convert, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pl, n, hw, V, out_image, out_body);
        return check_launch("k_layers_convert");
    }
    HL_REQUIRE(xtab && ytab, "hl_view_ingest_layers: NULL tap table");
    HL_REQUIRE(H <= 65535 && V <= 65535, "hl_view_ingest_layers: at most 65535 output rows and 65535 views per call (got %d, %d)", H, V);
    LayerArgs a{};
    a.pl = pl; a.xtab = xtab; a.ytab = ytab; a.out = out_image; a.body = out_body;
    a.msk_bytes = (long long)V * Hs * Ws;
    a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.Tx = hl_area_max_taps(Ws, W); a.Ty = hl_area_max_taps(Hs, H);
    // the staging area of k_view_ingest: the code byte takes the mask byte's place, so the budget and rows_per_pass are the same
    const long long cap = (long long)std::ceil(kTile * ((double)Ws / (double)W)) + 2;
    a.cap = (int)(cap < Ws ? cap : Ws);
    a.istride = round16(3LL * a.cap + 15);
    a.mstride = round16((long long)a.cap + 15);
    HL_REQUIRE(a.istride + a.mstride <= kMaxLds, "hl_view_ingest_layers: a reduction of %d -> %d columns needs %d bytes of LDS per source row (limit %d)",
               Ws, W, a.istride + a.mstride, kMaxLds);
    a.rows_per_pass = kStageBytes / (a.istride + a.mstride);
    a.rows_per_pass = a.rows_per_pass < 1 ? 1 : a.rows_per_pass > a.Ty ? a.Ty : a.rows_per_pass;
    const size_t lds = (size_t)a.rows_per_pass * (a.istride + a.mstride);
    hipLaunchKernelGGL(k_layers_ingest, dim3((unsigned)ceil_div(W, kTile), (unsigned)H, (unsigned)V), dim3(kTile), lds, (hipStream_t)stream, a);
    return check_launch("k_layers_ingest");
}

}  // extern "C"
