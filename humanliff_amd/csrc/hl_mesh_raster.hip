// Rasterising a triangle mesh, MI355X (gfx950): (vertices per frame, triangles, normals, colours) and pinhole cameras K, R, T ->
// rgb / acc / normal / depth maps in the renderer's layout and pixel convention, plus triangle ids and barycentrics.  Contract:
// DESIGN.md "Rasterising the mesh".  Coverage is exact integer arithmetic on 1/256-pixel coordinates, depth and attributes are fp32
// in a stated order (-ffp-contract=off: a product and the sum it goes into are two roundings), the z-buffer is a 64-bit integer
// atomicMin - order-independent, so an image has the same bits on every run, alone or inside a batch, for any order of the triangles
// (ids apart, where two triangles have the very same depth bits).  No float atomics, nothing scalar.
//
// k_raster_cameras: up to 8 camera rows per launch, passed by value, are written to the scratch (enqueue-only: no host copy).
// k_raster_clear:   z-buffer to all ones, the large list's counter and the status word to 0.
// k_raster_project: a thread per (vertex, image).  float64, camera_ray_pixel's term order run backwards:
//     cam = (R v) + T,  p = K cam,  sx = p.x / p.z,  sy = p.y / p.z,  X = llrint(256 sx),  Y = llrint(256 sy)
//   -> one 16-byte record {int32 X, int32 Y, float z = (float)cam.z, uint32 flags}.  Pixel CENTRES are the integer coordinates, as in
//   get_rays / hl_camera_rays (no half-pixel offset): pixel (px, py) is the point (256 px, 256 py).  flags bit 0 (invalid): a
//   non-finite coordinate, cam.z <= znear, or |sx|, |sy| > 2^19 pixels - inside that band |X|, |Y| <= 2^27, a difference < 2^29, an
//   edge function < 2^59: int64 with room.
// k_raster_cover:   a thread per (triangle, image).  Skipped: an index outside [0, N) (status bit 0 is set; never dereferenced), an
//   invalid vertex, doubled area A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) == 0, a culled sign of A.  A < 0: vertices 1 and 2 change
//   places (so A > 0 below and both windings are drawn); everything after that - edge functions, depth, weights, attribute sums - runs
//   on the swapped order, only `barycentrics` is written back in the triangle's own order.  Edge function i (the weight of vertex i)
//   belongs to the edge from a = i+1 to b = i+2 (mod 3):  E_i = dx (PY - Y_a) - dy (PX - X_a),  (dx, dy) = V_b - V_a; E0 + E1 + E2 = A.
//   A pixel is covered when every E_i > 0, or E_i == 0 and the edge is owned: dy < 0 || (dy == 0 && dx > 0) - true for exactly one
//   of d and -d, so a pixel on a shared edge belongs to exactly one of its two triangles.
//   depth = 1 / ((b0 / z0 + b1 / z1) + b2 / z2),  b_i = (float)E_i / (float)A;  key = bits(depth) << 32 | triangle;  a plain load of
//   the z-buffer word first: the word only ever decreases, so a stored key below ours settles it without the atomic.
//   A triangle whose clamped box holds more than HL_RASTER_SMALL_BOX pixels goes to the large list (one counter add per wave, slots
//   by lane rank); past the list's capacity the thread draws the box itself - slower, never wrong.
// k_raster_cover_large: fixed grid (count read from device memory: no host round trip).  A wave per list entry and SLICE: the box's
//   pixels, in row-major order, go round-robin in runs of 64 to the kLargeSlices slices (grid.y), so a triangle that fills the view is
//   drawn by 16 waves and a wave whose slice starts past the box's end moves on after reading the entry's 16 bytes.
// k_raster_resolve: a thread per pixel: winner's triangle reloaded, exact E_i recomputed, w_i = (b_i / z_i) * depth with depth the
//   key's high word (depth_map is exactly what won), attributes (w0 a0 + w1 a1) + w2 a2.
#include "hl_mesh.h"

#include <cmath>
#include <cstdint>

#define HL_RASTER_SMALL_BOX 64

namespace hl {
namespace {

constexpr int kThreads = kMeshThreads;
constexpr int kWave = 64;
constexpr int kCamsPerLaunch = 8;
constexpr int kMaxImages = 65535;                 // grid.y
constexpr int64_t kLargeCapacity = 1 << 20;       // entries of the large list (16 bytes each), at most
constexpr int kLargeBlocks = 256;                 // x 4 waves x kLargeSlices: 16 waves per CU drain the list
constexpr int kLargeSlices = 16;                  // waves that share one entry's box
constexpr int64_t kGuard = (int64_t)1 << 19;      // pixels
constexpr unsigned long long kEmpty = ~0ull;

struct RasterCam {                                // 36 float64
    double K[9], Ki[9], R[9], T[3], o[3], pad[3];
};
static_assert(sizeof(RasterCam) % 16 == 0, "camera rows keep the scratch 16-byte aligned");

struct CamChunk {
    RasterCam c[kCamsPerLaunch];
};

struct Rec {                                      // a projected vertex
    int X, Y;
    float z;
    unsigned flags;
};
static_assert(sizeof(Rec) == 16, "one dwordx4 per gather");

struct LargeEntry {                               // 16 bytes
    unsigned tri, img, pixels, pad;               // pixels: of the clamped box
};
static_assert(sizeof(LargeEntry) == 16, "one dwordx4 per entry");

struct Layout {                                   // the scratch, in this order; every part a multiple of 16 bytes
    size_t cams, recs, zbuf, counter, list, total;
    int64_t capacity;
};

inline Layout layout_of(int64_t N, int64_t T, int F, int H, int W) {
    Layout l;
    l.capacity = T * F < kLargeCapacity ? T * F : kLargeCapacity;
    l.cams = 0;
    l.recs = l.cams + (size_t)F * sizeof(RasterCam);
    l.zbuf = l.recs + (size_t)F * (size_t)N * sizeof(Rec);
    l.counter = l.zbuf + up16((size_t)F * H * W * sizeof(unsigned long long));
    l.list = l.counter + 16;
    l.total = l.list + up16((size_t)l.capacity * sizeof(LargeEntry));
    return l;
}

__global__ __launch_bounds__(kWave) void k_raster_cameras(const CamChunk ch, int n, RasterCam *__restrict__ cams) {
    const int t = threadIdx.x;
    constexpr int words = sizeof(RasterCam) / sizeof(double);
    for (int k = t; k < n * words; k += kWave) reinterpret_cast<double *>(cams)[k] = reinterpret_cast<const double *>(ch.c)[k];
}

__global__ __launch_bounds__(kThreads) void k_raster_clear(unsigned long long *__restrict__ zbuf, int64_t n, unsigned long long *__restrict__ counter,
                                                           int *__restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) zbuf[i] = kEmpty;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counter[0] = 0, counter[1] = 0;
        if (status) *status = 0;
    }
}

struct ProjectArgs {
    const float *vertices;                        // (Fv,N,3)
    int64_t N;
    int vertex_frames;                            // 1: shared by every image
    const RasterCam *cams;
    int cam_frames;                               // 1: shared
    double znear;
    Rec *recs;                                    // (F,N)
};

__global__ __launch_bounds__(kThreads) void k_raster_project(const ProjectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t img = blockIdx.y;
    const float *vp = a.vertices + ((a.vertex_frames == 1 ? 0 : img) * a.N + i) * 3;
    const RasterCam &c = a.cams[a.cam_frames == 1 ? 0 : img];
    const double v[3] = {(double)vp[0], (double)vp[1], (double)vp[2]};
    double cam[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = ((c.R[3 * r] * v[0] + c.R[3 * r + 1] * v[1]) + c.R[3 * r + 2] * v[2]) + c.T[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = (c.K[3 * r] * cam[0] + c.K[3 * r + 1] * cam[1]) + c.K[3 * r + 2] * cam[2];
    const double sx = p[0] / p[2], sy = p[1] / p[2];
    const double lim = (double)kGuard;
    // (every comparison is false for NaN: a non-finite coordinate fails one of them)
    const bool ok = fabs(sx) <= lim && fabs(sy) <= lim && cam[2] > a.znear && cam[2] < (double)INFINITY && fabs(cam[0]) < (double)INFINITY &&
                    fabs(cam[1]) < (double)INFINITY;
    Rec r;
    r.X = ok ? (int)llrint(sx * 256.0) : 0;
    r.Y = ok ? (int)llrint(sy * 256.0) : 0;
    r.z = ok ? (float)cam[2] : 0.f;
    r.flags = ok ? 0u : 1u;
    reinterpret_cast<int4 *>(a.recs)[img * a.N + i] = make_int4(r.X, r.Y, __float_as_int(r.z), (int)r.flags);
}

__device__ __forceinline__ Rec load_rec(const Rec *__restrict__ recs, int64_t k) {
    const int4 q = reinterpret_cast<const int4 *>(recs)[k];
    Rec r;
    r.X = q.x, r.Y = q.y, r.z = __int_as_float(q.z), r.flags = (unsigned)q.w;
    return r;
}

struct Setup {                                    // a triangle ready to draw: A > 0, vertices in drawing order
    int64_t X[3], Y[3], A;
    float z[3];
    bool swapped;
    int x0, x1, y0, y1;                           // clamped box, inclusive; empty when x1 < x0 or y1 < y0
};

enum { kCullBack = 1, kCullFront = 2 };

// records of one image, validated indices -> Setup; false: nothing to draw
__device__ __forceinline__ bool setup_triangle(const Rec *__restrict__ recs, int i0, int i1, int i2, int cull, int H, int W, Setup &s) {
    const Rec r0 = load_rec(recs, i0), r1 = load_rec(recs, i1), r2 = load_rec(recs, i2);
    if ((r0.flags | r1.flags | r2.flags) & 1u) return false;
    const int64_t A = ((int64_t)r1.X - r0.X) * ((int64_t)r2.Y - r0.Y) - ((int64_t)r1.Y - r0.Y) * ((int64_t)r2.X - r0.X);
    if (A == 0 || (A < 0 && cull == kCullBack) || (A > 0 && cull == kCullFront)) return false;
    s.swapped = A < 0;
    const Rec ra = s.swapped ? r2 : r1, rb = s.swapped ? r1 : r2;
    s.A = s.swapped ? -A : A;
    s.X[0] = r0.X, s.X[1] = ra.X, s.X[2] = rb.X;
    s.Y[0] = r0.Y, s.Y[1] = ra.Y, s.Y[2] = rb.Y;
    s.z[0] = r0.z, s.z[1] = ra.z, s.z[2] = rb.z;
    const int xmin = min(r0.X, min(r1.X, r2.X)), xmax = max(r0.X, max(r1.X, r2.X));
    const int ymin = min(r0.Y, min(r1.Y, r2.Y)), ymax = max(r0.Y, max(r1.Y, r2.Y));
    // ceil and floor of k / 256 by arithmetic shifts (|k| <= 2^27: no overflow)
    s.x0 = max((xmin + 255) >> 8, 0), s.x1 = min(xmax >> 8, W - 1);
    s.y0 = max((ymin + 255) >> 8, 0), s.y1 = min(ymax >> 8, H - 1);
    return s.x0 <= s.x1 && s.y0 <= s.y1;
}

// the three edge functions at pixel (px, py); true when the pixel is covered
__device__ __forceinline__ bool edge_functions(const Setup &s, int px, int py, int64_t (&E)[3]) {
    const int64_t PX = (int64_t)px * 256, PY = (int64_t)py * 256;
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const int64_t dx = s.X[b] - s.X[a], dy = s.Y[b] - s.Y[a];
        E[i] = dx * (PY - s.Y[a]) - dy * (PX - s.X[a]);
        in = in && (E[i] > 0 || (E[i] == 0 && (dy < 0 || (dy == 0 && dx > 0))));
    }
    return in;
}

// b_i / z_i, i = 0 .. 2, and the depth they give
__device__ __forceinline__ float depth_of(const Setup &s, const int64_t (&E)[3], float (&q)[3]) {
    const float fA = (float)s.A;
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = ((float)E[i] / fA) / s.z[i];
    return 1.f / ((q[0] + q[1]) + q[2]);
}

__device__ __forceinline__ void draw_pixel(const Setup &s, int px, int py, unsigned tri, unsigned long long *__restrict__ zimg, int W) {
    int64_t E[3];
    if (!edge_functions(s, px, py, E)) return;
    float q[3];
    const float depth = depth_of(s, E, q);
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | tri;
    unsigned long long *word = zimg + (int64_t)py * W + px;
    if (*word < key) return;                      // (a stale value is only ever larger than the stored one)
    atomicMin(word, key);
}

struct CoverArgs {
    const Rec *recs;                              // (F,N)
    const int *triangles;                         // (T,3)
    int64_t N, T;
    int F, H, W, cull;
    unsigned long long *zbuf;                     // (F,H,W)
    unsigned long long *counter;
    LargeEntry *list;
    int64_t capacity;
    int *status;                                  // or NULL
};

__global__ __launch_bounds__(kThreads) void k_raster_cover(const CoverArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t img = blockIdx.y;
    Setup s;
    bool draw = false;
    if (t < a.T) {
        int iv[3];
        if (load_indices(a.triangles, t, a.N, iv))
            draw = setup_triangle(a.recs + img * a.N, iv[0], iv[1], iv[2], a.cull, a.H, a.W, s);
        else if (a.status)
            atomicOr(a.status, 1);
    }
    const int64_t pixels = draw ? (int64_t)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) : 0;       // (< 2^31: H W is)
    const bool large = pixels > HL_RASTER_SMALL_BOX;
    // (all 64 lanes reach the ballot: nothing above returns)
    const unsigned long long m = __ballot(large);
    if (m) {
        const int lane = (int)(threadIdx.x % kWave);
        const int leader = __ffsll(m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(a.counter, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (large) {
            const int64_t slot = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < a.capacity) {
                LargeEntry e;
                e.tri = (unsigned)t, e.img = (unsigned)img, e.pixels = (unsigned)pixels, e.pad = 0;
                a.list[slot] = e;
                draw = false;
            }
        }
    }
    if (!draw) return;
    unsigned long long *zimg = a.zbuf + img * a.H * a.W;
    for (int py = s.y0; py <= s.y1; ++py)
        for (int px = s.x0; px <= s.x1; ++px) draw_pixel(s, px, py, (unsigned)t, zimg, a.W);
}

__global__ __launch_bounds__(kThreads) void k_raster_cover_large(const CoverArgs a) {
    const unsigned long long listed = *a.counter;
    const int64_t count = listed < (unsigned long long)a.capacity ? (int64_t)listed : a.capacity;
    const int lane = (int)(threadIdx.x % kWave);
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave, waves = (int64_t)gridDim.x * (kThreads / kWave);
    const int64_t first = (int64_t)blockIdx.y * kWave;     // this slice's first pixel of the box
    for (int64_t e = wave; e < count; e += waves) {
        const LargeEntry le = a.list[e];
        const int64_t t = le.tri, img = le.img;
        if (le.pixels <= first) continue;
        if (t >= a.T || img >= a.F) continue;              // (entries come from k_raster_cover; never index outside whatever they hold)
        int iv[3];
        Setup s;
        if (!load_indices(a.triangles, t, a.N, iv)) continue;
        if (!setup_triangle(a.recs + img * a.N, iv[0], iv[1], iv[2], a.cull, a.H, a.W, s)) continue;
        unsigned long long *zimg = a.zbuf + img * a.H * a.W;
        const int bw = s.x1 - s.x0 + 1;
        const int64_t n = (int64_t)bw * (s.y1 - s.y0 + 1);
        for (int64_t k = first + lane; k < n; k += (int64_t)kWave * kLargeSlices) draw_pixel(s, s.x0 + (int)(k % bw), s.y0 + (int)(k / bw), (unsigned)t, zimg, a.W);
    }
}

// x / |x|, (0,0,0) for a zero or non-finite vector
__device__ __forceinline__ void normalize3(float (&v)[3]) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const bool ok = len > 0.f && len < INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = ok ? v[i] / len : 0.f;
}

struct ResolveArgs {
    CoverArgs c;
    const float *vertices;                        // (Fv,N,3)
    int vertex_frames;
    const float *normals;                         // (Fn,N,3) or NULL
    int normal_frames;
    const unsigned char *colors;                  // (N,3) or NULL
    const RasterCam *cams;
    int cam_frames;
    int headlight, white;
    float *rgb, *acc, *normal, *depth, *bary;
    int *tri_id;
};

__global__ __launch_bounds__(kThreads) void k_raster_resolve(const ResolveArgs a) {
    const int64_t hw = (int64_t)a.c.H * a.c.W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= hw) return;
    const int64_t img = blockIdx.y, o = img * hw + p;
    const int px = (int)(p % a.c.W), py = (int)(p / a.c.W);
    const unsigned long long key = a.c.zbuf[o];
    const int64_t t = (int64_t)(key & 0xffffffffull);
    float rgb[3], nrm[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f}, depth = 0.f, acc = 0.f;
    int id = -1;
    rgb[0] = rgb[1] = rgb[2] = a.white ? 1.f : 0.f;
    int ti[3];                                    // the triangle's own order
    Setup s;
    if (key != kEmpty && t < a.c.T && load_indices(a.c.triangles, t, a.c.N, ti) &&
        setup_triangle(a.c.recs + img * a.c.N, ti[0], ti[1], ti[2], a.c.cull, a.c.H, a.c.W, s)) {
        int64_t E[3];
        edge_functions(s, px, py, E);
        float q[3];
        depth_of(s, E, q);
        depth = __uint_as_float((unsigned)(key >> 32));
        acc = 1.f, id = (int)t;
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = q[i] * depth;
        const int iv[3] = {ti[0], s.swapped ? ti[2] : ti[1], s.swapped ? ti[1] : ti[2]};      // the drawing order
        const RasterCam &cam = a.cams[a.cam_frames == 1 ? 0 : img];
        if (a.normals) {
            const float *nb = a.normals + (a.normal_frames == 1 ? 0 : img) * a.c.N * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) nrm[c] = (w[0] * nb[(int64_t)iv[0] * 3 + c] + w[1] * nb[(int64_t)iv[1] * 3 + c]) + w[2] * nb[(int64_t)iv[2] * 3 + c];
            normalize3(nrm);
        } else {
            // the flat normal of the triangle in its own order, turned towards the camera
            const float *vb = a.vertices + (a.vertex_frames == 1 ? 0 : img) * a.c.N * 3;
            const float *v0 = vb + (int64_t)ti[0] * 3, *v1 = vb + (int64_t)ti[1] * 3, *v2 = vb + (int64_t)ti[2] * 3;
            const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
            nrm[0] = e1[1] * e2[2] - e1[2] * e2[1], nrm[1] = e1[2] * e2[0] - e1[0] * e2[2], nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
            const float d[3] = {v0[0] - (float)cam.o[0], v0[1] - (float)cam.o[1], v0[2] - (float)cam.o[2]};
            if ((nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2] > 0.f) nrm[0] = -nrm[0], nrm[1] = -nrm[1], nrm[2] = -nrm[2];
            normalize3(nrm);
        }
        if (a.colors) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float c0 = (float)a.colors[(int64_t)iv[0] * 3 + c] / 255.f, c1 = (float)a.colors[(int64_t)iv[1] * 3 + c] / 255.f,
                            c2 = (float)a.colors[(int64_t)iv[2] * 3 + c] / 255.f;
                rgb[c] = (w[0] * c0 + w[1] * c1) + w[2] * c2;
            }
        } else {
            rgb[0] = rgb[1] = rgb[2] = 0.7f;
        }
        if (a.headlight) {
            // the pixel's ray direction as camera_ray_pixel forms it (hl_camera.h), rounded to fp32 there, unit length here
            const double x = (double)px, y = (double)py;
            double qc[3];
            float df[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) qc[c] = ((x * cam.Ki[c * 3 + 0] + y * cam.Ki[c * 3 + 1]) + cam.Ki[c * 3 + 2]) - cam.T[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) df[c] = (float)(((qc[0] * cam.R[0 * 3 + c] + qc[1] * cam.R[1 * 3 + c]) + qc[2] * cam.R[2 * 3 + c]) - cam.o[c]);
            normalize3(df);
            const float sh = fabsf((nrm[0] * df[0] + nrm[1] * df[1]) + nrm[2] * df[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * sh;
        }
        if (s.swapped) {                          // back to the triangle's own vertex order
            const float t1 = w[1];
            w[1] = w[2], w[2] = t1;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb[o * 3 + c] = rgb[c], a.normal[o * 3 + c] = nrm[c];
    a.acc[o] = acc, a.depth[o] = depth;
    if (a.tri_id) a.tri_id[o] = id;
    if (a.bary) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.bary[o * 3 + c] = w[c];
    }
}

inline bool sizes_ok(int64_t N, int64_t T, int F, int H, int W) {
    return count_ok(N) && count_ok(T) && F >= 1 && F <= kMaxImages && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff;
}

}  // namespace
}  // namespace hl

using namespace hl;

extern "C" {

int hl_mesh_raster_small_box(void) { return HL_RASTER_SMALL_BOX; }

size_t hl_mesh_raster_scratch_bytes(int64_t N, int64_t T, int F, int H, int W) {
    return sizes_ok(N, T, F, H, W) ? layout_of(N, T, F, H, W).total : 0;
}

int hl_mesh_raster(const float *vertices, int vertex_frames, int64_t N, const int32_t *triangles, int64_t T, const float *normals, int normal_frames,
                   const unsigned char *colors, const double *h_cams, int cam_stride, int F, int H, int W, double znear, unsigned flags, float *rgb_map,
                   float *acc_map, float *normal_map, float *depth_map, int32_t *triangle_id, float *barycentrics, int32_t *status, void *scratch,
                   size_t scratch_bytes, void *stream) {
    HL_REQUIRE(sizes_ok(N, T, F, H, W), "hl_mesh_raster: bad sizes (N %lld, T %lld, F %d, H %d, W %d; all >= 1, F <= %d, N, T, H W < 2^31)",
               (long long)N, (long long)T, F, H, W, kMaxImages);
    HL_REQUIRE(vertex_frames == 1 || vertex_frames == F, "hl_mesh_raster: vertex_frames must be 1 or F (got %d, F %d)", vertex_frames, F);
    HL_REQUIRE(!normals || normal_frames == 1 || normal_frames == vertex_frames, "hl_mesh_raster: normal_frames must be 1 or vertex_frames (got %d)",
               normal_frames);
    HL_REQUIRE(cam_stride == 0 || cam_stride == HL_RASTER_CAM_ROW, "hl_mesh_raster: cam_stride must be 0 or %d (got %d)", HL_RASTER_CAM_ROW, cam_stride);
    HL_REQUIRE(znear > 0.0 && znear < (double)INFINITY, "hl_mesh_raster: znear must be positive and finite (got %g)", znear);
    HL_REQUIRE((flags & ~(unsigned)(HL_RASTER_WHITE_BKGD | HL_RASTER_HEADLIGHT | HL_RASTER_CULL_BACK | HL_RASTER_CULL_FRONT)) == 0 &&
                   (flags & (HL_RASTER_CULL_BACK | HL_RASTER_CULL_FRONT)) != (HL_RASTER_CULL_BACK | HL_RASTER_CULL_FRONT),
               "hl_mesh_raster: bad flags (%#x)", flags);
    HL_REQUIRE(vertices && triangles && h_cams && rgb_map && acc_map && normal_map && depth_map && scratch, "hl_mesh_raster: NULL argument");
    const Layout l = layout_of(N, T, F, H, W);
    HL_REQUIRE(scratch_bytes >= l.total, "hl_mesh_raster: scratch too small (%zu bytes, need %zu)", scratch_bytes, l.total);
    HL_REQUIRE(aligned16({scratch}), "hl_mesh_raster: scratch must be 16-byte aligned");
    char *base = static_cast<char *>(scratch);
    RasterCam *cams = reinterpret_cast<RasterCam *>(base + l.cams);
    Rec *recs = reinterpret_cast<Rec *>(base + l.recs);
    unsigned long long *zbuf = reinterpret_cast<unsigned long long *>(base + l.zbuf);
    unsigned long long *counter = reinterpret_cast<unsigned long long *>(base + l.counter);
    LargeEntry *list = reinterpret_cast<LargeEntry *>(base + l.list);
    const hipStream_t st = (hipStream_t)stream;
    const int cam_frames = cam_stride == 0 ? 1 : F;

    for (int c0 = 0; c0 < cam_frames; c0 += kCamsPerLaunch) {
        CamChunk ch;
        memset(&ch, 0, sizeof ch);
        const int n = cam_frames - c0 < kCamsPerLaunch ? cam_frames - c0 : kCamsPerLaunch;
        for (int k = 0; k < n; ++k) {
            const double *row = h_cams + (size_t)(c0 + k) * cam_stride, *hK = row, *hKi = row + 9, *hR = row + 18, *hT = row + 27;
            RasterCam &c = ch.c[k];
            for (int i = 0; i < 9; ++i) c.K[i] = hK[i], c.Ki[i] = hKi[i], c.R[i] = hR[i];
            for (int i = 0; i < 3; ++i) {
                c.T[i] = hT[i];
                c.o[i] = -((hR[0 * 3 + i] * hT[0] + hR[1 * 3 + i] * hT[1]) + hR[2 * 3 + i] * hT[2]);      // as cam_view_fill (hl_camera.h)
            }
        }
        hipLaunchKernelGGL(k_raster_cameras, dim3(1), dim3(kWave), 0, st, ch, n, cams + c0);
        const int rc = check_launch("k_raster_cameras");
        if (rc != HL_OK) return rc;
    }

    const int64_t zwords = (int64_t)F * H * W;
    const int64_t clear_blocks = blocks_of(zwords) < 2048 ? blocks_of(zwords) : 2048;
    hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)clear_blocks), dim3(kThreads), 0, st, zbuf, zwords, counter, status);
    int rc = check_launch("k_raster_clear");
    if (rc != HL_OK) return rc;

    ProjectArgs pa;
    pa.vertices = vertices, pa.N = N, pa.vertex_frames = vertex_frames, pa.cams = cams, pa.cam_frames = cam_frames, pa.znear = znear, pa.recs = recs;
    hipLaunchKernelGGL(k_raster_project, dim3((unsigned)blocks_of(N), (unsigned)F), dim3(kThreads), 0, st, pa);
    rc = check_launch("k_raster_project");
    if (rc != HL_OK) return rc;

    ResolveArgs ra;
    CoverArgs &ca = ra.c;
    ca.recs = recs, ca.triangles = triangles, ca.N = N, ca.T = T, ca.F = F, ca.H = H, ca.W = W;
    ca.cull = flags & HL_RASTER_CULL_BACK ? kCullBack : (flags & HL_RASTER_CULL_FRONT ? kCullFront : 0);
    ca.zbuf = zbuf, ca.counter = counter, ca.list = list, ca.capacity = l.capacity, ca.status = status;
    hipLaunchKernelGGL(k_raster_cover, dim3((unsigned)blocks_of(T), (unsigned)F), dim3(kThreads), 0, st, ca);
    rc = check_launch("k_raster_cover");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_raster_cover_large, dim3(kLargeBlocks, kLargeSlices), dim3(kThreads), 0, st, ca);
    rc = check_launch("k_raster_cover_large");
    if (rc != HL_OK) return rc;

    ra.vertices = vertices, ra.vertex_frames = vertex_frames, ra.normals = normals, ra.normal_frames = normal_frames, ra.colors = colors;
    ra.cams = cams, ra.cam_frames = cam_frames, ra.headlight = (flags & HL_RASTER_HEADLIGHT) != 0, ra.white = (flags & HL_RASTER_WHITE_BKGD) != 0;
    ra.rgb = rgb_map, ra.acc = acc_map, ra.normal = normal_map, ra.depth = depth_map, ra.bary = barycentrics, ra.tri_id = triangle_id;
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)blocks_of((int64_t)H * W), (unsigned)F), dim3(kThreads), 0, st, ra);
    return check_launch("k_raster_resolve");
}

}  // extern "C"
