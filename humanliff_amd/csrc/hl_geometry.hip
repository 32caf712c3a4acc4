// Mesh extraction on the MI355X: constrained smoothing and marching cubes behind Renderer.extract_geometry.
//
// Replaces the PyMCubes calls of the reference (human_diffusion/NeRF/renderer.py:290-321 and recon_NeRF/lib/renderer.py:304-348):
//   mcubes.smooth(u)                -> hl_smooth_prepare / hl_smooth_band / hl_smooth_sweeps / hl_smooth_scatter
//   mcubes.marching_cubes(u, iso)   -> hl_mc_count / hl_mc_emit
// The contract (signed distance, band, bounds, operator, stopping rule, corner rule, case table, ordering) is in DESIGN.md
// ("Mesh extraction"); tests/geometry_restatement.py states it again in numpy.  Everything is fp64, the file is built with
// -ffp-contract=off, and every reduction is integer or fixed-order, so results are bit-reproducible run to run.
#include "hl_reduce.h"
#include "hl_mc_table.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == hl::kReduceThreads, "block_sum / strided_sum reduce a workgroup of kReduceThreads");
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = TPB * SCAN_ITEMS;
constexpr int INF32 = 0x3fffffff;            // "no feature on this line yet" in the int32 squared-distance buffers
constexpr long long INF64 = 1LL << 40;       // the same inside the envelope arithmetic (squares of the lattice stay below 2^32)

inline long scan_blocks(long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
inline unsigned grid_of(long n) { return (unsigned)((n + TPB - 1) / TPB); }

// ---- exclusive scan of packed (low 32, high 32) integer counts; integer sums, so the order does not matter ----------------
template <class F>
__global__ __launch_bounds__(TPB) void k_scan_reduce(F f, long n, unsigned long long *__restrict__ block_sums) {
    __shared__ unsigned long long red[TPB];
    const long base = (long)blockIdx.x * SCAN_TILE;
    unsigned long long s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long i = base + (long)k * TPB + threadIdx.x;
        if (i < n) s += f(i);
    }
    s = hl::block_sum(s, red);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s;
}

__device__ unsigned long long block_exclusive(unsigned long long v, unsigned long long *sh, unsigned long long *total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 1; w < TPB; w <<= 1) {            // Hillis-Steele inclusive scan
        const unsigned long long add = (int)threadIdx.x >= w ? sh[threadIdx.x - w] : 0ull;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long incl = sh[threadIdx.x];
    if (total) *total = sh[TPB - 1];
    __syncthreads();
    return incl - v;
}

// one workgroup: block sums -> exclusive block offsets (in place); the grand total unpacked into counts[0] (low) / counts[1] (high)
__global__ __launch_bounds__(TPB) void k_scan_top(unsigned long long *__restrict__ block_sums, long nblocks, int64_t *__restrict__ counts) {
    __shared__ unsigned long long sh[TPB];
    const long chunk = (nblocks + TPB - 1) / TPB;
    const long b0 = (long)threadIdx.x * chunk;
    const long b1 = b0 + chunk < nblocks ? b0 + chunk : nblocks;
    unsigned long long s = 0;
    for (long b = b0; b < b1; ++b) s += block_sums[b];
    unsigned long long total;
    unsigned long long run = block_exclusive(s, sh, &total);
    for (long b = b0; b < b1; ++b) {
        const unsigned long long v = block_sums[b];
        block_sums[b] = run;
        run += v;
    }
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)(total & 0xffffffffull);
        counts[1] = (int64_t)(total >> 32);
    }
}

template <class F, class O>
__global__ __launch_bounds__(TPB) void k_scan_down(F f, O out, long n, const unsigned long long *__restrict__ block_off) {
    __shared__ unsigned long long sh[TPB];
    const long base = (long)blockIdx.x * SCAN_TILE + (long)threadIdx.x * SCAN_ITEMS;
    unsigned long long s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += f(base + k);
    unsigned long long run = block_off[blockIdx.x] + block_exclusive(s, sh, nullptr);
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long i = base + k;
        if (i >= n) break;
        const unsigned long long v = f(i);
        out(i, run, v);
        run += v;
    }
}

// ---- exact squared Euclidean distance transform, one axis per pass (Meijster et al. 2000 lower envelope) ------------------
// Source of the first pass: f = 0 on feature voxels (v > 0 equals `feature`), INF elsewhere; later passes read the int32 buffer.
template <class T>
struct FeatureSrc {
    const T *v;
    int feature;
    __device__ long long operator()(long i) const { return ((v[i] > (T)0) == (bool)feature) ? 0 : INF64; }
};
struct BufSrc {
    const int *b;
    __device__ long long operator()(long i) const { const int x = b[i]; return x >= INF32 ? INF64 : (long long)x; }
};

__device__ inline long long floordiv(long long a, long long b) {   // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// One thread per line. Line l = (l / inner, l % inner) -> base = (l / inner) * outer_stride + (l % inner) * inner_stride; the
// line's n points are `stride` apart.  s / t: the envelope's sites and starts, n x nlines ints laid out [k][line] (coalesced).
template <class S>
__global__ __launch_bounds__(TPB) void k_edt_pass(S src, int *__restrict__ out, long nlines, int n, long stride, long inner,
                                                  long outer_stride, long inner_stride, int *__restrict__ s, int *__restrict__ t) {
    const long l = (long)blockIdx.x * TPB + threadIdx.x;
    if (l >= nlines) return;
    const long base = (l / inner) * outer_stride + (l % inner) * inner_stride;
    auto f = [&](int i) { return src(base + (long)i * stride); };
    auto F = [&](long long x, int i, long long fi) { return (x - i) * (x - i) + fi; };
    int q = 0;
    s[l] = 0;
    t[l] = 0;
    for (int u = 1; u < n; ++u) {
        const long long fu = f(u);
        while (q >= 0) {
            const int sq = s[(long)q * nlines + l];
            const int tq = t[(long)q * nlines + l];
            if (F(tq, sq, f(sq)) > F(tq, u, fu)) --q;
            else break;
        }
        if (q < 0) {
            q = 0;
            s[l] = u;
            t[l] = 0;
        } else {
            const int sq = s[(long)q * nlines + l];
            const long long w = 1 + floordiv((long long)u * u - (long long)sq * sq + fu - f(sq), 2LL * (u - sq));
            if (w < n) {
                ++q;
                s[(long)q * nlines + l] = u;
                t[(long)q * nlines + l] = (int)w;
            }
        }
    }
    for (int u = n - 1; u >= 0; --u) {
        const int sq = s[(long)q * nlines + l];
        const long long d = F(u, sq, f(sq));
        out[base + (long)u * stride] = d >= INF32 ? INF32 : (int)d;
        if (u == t[(long)q * nlines + l]) --q;
    }
}

// d = edt(b) - 0.5 on b, -edt(~b) + 0.5 off b; each call fills the voxels of one class
template <class T>
__global__ __launch_bounds__(TPB) void k_signed(const T *__restrict__ v, const int *__restrict__ dsq, int cls, long n, double *__restrict__ d) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if ((v[i] > (T)0) != (bool)cls) return;
    const double e = sqrt((double)dsq[i]);
    d[i] = cls ? e - 0.5 : -e + 0.5;
}

template <class T>
int signed_distance(const T *v, int nx, int ny, int nz, double *d, int *bufA, int *bufB, int *s, int *t, hipStream_t st) {
    const long n = (long)nx * ny * nz, nyz = (long)ny * nz;
    for (int cls = 0; cls < 2; ++cls) {
        // features: the voxels of the OTHER class; distance filled in on the voxels of class `cls`
        FeatureSrc<T> fs{v, 1 - cls};
        hipLaunchKernelGGL((k_edt_pass<FeatureSrc<T>>), dim3(grid_of((long)nx * ny)), dim3(TPB), 0, st, fs, bufA, (long)nx * ny, nz, 1L,
                           (long)ny, nyz, (long)nz, s, t);                              // along z: lines (x, y)
        hipLaunchKernelGGL((k_edt_pass<BufSrc>), dim3(grid_of((long)nx * nz)), dim3(TPB), 0, st, BufSrc{bufA}, bufB, (long)nx * nz, ny,
                           (long)nz, (long)nz, nyz, 1L, s, t);                          // along y: lines (x, z)
        hipLaunchKernelGGL((k_edt_pass<BufSrc>), dim3(grid_of(nyz)), dim3(TPB), 0, st, BufSrc{bufB}, bufA, nyz, nx, nyz, nyz, 0L, 1L,
                           s, t);                                                       // along x: lines (y, z)
        hipLaunchKernelGGL((k_signed<T>), dim3(grid_of(n)), dim3(TPB), 0, st, v, bufA, cls, n, d);
    }
    return hl::check_launch("hl_smooth_prepare: signed distance");
}

// ---- band ---------------------------------------------------------------------------------------------------------------
struct BandCount {   // low: band voxel, high: voxel with v > 0 (d > 0 exactly there)
    const double *d;
    double r;
    __device__ unsigned long long operator()(long i) const {
        const double x = d[i];
        return (unsigned long long)(fabs(x) <= r) | ((unsigned long long)(x > 0.0) << 32);
    }
};
struct BandOut {
    const double *d;
    long nb;          // (the caller's band size: a slot beyond it is never written)
    int *slot;
    int *lin;
    double *x, *lower, *upper;
    __device__ void operator()(long i, unsigned long long prefix, unsigned long long v) const {
        if (!(v & 1ull)) {
            slot[i] = -1;
            return;
        }
        const int s = (int)(prefix & 0xffffffffull);
        if (s >= nb) {
            slot[i] = -1;
            return;
        }
        const double di = d[i];
        double lo = di > 0.0 ? di : -HUGE_VAL, hi = di < 0.0 ? di : HUGE_VAL;
        if (lo != -HUGE_VAL && fabs(lo) < 1.0) lo = 0.0;
        if (hi != HUGE_VAL && fabs(hi) < 1.0) hi = 0.0;
        slot[i] = s;
        lin[s] = (int)i;
        x[s] = di;
        lower[s] = lo;
        upper[s] = hi;
    }
};

__global__ __launch_bounds__(TPB) void k_band_nbr(const int *__restrict__ lin, const int *__restrict__ slot, int nx, int ny, int nz, long nb,
                                                  int *__restrict__ nbr) {
    const long s = (long)blockIdx.x * TPB + threadIdx.x;
    if (s >= nb) return;
    const long i = lin[s];
    const int c[3] = {(int)(i / ((long)ny * nz)), (int)((i / nz) % ny), (int)(i % nz)};
    const int dim[3] = {nx, ny, nz};
    const long step[3] = {(long)ny * nz, (long)nz, 1L};
    for (int a = 0; a < 3; ++a) {
        nbr[(2 * a) * nb + s] = c[a] > 0 ? slot[i - step[a]] : -1;
        nbr[(2 * a + 1) * nb + s] = c[a] + 1 < dim[a] ? slot[i + step[a]] : -1;
    }
}

// ---- damped projected Jacobi on A = Q^T Q ---------------------------------------------------------------------------------
// g[a][s] = sum over band neighbours along a of (x_nb - x_s); with `partial`, also the workgroup's sum of g^2 (x^T A x = |Q x|^2)
__global__ __launch_bounds__(TPB) void k_grad(const int *__restrict__ nbr, const double *__restrict__ x, long nb, double *__restrict__ g,
                                              double *__restrict__ partial) {
    __shared__ double red[TPB];
    const long s = (long)blockIdx.x * TPB + threadIdx.x;
    double e = 0.0;
    if (s < nb) {
        const double xc = x[s];
        for (int a = 0; a < 3; ++a) {
            const int n0 = nbr[(2 * a) * nb + s], n1 = nbr[(2 * a + 1) * nb + s];
            double ga = 0.0;
            if (n0 >= 0) ga += x[n0] - xc;
            if (n1 >= 0) ga += x[n1] - xc;
            g[a * nb + s] = ga;
            e += ga * ga;
        }
    }
    if (!partial) return;
    e = hl::block_sum(e, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = e;
}

__global__ __launch_bounds__(TPB) void k_energy_final(const double *__restrict__ partial, long nparts, double *__restrict__ energy) {
    __shared__ double red[TPB];
    const double e = hl::strided_sum(partial, nparts, 1, red);
    if (threadIdx.x == 0) energy[0] = 0.5 * e;
}

// (A x)_s = sum_a ( -m_a g[a][s] + sum_{band nb along a} g[a][nb] ), diag_s = sum_a (m_a^2 + m_a);
// y = -((A x) - diag x) / diag, x' = clamp(w y + (1 - w) x, lower, upper), w = 1/2
__global__ __launch_bounds__(TPB) void k_jacobi(const int *__restrict__ nbr, const double *__restrict__ g, const double *__restrict__ x,
                                                const double *__restrict__ lower, const double *__restrict__ upper, long nb,
                                                double *__restrict__ xout) {
    const long s = (long)blockIdx.x * TPB + threadIdx.x;
    if (s >= nb) return;
    double ax = 0.0, diag = 0.0;
    for (int a = 0; a < 3; ++a) {
        const int n0 = nbr[(2 * a) * nb + s], n1 = nbr[(2 * a + 1) * nb + s];
        const double m = (double)((n0 >= 0) + (n1 >= 0));
        double nsum = 0.0;
        if (n0 >= 0) nsum += g[a * nb + n0];
        if (n1 >= 0) nsum += g[a * nb + n1];
        ax += -m * g[a * nb + s] + nsum;
        diag += m * m + m;
    }
    const double xc = x[s];
    const double y = -(ax - diag * xc) / diag;
    const double xn = 0.5 * y + 0.5 * xc;
    xout[s] = fmin(fmax(xn, lower[s]), upper[s]);
}

__global__ __launch_bounds__(TPB) void k_scatter(const double *__restrict__ x, const int *__restrict__ lin, long nb, double *__restrict__ out) {
    const long s = (long)blockIdx.x * TPB + threadIdx.x;
    if (s < nb) out[lin[s]] = x[s];
}

// ---- marching cubes -------------------------------------------------------------------------------------------------------
// code[i] = owned crossing edges (bit a: edge from voxel i along axis a) | triangle count of the cube at i << 3
__global__ __launch_bounds__(TPB) void k_mc_classify(const double *__restrict__ v, int nx, int ny, int nz, double iso,
                                                     unsigned char *__restrict__ code) {
    const long n = (long)nx * ny * nz;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const long nyz = (long)ny * nz;
    const int x = (int)(i / nyz), y = (int)((i / nz) % ny), z = (int)(i % nz);
    const bool a = v[i] > iso;
    unsigned c = 0;
    if (x + 1 < nx && (v[i + nyz] > iso) != a) c |= 1u;
    if (y + 1 < ny && (v[i + nz] > iso) != a) c |= 2u;
    if (z + 1 < nz && (v[i + 1] > iso) != a) c |= 4u;
    if (x + 1 < nx && y + 1 < ny && z + 1 < nz) {
        unsigned cfg = 0;
        for (int k = 0; k < 8; ++k)
            cfg |= (unsigned)(v[i + (k & 1) * nyz + ((k >> 1) & 1) * nz + ((k >> 2) & 1)] > iso) << k;
        c |= (unsigned)HL_MC_NTRI[cfg] << 3;
    }
    code[i] = (unsigned char)c;
}

struct McCount {
    const unsigned char *code;
    __device__ unsigned long long operator()(long i) const {
        const unsigned c = code[i];
        return (unsigned long long)__popc(c & 7u) | ((unsigned long long)(c >> 3) << 32);
    }
};
struct McOut {
    int *voff, *toff;
    __device__ void operator()(long i, unsigned long long prefix, unsigned long long) const {
        voff[i] = (int)(prefix & 0xffffffffull);
        toff[i] = (int)(prefix >> 32);
    }
};

__global__ __launch_bounds__(TPB) void k_mc_emit(const double *__restrict__ v, int nx, int ny, int nz, double iso,
                                                 const unsigned char *__restrict__ code, const int *__restrict__ voff,
                                                 const int *__restrict__ toff, double *__restrict__ verts, int64_t *__restrict__ tris) {
    const long n = (long)nx * ny * nz;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const unsigned c = code[i];
    if (c == 0) return;
    const long nyz = (long)ny * nz;
    const int p[3] = {(int)(i / nyz), (int)((i / nz) % ny), (int)(i % nz)};
    const long step[3] = {nyz, (long)nz, 1L};
    const double fa = v[i];
    long j = voff[i];
    for (int a = 0; a < 3; ++a) {
        if (!(c & (1u << a))) continue;
        const double fb = v[i + step[a]];
        const double t = (iso - fa) / (fb - fa);
        for (int k = 0; k < 3; ++k) verts[j * 3 + k] = k == a ? (double)p[k] + t : (double)p[k];
        ++j;
    }
    const unsigned nt = c >> 3;
    if (nt == 0) return;
    unsigned cfg = 0;
    for (int k = 0; k < 8; ++k) cfg |= (unsigned)(v[i + (k & 1) * nyz + ((k >> 1) & 1) * nz + ((k >> 2) & 1)] > iso) << k;
    if (HL_MC_NTRI[cfg] != nt) return;           // (another iso than hl_mc_count's: never index past the case's triangles)
    const long t0 = toff[i];
    for (unsigned tr = 0; tr < nt; ++tr) {
        for (int k = 0; k < 3; ++k) {
            const int e = HL_MC_TRIS[cfg][tr][k];
            const int ax = e >> 2, o0 = e & 1, o1 = (e >> 1) & 1;
            int d[3] = {0, 0, 0};
            d[ax == 0 ? 1 : 0] = o0;                 // the edge's lower corner: the two other coordinates, in axis order
            d[ax == 2 ? 1 : 2] = o1;
            const long owner = i + d[0] * nyz + d[1] * nz + d[2];
            tris[(t0 + tr) * 3 + k] = (int64_t)voff[owner] + __popc(code[owner] & ((1u << ax) - 1u));
        }
    }
}

// workspace layouts
struct SmoothWs {
    int *a, *b, *s, *t;
    unsigned long long *blocks;
};
SmoothWs smooth_ws(void *ws, long n) {
    char *p = (char *)ws;
    SmoothWs w;
    w.a = (int *)p; p += n * 4;
    w.b = (int *)p; p += n * 4;
    w.s = (int *)p; p += n * 4;
    w.t = (int *)p; p += n * 4;
    w.blocks = (unsigned long long *)p;
    return w;
}
struct McWs {
    int *voff, *toff;
    unsigned long long *blocks;
    unsigned char *code;
};
McWs mc_ws(void *ws, long n) {
    char *p = (char *)ws;
    McWs w;
    w.voff = (int *)p; p += n * 4;
    w.toff = (int *)p; p += n * 4;
    w.blocks = (unsigned long long *)p; p += scan_blocks(n) * 8;
    w.code = (unsigned char *)p;
    return w;
}

// the int32 slots / offsets and the 5-triangles-per-cube bound keep every index below 2^31
bool volume_ok(int nx, int ny, int nz) {
    return nx > 0 && ny > 0 && nz > 0 && (long long)nx * ny * nz * HL_MC_MAX_TRI < (1LL << 31);
}

}  // namespace

extern "C" size_t hl_smooth_workspace_bytes(int nx, int ny, int nz) {
    if (!volume_ok(nx, ny, nz)) return 0;
    const long n = (long)nx * ny * nz;
    return (size_t)(n * 16 + scan_blocks(n) * 8);
}

extern "C" int hl_smooth_prepare(const void *vol, int is_fp64, int nx, int ny, int nz, double band_radius, double *d_out, int64_t *counts,
                                 void *ws, size_t ws_bytes, void *stream) {
    HL_REQUIRE(vol && d_out && counts && ws, "hl_smooth_prepare: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_smooth_prepare: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_smooth_workspace_bytes(nx, ny, nz), "hl_smooth_prepare: workspace too small");
    const long n = (long)nx * ny * nz;
    hipStream_t st = (hipStream_t)stream;
    SmoothWs w = smooth_ws(ws, n);
    const int rc = is_fp64 ? signed_distance((const double *)vol, nx, ny, nz, d_out, w.a, w.b, w.s, w.t, st)
                           : signed_distance((const float *)vol, nx, ny, nz, d_out, w.a, w.b, w.s, w.t, st);
    if (rc) return rc;
    const long nbk = scan_blocks(n);
    hipLaunchKernelGGL((k_scan_reduce<BandCount>), dim3((unsigned)nbk), dim3(TPB), 0, st, BandCount{d_out, band_radius}, n, w.blocks);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(TPB), 0, st, w.blocks, nbk, counts);
    return hl::check_launch("hl_smooth_prepare");
}

extern "C" int hl_smooth_band(const double *d, int nx, int ny, int nz, double band_radius, int64_t nb, int *lin, int *nbr, double *x,
                              double *lower, double *upper, void *ws, size_t ws_bytes, void *stream) {
    HL_REQUIRE(d && lin && nbr && x && lower && upper && ws, "hl_smooth_band: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_smooth_band: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_smooth_workspace_bytes(nx, ny, nz), "hl_smooth_band: workspace too small");
    const long n = (long)nx * ny * nz;
    HL_REQUIRE(nb > 0 && nb <= n, "hl_smooth_band: band size %lld", (long long)nb);
    hipStream_t st = (hipStream_t)stream;
    SmoothWs w = smooth_ws(ws, n);
    BandOut o{d, (long)nb, w.a, lin, x, lower, upper};
    hipLaunchKernelGGL((k_scan_down<BandCount, BandOut>), dim3((unsigned)scan_blocks(n)), dim3(TPB), 0, st, BandCount{d, band_radius}, o, n,
                       (const unsigned long long *)w.blocks);
    hipLaunchKernelGGL(k_band_nbr, dim3(grid_of(nb)), dim3(TPB), 0, st, lin, w.a, nx, ny, nz, (long)nb, nbr);
    return hl::check_launch("hl_smooth_band");
}

extern "C" size_t hl_smooth_sweep_scratch_bytes(int64_t nb) {
    return (size_t)(nb * 4 * 8 + (long)grid_of(nb) * 8);
}

extern "C" int hl_smooth_sweeps(const int *nbr, const double *lower, const double *upper, int64_t nb, int n_sweeps, double *x, double *energy,
                                void *scratch, size_t scratch_bytes, void *stream) {
    HL_REQUIRE(nbr && lower && upper && x && scratch, "hl_smooth_sweeps: null argument");
    HL_REQUIRE(nb > 0 && nb < (1LL << 31) && n_sweeps >= 0, "hl_smooth_sweeps: bad sizes");
    HL_REQUIRE(scratch_bytes >= hl_smooth_sweep_scratch_bytes(nb), "hl_smooth_sweeps: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    double *g = (double *)scratch, *xt = g + 3 * nb, *partial = xt + nb;
    const unsigned gr = grid_of(nb);
    double *cur = x, *nxt = xt;
    for (int it = 0; it < n_sweeps; ++it) {
        hipLaunchKernelGGL(k_grad, dim3(gr), dim3(TPB), 0, st, nbr, cur, (long)nb, g, (double *)nullptr);
        hipLaunchKernelGGL(k_jacobi, dim3(gr), dim3(TPB), 0, st, nbr, g, cur, lower, upper, (long)nb, nxt);
        double *tmp = cur; cur = nxt; nxt = tmp;
    }
    if (cur != x) HL_HIP(hipMemcpyAsync(x, cur, nb * 8, hipMemcpyDeviceToDevice, st));
    if (energy) {
        hipLaunchKernelGGL(k_grad, dim3(gr), dim3(TPB), 0, st, nbr, x, (long)nb, g, partial);
        hipLaunchKernelGGL(k_energy_final, dim3(1), dim3(TPB), 0, st, partial, (long)gr, energy);
    }
    return hl::check_launch("hl_smooth_sweeps");
}

extern "C" int hl_smooth_scatter(const double *x, const int *lin, int64_t nb, double *out, void *stream) {
    HL_REQUIRE(x && lin && out && nb > 0 && nb < (1LL << 31), "hl_smooth_scatter: bad argument");
    hipLaunchKernelGGL(k_scatter, dim3(grid_of(nb)), dim3(TPB), 0, (hipStream_t)stream, x, lin, (long)nb, out);
    return hl::check_launch("hl_smooth_scatter");
}

extern "C" size_t hl_mc_workspace_bytes(int nx, int ny, int nz) {
    if (!volume_ok(nx, ny, nz)) return 0;
    const long n = (long)nx * ny * nz;
    return (size_t)(n * 9 + scan_blocks(n) * 8);
}

extern "C" int hl_mc_count(const double *vol, int nx, int ny, int nz, double iso, int64_t *counts, void *ws, size_t ws_bytes, void *stream) {
    HL_REQUIRE(vol && counts && ws, "hl_mc_count: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_mc_count: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_mc_workspace_bytes(nx, ny, nz), "hl_mc_count: workspace too small");
    const long n = (long)nx * ny * nz;
    hipStream_t st = (hipStream_t)stream;
    McWs w = mc_ws(ws, n);
    hipLaunchKernelGGL(k_mc_classify, dim3(grid_of(n)), dim3(TPB), 0, st, vol, nx, ny, nz, iso, w.code);
    hipLaunchKernelGGL((k_scan_reduce<McCount>), dim3((unsigned)scan_blocks(n)), dim3(TPB), 0, st, McCount{w.code}, n, w.blocks);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(TPB), 0, st, w.blocks, scan_blocks(n), counts);
    return hl::check_launch("hl_mc_count");
}

extern "C" int hl_mc_emit(const double *vol, int nx, int ny, int nz, double iso, double *verts, int64_t *tris, void *ws, size_t ws_bytes,
                          void *stream) {
    HL_REQUIRE(vol && ws, "hl_mc_emit: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_mc_emit: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_mc_workspace_bytes(nx, ny, nz), "hl_mc_emit: workspace too small");
    const long n = (long)nx * ny * nz;
    hipStream_t st = (hipStream_t)stream;
    McWs w = mc_ws(ws, n);
    hipLaunchKernelGGL((k_scan_down<McCount, McOut>), dim3((unsigned)scan_blocks(n)), dim3(TPB), 0, st, McCount{w.code}, McOut{w.voff, w.toff},
                       n, (const unsigned long long *)w.blocks);
    hipLaunchKernelGGL(k_mc_emit, dim3(grid_of(n)), dim3(TPB), 0, st, vol, nx, ny, nz, iso, w.code, w.voff, w.toff, verts, tris);
    return hl::check_launch("hl_mc_emit");
}

extern "C" int hl_mc_max_triangles(void) { return HL_MC_MAX_TRI; }

extern "C" int hl_mc_case_table(signed char *h_tris, unsigned char *h_ntri) {
    HL_REQUIRE(h_tris && h_ntri, "hl_mc_case_table: null argument");
    memcpy(h_tris, HL_MC_TRIS, sizeof(HL_MC_TRIS));
    memcpy(h_ntri, HL_MC_NTRI, sizeof(HL_MC_NTRI));
    return HL_OK;
}
