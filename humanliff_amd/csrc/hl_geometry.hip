// Mesh extraction on the MI355X: constrained smoothing and marching cubes behind Renderer.extract_geometry.
//
// Replaces the PyMCubes calls of the reference (human_diffusion/NeRF/renderer.py:290-321 and recon_NeRF/lib/renderer.py:304-348):
//   mcubes.smooth(u)                -> hl_smooth_prepare / hl_smooth_band / hl_smooth_sweeps / hl_smooth_scatter
//   mcubes.marching_cubes(u, iso)   -> hl_mc_count / hl_mc_emit
// and, beside the reference (which stops at vertices and triangles), finishes the mesh behind Renderer.extract_mesh:
//   components of the solid side    -> hl_cc_label / hl_cc_sizes / hl_cc_filter
//   vertex normals                  -> hl_mc_vertex_normals
//   vertex colours                  -> hl_mesh_pack_points / hl_mesh_unpack_colors around hl_render_eval_points
// The contract (signed distance, band, bounds, operator, stopping rule, corner rule, case table, ordering) is in DESIGN.md
// ("Mesh extraction"); tests/geometry_restatement.py states it again in numpy.  Everything is fp64, the file is built with
// -ffp-contract=off, and every reduction is integer or fixed-order, so results are bit-reproducible run to run.
#include "hl_scan.h"
#include "hl_mc_table.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == hl::kReduceThreads, "block_sum / strided_sum reduce a workgroup of kReduceThreads");
static_assert(TPB == hl::kScanThreads, "the scan kernels (hl_scan.h: the exclusive scan of packed integer counts) run workgroups of kScanThreads");
constexpr int INF32 = 0x3fffffff;            // "no feature on this line yet" in the int32 squared-distance buffers
constexpr long long INF64 = 1LL << 40;       // the same inside the envelope arithmetic (squares of the lattice stay below 2^32)

using hl::k_scan_down;
using hl::scan_blocks;
inline unsigned grid_of(long n) { return (unsigned)((n + TPB - 1) / TPB); }

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

// ---- vertex normals: the field's gradient, interpolated along the vertex's lattice edge -------------------------------------
// keys[j] = voxel * 3 + axis of vertex j, in hl_mc_emit's vertex order (voff as the scan left it)
__global__ __launch_bounds__(TPB) void k_mc_keys(const unsigned char *__restrict__ code, const int *__restrict__ voff, long n, long n_verts,
                                                 int *__restrict__ keys) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const unsigned c = code[i] & 7u;
    long j = voff[i];
    for (int a = 0; a < 3; ++a) {
        if (!(c & (1u << a))) continue;
        if (j < n_verts) keys[j] = (int)(i * 3 + a);
        ++j;
    }
}

// central difference at lattice point p, one-sided at a volume face, 0 along an axis of one voxel
__device__ inline void mc_gradient(const double *__restrict__ v, const int p[3], const int dim[3], const long step[3], double g[3]) {
    const long i = p[0] * step[0] + p[1] * step[1] + p[2] * step[2];
    for (int k = 0; k < 3; ++k) {
        if (dim[k] < 2) g[k] = 0.0;
        else if (p[k] == 0) g[k] = v[i + step[k]] - v[i];
        else if (p[k] == dim[k] - 1) g[k] = v[i] - v[i - step[k]];
        else g[k] = (v[i + step[k]] - v[i - step[k]]) * 0.5;
    }
}

__global__ __launch_bounds__(TPB) void k_mc_normals(const double *__restrict__ v, int nx, int ny, int nz, double iso, double ex, double ey,
                                                    double ez, const int *__restrict__ keys, long n_verts, double *__restrict__ normals) {
    const long j = (long)blockIdx.x * TPB + threadIdx.x;
    if (j >= n_verts) return;
    const long n = (long)nx * ny * nz, nyz = (long)ny * nz;
    const int key = keys[j];
    const long i = key / 3;
    const int a = key % 3;
    const int dim[3] = {nx, ny, nz};
    const long step[3] = {nyz, (long)nz, 1L};
    const double ext[3] = {ex, ey, ez};
    double out[3] = {0.0, 0.0, 0.0};
    if (key >= 0 && i < n) {
        int pa[3] = {(int)(i / nyz), (int)((i / nz) % ny), (int)(i % nz)};
        if (pa[a] + 1 < dim[a]) {                  // (an edge that leaves the volume is never a key of this volume)
            int pb[3] = {pa[0], pa[1], pa[2]};
            pb[a] += 1;
            const double fa = v[i], fb = v[i + step[a]];
            const double t = (iso - fa) / (fb - fa);
            double ga[3], gb[3];
            mc_gradient(v, pa, dim, step, ga);
            mc_gradient(v, pb, dim, step, gb);
            double len2 = 0.0;
            for (int k = 0; k < 3; ++k) {
                out[k] = ((1.0 - t) * ga[k] + t * gb[k]) / ext[k];
                len2 += out[k] * out[k];
            }
            const double len = sqrt(len2);
            const bool ok = len > 0.0 && len < HUGE_VAL;      // zero stays zero; NaN / inf give zero, never NaN
            for (int k = 0; k < 3; ++k) out[k] = ok ? out[k] / len : 0.0;
        }
    }
    for (int k = 0; k < 3; ++k) normals[j * 3 + k] = out[k];
}

// ---- connected components of the solid side (26-connectivity) --------------------------------------------------------------
// Union-find on parent[] (int32 voxel index): parent[i] = -1 off the solid side, and on it parent[i] <= i at all times; every
// update is an integer atomicMin, so entries only decrease.  Every access another workgroup may race with is an agent-scope
// atomic, and the host relaunches link + flatten until a round changes nothing (hl_cc_label).
__device__ inline int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root walk.  Invariant: parent[i] <= i on solid voxels and updates only decrease entries.  So whatever mix of old and new
// parents the walk reads, each step goes to a strictly smaller index and it ends at a self-parent after at most i steps: it
// never waits for another workgroup's write.
__device__ inline int cc_find(const int *parent, int i) {
    for (;;) {
        const int p = cc_load(parent + i);
        if (p >= i || p < 0) return i;
        i = p;
    }
}

// a + b strictly decreases with every iteration, so the loop ends on its own
__device__ inline bool cc_unite(int *parent, int a, int b) {
    bool changed = false;
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    while (a != b) {
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(parent + a, b);        // (agent scope)
        if (old > b) changed = true;
        if (old == a) break;                             // a was a root and now hangs below b
        a = old;                                         // a had the parent `old` already: old and b are one component too
    }
    return changed;
}

__global__ __launch_bounds__(TPB) void k_cc_init(const double *__restrict__ v, double iso, long n, int *__restrict__ parent) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) parent[i] = !(v[i] > iso) ? (int)i : -1;
}

__global__ __launch_bounds__(TPB) void k_cc_link(int *__restrict__ parent, int nx, int ny, int nz, int *__restrict__ changed) {
    const long n = (long)nx * ny * nz;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (cc_load(parent + i) < 0) return;
    const long nyz = (long)ny * nz;
    const int x = (int)(i / nyz), y = (int)((i / nz) % ny), z = (int)(i % nz);
    bool any = false;
    for (int k = 14; k < 27; ++k) {                      // the 13 neighbours behind i in C order
        const int dx = k / 9 - 1, dy = (k / 3) % 3 - 1, dz = k % 3 - 1;
        const int X = x + dx, Y = y + dy, Z = z + dz;
        if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
        const long j = i + dx * nyz + dy * (long)nz + dz;
        if (cc_load(parent + j) < 0) continue;
        any |= cc_unite(parent, (int)i, (int)j);
    }
    if (any) atomicOr(changed, 1);
}

// pointer jumping: every solid voxel takes the root its walk ends at (an ancestor: the entry only decreases)
__global__ __launch_bounds__(TPB) void k_cc_flatten(int *__restrict__ parent, long n) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int p = cc_load(parent + i);
    if (p < 0 || p == (int)i) return;
    const int r = cc_find(parent, p);
    if (r != p) atomicMin(parent + i, r);
}

struct CcRootCount {
    const int *parent;
    __device__ unsigned long long operator()(long i) const { return (unsigned long long)(parent[i] == (int)i); }
};
struct CcRankOut {
    int *rank;
    __device__ void operator()(long i, unsigned long long prefix, unsigned long long) const { rank[i] = (int)(prefix & 0xffffffffull); }
};

__global__ __launch_bounds__(TPB) void k_cc_labels(const int *__restrict__ parent, const int *__restrict__ rank, long n, int *__restrict__ labels,
                                                   int64_t *__restrict__ counts, int rounds) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i == 0) counts[1] = rounds;
    if (i >= n) return;
    const int p = parent[i];
    labels[i] = p < 0 ? 0 : rank[p] + 1;
}

__global__ __launch_bounds__(TPB) void k_cc_sizes(const int *__restrict__ labels, long n, long n_labels, unsigned long long *__restrict__ sizes) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int l = labels[i];
    if (l > 0 && l <= n_labels) atomicAdd(sizes + (l - 1), 1ull);
}

// a voxel of a dropped component moves to the above side, mirrored about iso; everything else is copied
__global__ __launch_bounds__(TPB) void k_cc_filter(const double *__restrict__ v, const int *__restrict__ labels, const unsigned char *__restrict__ keep,
                                                   long n, long n_labels, double iso, double *__restrict__ out) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int l = labels[i];
    double x = v[i];
    if (l > 0 && l <= n_labels && !keep[l - 1]) {
        x = iso + fabs(x - iso);
        if (!(x > iso)) x = nextafter(iso, HUGE_VAL);
    }
    out[i] = x;
}

// ---- vertex colours: the hand-over to and from hl_render_eval_points -------------------------------------------------------
// (V,3) points / directions -> float4 rows padded to a multiple of 32 (n_samples = 1: the tile-major layout is the plain array)
__global__ __launch_bounds__(TPB) void k_mesh_pack(const float *__restrict__ pts, const float *__restrict__ dirs, long nv, long nv32,
                                                   float4 *__restrict__ pts4, float4 *__restrict__ dirs4) {
    const long j = (long)blockIdx.x * TPB + threadIdx.x;
    if (j >= nv32) return;
    float4 p = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 1.f, 0.f};
    if (j < nv) {
        p = make_float4(pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2], 0.f);
        d = make_float4(dirs[j * 3], dirs[j * 3 + 1], dirs[j * 3 + 2], 0.f);
    }
    pts4[j] = p;
    dirs4[j] = d;
}

// raw records (sigma, r, g, b) -> sigmoid colours, the compositing kernels' form of it; u8 = round(clip(c, 0, 1) * 255)
__global__ __launch_bounds__(TPB) void k_mesh_colors(const float4 *__restrict__ rec, long nv, float *__restrict__ rgb, unsigned char *__restrict__ rgb8) {
    const long j = (long)blockIdx.x * TPB + threadIdx.x;
    if (j >= nv) return;
    const float4 r = rec[j];
    const float raw[3] = {r.y, r.z, r.w};
    for (int k = 0; k < 3; ++k) {
        const float c = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * raw[k]));
        rgb[j * 3 + k] = c;
        if (rgb8) rgb8[j * 3 + k] = (unsigned char)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.f);
    }
}

// workspace layouts
struct CcWs {
    int *parent, *rank;
    unsigned long long *blocks;
    int *changed;
};
CcWs cc_ws(void *ws, long n) {
    char *p = (char *)ws;
    CcWs w;
    w.parent = (int *)p; p += n * 4;
    w.rank = (int *)p; p += n * 4;
    w.blocks = (unsigned long long *)p; p += scan_blocks(n) * 8;
    w.changed = (int *)p;
    return w;
}
constexpr int CC_MAX_ROUNDS = 40;      // pointer jumping: logarithmic in the longest chain, and a chain is shorter than 2^31

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
    return hl::scan_total(BandCount{d_out, band_radius}, n, w.blocks, counts, st, "hl_smooth_prepare");
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
    return hl::scan_total(McCount{w.code}, n, w.blocks, counts, st, "hl_mc_count");
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

extern "C" int hl_mc_vertex_normals(const double *vol, int nx, int ny, int nz, double iso, const double *h_ext, int64_t n_verts, int *keys,
                                    double *normals, void *ws, size_t ws_bytes, void *stream) {
    HL_REQUIRE(vol && ws, "hl_mc_vertex_normals: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_mc_vertex_normals: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_mc_workspace_bytes(nx, ny, nz), "hl_mc_vertex_normals: workspace too small");
    const long n = (long)nx * ny * nz;
    HL_REQUIRE(n_verts >= 0 && n_verts <= 3 * n, "hl_mc_vertex_normals: vertex count %lld", (long long)n_verts);
    if (n_verts == 0) return HL_OK;
    HL_REQUIRE(keys && normals, "hl_mc_vertex_normals: null argument");
    const double ex = h_ext ? h_ext[0] : 1.0, ey = h_ext ? h_ext[1] : 1.0, ez = h_ext ? h_ext[2] : 1.0;
    hipStream_t st = (hipStream_t)stream;
    McWs w = mc_ws(ws, n);
    hipLaunchKernelGGL((k_scan_down<McCount, McOut>), dim3((unsigned)scan_blocks(n)), dim3(TPB), 0, st, McCount{w.code}, McOut{w.voff, w.toff},
                       n, (const unsigned long long *)w.blocks);
    hipLaunchKernelGGL(k_mc_keys, dim3(grid_of(n)), dim3(TPB), 0, st, (const unsigned char *)w.code, (const int *)w.voff, n, (long)n_verts, keys);
    hipLaunchKernelGGL(k_mc_normals, dim3(grid_of(n_verts)), dim3(TPB), 0, st, vol, nx, ny, nz, iso, ex, ey, ez, (const int *)keys, (long)n_verts,
                       normals);
    return hl::check_launch("hl_mc_vertex_normals");
}

extern "C" size_t hl_cc_workspace_bytes(int nx, int ny, int nz) {
    if (!volume_ok(nx, ny, nz)) return 0;
    const long n = (long)nx * ny * nz;
    return (size_t)(n * 8 + scan_blocks(n) * 8 + 8);
}

extern "C" int hl_cc_label(const double *vol, int nx, int ny, int nz, double iso, int *labels, int64_t *counts, void *ws, size_t ws_bytes,
                           void *stream) {
    HL_REQUIRE(vol && labels && counts && ws, "hl_cc_label: null argument");
    HL_REQUIRE(volume_ok(nx, ny, nz), "hl_cc_label: volume %d x %d x %d outside the supported sizes", nx, ny, nz);
    HL_REQUIRE(ws_bytes >= hl_cc_workspace_bytes(nx, ny, nz), "hl_cc_label: workspace too small");
    const long n = (long)nx * ny * nz;
    hipStream_t st = (hipStream_t)stream;
    CcWs w = cc_ws(ws, n);
    hipLaunchKernelGGL(k_cc_init, dim3(grid_of(n)), dim3(TPB), 0, st, vol, iso, n, w.parent);
    int rounds = 0;
    for (;;) {
        // one round: link, flatten, and the host reads whether anything moved (the pipeline's `counts` reads are of this kind)
        if (rounds == CC_MAX_ROUNDS)
            return hl::fail(HL_ERR_RUNTIME, "hl_cc_label: labels still changing after %d link / flatten rounds", CC_MAX_ROUNDS);
        ++rounds;
        HL_HIP(hipMemsetAsync(w.changed, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_cc_link, dim3(grid_of(n)), dim3(TPB), 0, st, w.parent, nx, ny, nz, w.changed);
        hipLaunchKernelGGL(k_cc_flatten, dim3(grid_of(n)), dim3(TPB), 0, st, w.parent, n);
        int changed = 0;
        HL_HIP(hipMemcpyAsync(&changed, w.changed, sizeof(int), hipMemcpyDeviceToHost, st));
        HL_HIP(hipStreamSynchronize(st));
        if (!changed) break;
    }
    const int rc = hl::scan_exclusive(CcRootCount{w.parent}, CcRankOut{w.rank}, n, w.blocks, counts, st, "hl_cc_label: scan");
    if (rc != HL_OK) return rc;
    hipLaunchKernelGGL(k_cc_labels, dim3(grid_of(n)), dim3(TPB), 0, st, (const int *)w.parent, (const int *)w.rank, n, labels, counts, rounds);
    return hl::check_launch("hl_cc_label");
}

extern "C" int hl_cc_sizes(const int *labels, int64_t n_voxels, int64_t n_labels, int64_t *sizes, void *stream) {
    HL_REQUIRE(labels && n_voxels > 0 && n_voxels < (1LL << 31) && n_labels >= 0, "hl_cc_sizes: bad argument");
    if (n_labels == 0) return HL_OK;
    HL_REQUIRE(sizes, "hl_cc_sizes: null argument");
    hipStream_t st = (hipStream_t)stream;
    HL_HIP(hipMemsetAsync(sizes, 0, (size_t)n_labels * 8, st));
    hipLaunchKernelGGL(k_cc_sizes, dim3(grid_of(n_voxels)), dim3(TPB), 0, st, labels, (long)n_voxels, (long)n_labels, (unsigned long long *)sizes);
    return hl::check_launch("hl_cc_sizes");
}

extern "C" int hl_cc_filter(const double *vol, const int *labels, const unsigned char *keep, int64_t n_voxels, int64_t n_labels, double iso,
                            double *out, void *stream) {
    HL_REQUIRE(vol && labels && out && n_voxels > 0 && n_voxels < (1LL << 31) && n_labels >= 0, "hl_cc_filter: bad argument");
    HL_REQUIRE(keep || n_labels == 0, "hl_cc_filter: null argument");
    hipLaunchKernelGGL(k_cc_filter, dim3(grid_of(n_voxels)), dim3(TPB), 0, (hipStream_t)stream, vol, labels, keep, (long)n_voxels, (long)n_labels, iso,
                       out);
    return hl::check_launch("hl_cc_filter");
}

extern "C" int hl_mesh_pack_points(const float *pts, const float *dirs, int64_t n_verts, float *pts4, float *dirs4, void *stream) {
    HL_REQUIRE(pts && dirs && pts4 && dirs4 && n_verts > 0, "hl_mesh_pack_points: bad argument");
    const long nv32 = (n_verts + 31) / 32 * 32;
    hipLaunchKernelGGL(k_mesh_pack, dim3(grid_of(nv32)), dim3(TPB), 0, (hipStream_t)stream, pts, dirs, (long)n_verts, nv32, (float4 *)pts4,
                       (float4 *)dirs4);
    return hl::check_launch("hl_mesh_pack_points");
}

extern "C" int hl_mesh_unpack_colors(const float *records, int64_t n_verts, float *rgb, unsigned char *rgb8, void *stream) {
    HL_REQUIRE(records && rgb && n_verts > 0, "hl_mesh_unpack_colors: bad argument");
    hipLaunchKernelGGL(k_mesh_colors, dim3(grid_of(n_verts)), dim3(TPB), 0, (hipStream_t)stream, (const float4 *)records, (long)n_verts, rgb, rgb8);
    return hl::check_launch("hl_mesh_unpack_colors");
}

extern "C" int hl_mc_max_triangles(void) { return HL_MC_MAX_TRI; }

extern "C" int hl_mc_case_table(signed char *h_tris, unsigned char *h_ntri) {
    HL_REQUIRE(h_tris && h_ntri, "hl_mc_case_table: null argument");
    memcpy(h_tris, HL_MC_TRIS, sizeof(HL_MC_TRIS));
    memcpy(h_ntri, HL_MC_NTRI, sizeof(HL_MC_NTRI));
    return HL_OK;
}
