// What the mesh stages (hl_mesh_simplify.hip, hl_mesh_distance.hip, hl_mesh_raster.hip, hl_mesh_animate.hip) share: the host arithmetic of
// their size checks and scratch layouts, and the device loads that never follow a bad index.  Each file keeps its own Layout, Grid and
// MeshIn.
#pragma once
#include "hl_common.h"

#include <cmath>
#include <cstdint>

namespace hl {

constexpr int kMeshThreads = 256;                   // the workgroup of every per-vertex and per-triangle kernel

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline int64_t blocks_of(int64_t n) { return (n + kMeshThreads - 1) / kMeshThreads; }
inline bool count_ok(int64_t n) { return n >= 1 && n <= 0x7fffffff; }

// extents -> number of cells, 0 when an extent is below 1 or the grid holds more than max_cells (<= 2^31: checked without overflow)
inline int64_t cells_of(int64_t gx, int64_t gy, int64_t gz, int64_t max_cells) {
    if (gx < 1 || gy < 1 || gz < 1 || gx > max_cells || gy > max_cells || gz > max_cells) return 0;
    if (gx * gy > max_cells) return 0;              // (<= 2^62)
    if (gx * gy * gz > max_cells) return 0;         // (<= 2^62)
    return gx * gy * gz;
}

inline bool finite_host(double x) { return fabs(x) < (double)INFINITY; }      // (false for NaN)
inline bool origin_ok(const double *o) { return o && finite_host(o[0]) && finite_host(o[1]) && finite_host(o[2]); }

#if defined(__HIPCC__)
__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return fabs(x) < (double)INFINITY && fabs(y) < (double)INFINITY && fabs(z) < (double)INFINITY;      // (false for NaN)
}

// the indices of triangle t, validated; false: an index outside [0, N), which the caller must not dereference.  (N by reference: a
// caller's kernel argument, read where it is compared - the order the stages' kernels were compiled in before they shared this.)
__device__ __forceinline__ bool load_indices(const int *triangles, int64_t t, const int64_t &N, int (&iv)[3]) {
    const int *tp = triangles + t * 3;
    iv[0] = tp[0], iv[1] = tp[1], iv[2] = tp[2];
    return iv[0] >= 0 && iv[1] >= 0 && iv[2] >= 0 && iv[0] < N && iv[1] < N && iv[2] < N;
}
#endif

}  // namespace hl
