// One pinhole view's ray of one pixel   [SynBodyView_datasets.py:316-329 get_rays, :370-403 get_near_far, :422-433]
// Shared by k_camera_rays (hl_render.hip: every pixel of a view) and k_ray_batch (hl_ray_batch.hip: the sampled pixels of a training
// batch), so that a sampled ray is bit for bit the ray of the view at that pixel.  float64 like the reference's numpy (K, R, T are
// float64 there), rounded to float32 exactly where sample_ray_batch casts.  Term order follows oracle/camera_oracle.py (no FMA
// contraction in this build).
// The reference runs get_near_far at two precisions, and the function has both (kTrain):
//   false  the split != 'train' branch of recon_NeRF/lib/if_nerf_data_utils.py (:173-178) and SynBodyView_datasets.py: the rays are
//          rounded to float32 first, the box test reads the rounded rays, |ray_d| is a float32 norm  - hl_camera_rays
//   true   the split == 'train' branch (:146-149, 163-167): the box test reads the float64 rays, everything is rounded afterwards
//          - hl_camera_rays_train, hl_ray_batch
// ray_o and ray_d are the same bits either way (but for a float64 direction component that is non-zero and rounds to zero: the
// float32 branch turns it into 1e-8, the float64 branch leaves the rounded 0, each as its reference does); near / far differ by a few ulp.
#pragma once
#include "hl_common.h"

namespace hl {

struct CamView {
    double Ki[9], R[9], T[3], o[3];   // inv(K), world->camera rotation, translation, camera centre -(R^T T)
    double b[6];                      // padded bounds: min xyz, max xyz
};
static_assert(sizeof(CamView) == HL_CAMERA_ROW * sizeof(double), "camera table row layout");

// host: the derived values of a view, computed once where both entry points agree on them
inline void cam_view_fill(const double *h_Kinv, const double *h_R, const double *h_T, const double *h_bounds, CamView &a) {
    for (int i = 0; i < 9; ++i) { a.Ki[i] = h_Kinv[i]; a.R[i] = h_R[i]; }
    for (int c = 0; c < 3; ++c) {
        a.T[c] = h_T[c];
        a.o[c] = -((h_R[0 * 3 + c] * h_T[0] + h_R[1 * 3 + c] * h_T[1]) + h_R[2 * 3 + c] * h_T[2]);
        a.b[c] = h_bounds[c] + -0.01;
        a.b[3 + c] = h_bounds[3 + c] + 0.01;
    }
}

#if defined(__HIPCC__)
// pixel (x, y) -> origin, direction (exact zeros become 1e-8, as get_near_far writes them into the caller's ray_d), near / far (0 / 1
// unless the ray crosses the padded box exactly twice); returns mask_at_box.
template <bool kTrain>
__device__ __forceinline__ bool camera_ray_pixel(const CamView &a, int px, int py, float of[3], float df[3], float &near, float &far) {
    const double x = (double)px, y = (double)py;
    double pc[3], q[3], d64[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pc[c] = (x * a.Ki[c * 3 + 0] + y * a.Ki[c * 3 + 1]) + a.Ki[c * 3 + 2];
        q[c] = pc[c] - a.T[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double pw = (q[0] * a.R[0 * 3 + c] + q[1] * a.R[1 * 3 + c]) + q[2] * a.R[2 * 3 + c];
        d64[c] = pw - a.o[c];
        if (kTrain && d64[c] == 0.0) d64[c] = 1e-8;
        df[c] = (float)d64[c];
        of[c] = (float)a.o[c];
        if (!kTrain && df[c] == 0.0f) df[c] = 1e-8f;   // get_near_far writes this into the caller's ray_d
    }
    const double o[3] = {kTrain ? a.o[0] : (double)of[0], kTrain ? a.o[1] : (double)of[1], kTrain ? a.o[2] : (double)of[2]};
    const double d[3] = {kTrain ? d64[0] : (double)df[0], kTrain ? d64[1] : (double)df[1], kTrain ? d64[2] : (double)df[2]};
    const double norm = kTrain ? sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                               : (double)sqrtf((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]);     // (:79 float64 / :395 float32 norm)
    const double eps = 1e-6;
    int cnt = 0;
    double d0 = 0.0, d1 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {   // min_x, min_y, min_z, max_x, max_y, max_z
        const int ax = k % 3;
        const double t = (a.b[k] - o[ax]) / d[ax];
        const double p0 = t * d[0] + o[0], p1 = t * d[1] + o[1], p2 = t * d[2] + o[2];
        const bool inside = p0 >= a.b[0] - eps && p0 <= a.b[3] + eps && p1 >= a.b[1] - eps && p1 <= a.b[4] + eps &&
                            p2 >= a.b[2] - eps && p2 <= a.b[5] + eps;
        if (inside) {
            const double e0 = p0 - o[0], e1 = p1 - o[1], e2 = p2 - o[2];
            const double r = sqrt((e0 * e0 + e1 * e1) + e2 * e2) / norm;
            if (cnt == 0) d0 = r;
            else if (cnt == 1) d1 = r;
            ++cnt;
        }
    }
    const bool hit = cnt == 2;
    near = hit ? (float)fmin(d0, d1) : 0.f;
    far = hit ? (float)fmax(d0, d1) : 1.f;
    return hit;
}
#endif

}  // namespace hl
