/*
 * humanliff_hip.h — C ABI of libhumanliff_hip.so (MI355X / gfx950 only).
 *
 * The reference (skhu101/HumanLiff) has no FFI layer: its boundary is the
 * Python API of two hot paths.  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference).  The Python
 * mirrors in humanliff_amd/ (same class / function names and argument
 * meaning as the reference) are thin callers of this ABI; INTEGRATION.md
 * shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named h_* (host);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - the library never allocates device memory: packed buffers and workspace
 *     are sized by *_bytes() and owned by the caller;
 *   - all calls are enqueue-only (no device synchronisation) and re-entrant
 *     per (device, stream);
 *   - return 0 on success, a negative hl_status on failure; the message is
 *     available (thread-local) from hl_last_error().
 */
#ifndef HUMANLIFF_HIP_H
#define HUMANLIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hl_status {
    HL_OK = 0,
    HL_ERR_INVALID = -1,   /* bad argument (the reference would `assert`)        */
    HL_ERR_UNSUPPORTED = -2, /* configuration outside what the kernels cover      */
    HL_ERR_RUNTIME = -3    /* HIP runtime error (launch failed, wrong device ...) */
} hl_status;

int hl_version(void);
const char *hl_last_error(void);

/* ------------------------------------------------------------------------
 * Path 2 — tri-plane NeRF volume renderer
 * ------------------------------------------------------------------------ */

/* Render-MLP parameters, in the reference's state_dict layout (row-major
 * (out,in) nn.Linear weights), human_diffusion/NeRF/renderer.py:29-39. */
typedef struct hl_render_mlp_params {
    const float *pts0_w, *pts0_b;   /* pts_linears.0   (128,27)  (128) */
    const float *pts1_w, *pts1_b;   /* pts_linears.1   (128,128) (128) */
    const float *pts2_w, *pts2_b;   /* pts_linears.2   (128,155) (128) */
    const float *feat_w, *feat_b;   /* feature_linear  (128,128) (128) */
    const float *alpha_w, *alpha_b; /* alpha_linear    (1,128)   (1)   */
    const float *views_w, *views_b; /* views_linear    (64,155)  (64)  */
    const float *rgb_w, *rgb_b;     /* rgb_linear      (3,64)    (3)   */
} hl_render_mlp_params;

/* Re-lay the MLP for the MFMA ray-march kernel (done once per checkpoint). */
size_t hl_render_mlp_packed_bytes(void);
int hl_render_mlp_pack(const hl_render_mlp_params *h_params, void *packed, void *stream);

/* Re-lay one subject's tri-plane (3,9,H,W) fp32 — the (1,3,9,H,W) tensor the
 * sampler script builds at scripts/triplane_sample_layered.py:158 — into the
 * texel-major layout the kernel gathers from (done once per subject). */
size_t hl_planes_packed_bytes(int H, int W);
int hl_planes_pack(const float *planes, int H, int W, void *packed, void *stream);

#define HL_RENDER_WHITE_BKGD 1u      /* renderer.py:224-225 (per-ray intent)            */
#define HL_RENDER_NORMALIZE_DEPTH 2u /* depth = (depth - near) / (far - near + 1e-5): NeRF/renderer.py:271, recon_NeRF/lib/renderer.py:288 */
#define HL_RENDER_REEVALUATE 4u      /* hl_render_rays: run the fine pass over all n_samples+n_importance depths like the reference
                                        (re-evaluating the coarse points) instead of evaluating every point once; same image */
#define HL_RENDER_CLAMP_DEPTH 8u     /* clamp the normalised depth to [0,1]: NeRF/renderer.py:272-274 - the human_diffusion twin only,
                                        recon_NeRF/lib/renderer.py leaves it unclamped */

#define HL_RENDER_MLP_FP16 16u       /* opt-in (hl_render_rays, evaluate-once pipeline): the MLP with fp16 operands / fp32 accumulation
                                        (k_march16, all weights LDS-resident); features, encodings, softplus, compositing stay fp32 */
#define HL_RENDER_MLP_BF16X3 32u     /* hl_render_rays, evaluate-once pipeline: every fp32 product of the MLP (renderer.py:134-156) formed from an
                                        EXACT three-way bf16 split of both operands - six partial products on v_mfma_f32_32x32x16_bf16, fp32
                                        accumulation, dropped terms < 2^-24 |a b| (k_march_plw<3>); an fp32-tolerance mode, not a reduced-precision one */

#define HL_RENDER_MLP_FP16X2 64u     /* the same pipeline with TWO fp16 planes per operand (activations x = h0 + h1 to 2^-20 |x| while 2^-3 <= |x| < 65504, absolute 2^-24
                                        below; weights: every layer's planes are those of 2^k W with max |2^k W| in [2^12, 2^13) - nearest-even, 2^-22 of the layer's
                                        largest weight WHATEVER its magnitude (round 6; the accumulators are multiplied by 2^-k on their way into the softplus) - and
                                        the three partial products h0 w0 + h0 w1 + h1 w0 on v_mfma_f32_32x32x16_f16, fp32 accumulation (k_march_plw<2>): half the
                                        matrix instructions of BF16X3 at the same fp32-class error against the reference's renders (goldens a ... f: weights from
                                        2^-8 below to 2^4 above nn.Linear's initialisation); softplus returns x beyond a pre-activation of 88.7 like F.softplus */

#define HL_RENDER_FOUR_LAUNCH 128u    /* hl_render_rays: keep rounds 2-5's schedule of the evaluate-once pipeline - evaluate, k_importance, evaluate, k_composite, with the raw
                                        records of BOTH halves through HBM.  Default (round 6, HL_RENDER_MLP_FP16X2, n_samples <= 128, linspace depths): TWO
                                        launches per view - the coarse evaluate, then the one-pass fine launch (k_march_plw<., false, true>): the wave that owns 32
                                        rays draws their importance depths from the coarse records (renderer.py:158-170, 533-563), evaluates them and composites
                                        coarse + new samples in depth order as it goes (renderer.py:172-231, 252-253); bit-identical images */

size_t hl_render_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);
/* Byte offset, inside that workspace, of the sorted new depths of the evaluate-once schedules (tile-major [ceil(R/32)][n_importance][32],
 * behind the raw records of the coarse and the new points); 0 where the workspace holds nothing (no rays, n_importance <= 0).  Host arithmetic. */
size_t hl_render_workspace_new_depths_offset(int64_t n_rays, int n_samples, int n_importance);

/* Replaces Renderer.render (human_diffusion/NeRF/renderer.py:234-281,
 * recon_NeRF/lib/renderer.py:244-291) together with the per-chunk body of
 * render() (scripts/triplane_sample_layered.py:262-279,
 * recon_NeRF/run_nerf_batch.py:41-58) for use_canonical_space=False, test mode.
 *
 *   bounds   (2,3)   tp_input['world_bounds'][b]
 *   rays_o/d (R,3)   near/far (R)
 *   z_vals   (R,n_samples) or NULL -> near*(1-t)+far*t, t = linspace(0,1,n_samples)
 *   u        (R,n_importance) uniform draws of sample_pdf (renderer.py:545); required
 *            when n_importance > 0 (n_importance must then equal n_samples, renderer.py:250)
 *   rgb (R,3)  acc (R)  depth (R)   outputs; normal_map == rgb_map in the reference
 *   workspace  hl_render_workspace_bytes(); scratch, tile-major [ceil(R/32)][sample][32 rays] (ray r = tile r/32, lane r%32: one
 *            line per wave and sample instead of 4-byte accesses at a row stride): the raw (sigma, r, g, b) records of the
 *            n_samples coarse and the n_importance new points and the sorted new depths - every point is evaluated ONCE with the
 *            full MLP and a merge kernel composites them in depth order (the reference re-evaluates the coarse points in its
 *            fine pass; the outputs are bit-identical, HL_RENDER_REEVALUATE selects that schedule)
 */
int hl_render_rays(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds,
                   const float *rays_o, const float *rays_d, const float *near, const float *far,
                   const float *z_vals, const float *u, int64_t n_rays, int n_samples, int n_importance,
                   unsigned flags, float *rgb, float *acc, float *depth, void *workspace, void *stream);
/* hl_render_rays whose `u` is still being written on another stream (hl_mt19937_uniform): u_ready_event (hipEvent_t, recorded behind that
 * writer; NULL = none) is waited for in front of the importance-sampling launch only, so the coarse evaluate pass overlaps the generator. */
int hl_render_rays_u_event(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds,
                   const float *rays_o, const float *rays_d, const float *near, const float *far,
                   const float *z_vals, const float *u, void *u_ready_event, int64_t n_rays, int n_samples, int n_importance,
                   unsigned flags, float *rgb, float *acc, float *depth, void *workspace, void *stream);

/* The three stages of hl_render_rays, exposed for tests and profiling.  sigma_out / sigma and z_all_out /
 * z_all use the tile-major workspace layout described above (buffers sized for ceil(R/32)*32 rays);
 * hl_render_fine takes z_all either tile-major (z_tiled = 1) or as caller rows (R,S) (z_tiled = 0). */
int hl_render_coarse(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds,
                     const float *rays_o, const float *rays_d, const float *near, const float *far,
                     const float *z_vals, int64_t n_rays, int n_samples, float *sigma_out, void *stream);
int hl_render_importance(const float *sigma, const float *rays_d, const float *near, const float *far,
                         const float *z_vals, const float *u, int64_t n_rays, int n_samples, int n_importance,
                         float *z_all_out, void *stream);
/* The stages of the default (evaluate-once) schedule of hl_render_rays.  A "record" is the raw network output of one sample
 * point, float[4] = (sigma, r, g, b) before softplus / sigmoid; record and depth arrays are tile-major [ceil(R/32)][samples][32].
 *   hl_render_eval            full MLP at every given depth (z: NULL -> linspace, caller rows (R,S) with z_tiled = 0, or tile-major
 *                             with z_tiled = 1) -> records_out
 *   hl_render_importance_new  sample_pdf on the coarse records' densities (renderer.py:158-170, 533-563) -> the n_importance NEW
 *                             depths only, sorted (the reference sorts the union, :252-253; hl_render_composite merges instead)
 *   hl_render_composite       merge the coarse and the new depths and alpha-composite their records in depth order (:172-231) */
int hl_render_eval(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds, const float *rays_o,
                   const float *rays_d, const float *near, const float *far, const float *z, int z_tiled, int64_t n_rays,
                   int n_samples, float *records_out, void *stream);
/* hl_render_eval with the product mode of hl_render_rays: flags = 0 (fp32 MFMA), HL_RENDER_MLP_BF16X3 or HL_RENDER_MLP_FP16 */
int hl_render_eval_products(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds, const float *rays_o,
                            const float *rays_d, const float *near, const float *far, const float *z, int z_tiled, int64_t n_rays,
                            int n_samples, unsigned flags, float *records_out, void *stream);
int hl_render_importance_new(const float *records, const float *rays_d, const float *near, const float *far, const float *z_vals,
                             const float *u, int64_t n_rays, int n_samples, int n_importance, float *z_new_out, void *stream);
/* Rays a wave of k_importance walks one after the other in a call of hl_render_importance / hl_render_importance_new with n_rays rays (host
 * arithmetic; both entries launch with the same function): 8 = one workgroup per 32-ray tile, from 1024 tiles; 4 from 512 tiles, 2 from 256,
 * 1 below (the tile is spread over 2, 4, 8 workgroups).  HL_ERR_INVALID for n_rays <= 0. */
int hl_render_importance_plan(int64_t n_rays);
int hl_render_composite(const float *near, const float *far, const float *z_vals /* coarse rows or NULL */, const float *z_new,
                        const float *rec_coarse, const float *rec_new, int64_t n_rays, int n_samples, int n_importance,
                        unsigned flags, float *rgb, float *acc, float *depth, void *stream);
int hl_render_fine(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds,
                   const float *rays_o, const float *rays_d, const float *near, const float *far,
                   const float *z_all /* or NULL -> linspace */, int z_tiled, int64_t n_rays, int n_total_samples,
                   unsigned flags, float *rgb, float *acc, float *depth, void *stream);

/* Training of the renderer: forward with saved activations + backward of the evaluate-once schedule, for
 * the tri-plane fitting loop (recon_NeRF/run_nerf_batch.py:236-265: render -> img/acc loss -> backward -> Adam) and any other loss
 * on rgb_map / acc_map of Renderer.render with test=False (human_diffusion/NeRF/renderer.py:172-281).  The importance depths are
 * drawn under no_grad in the reference (:243-253), so gradients flow through the evaluation of the 2N sample points and the
 * compositing only.  Matrices are "row = unit, column = sample point" (point order: the pass's tile-major record order at column
 * offset *_off), row stride *_stride floats, hl_render_train_rows() rows:
 *   activations (630 rows): [0,27) tri-plane features | [27,155) softplus(pts_linears.1) | [155,283) softplus(pts_linears.0) |
 *                           [283,411) softplus(pts_linears.2) | [411,539) feature_linear | [539,566) view encoding |
 *                           [566,630) softplus(views_linear)
 *   deltas (634 rows, dL/d pre-activation): [0,128) pts_linears.0 | [128,256) pts_linears.1 | [256,384) pts_linears.2 |
 *                           [384,512) feature_linear | [512,576) views_linear | 576 alpha_linear | [577,580) rgb_linear |
 *                           [580,607) dL/d tri-plane features | [607,634) the same, ray-major (written by hl_render_plane_grads*,
 *                           which therefore take `del` as scratch although it is declared const)
 * so that every weight gradient is one product delta_rows x activation_rows^T over the sample points (e.g. pts_linears.2.weight =
 * deltas[256:384] x activations[0:155]^T) and every bias gradient a row sum: hl_render_weight_grads.
 *   hl_render_composite_noise     hl_render_composite with `noise` (R, n_samples+n_importance) added to the raw density of sorted
 *                                 sample s of each ray (renderer.py:212, randn_like in training mode); NULL = none
 *   hl_render_eval_acts           hl_render_eval that also writes the activation matrix; round 5: on the fp16x2 kernel of the inference default
 *                                 (k_march_plw<2, ACTS>: fp32 products from two fp16 planes per operand, softplus in the log2 domain, activations stored in
 *                                 natural units) - 0.38 -> 0.20 ms per 2 048 rays x 128 samples; gradient tests unchanged
 *   hl_render_composite_backward  g_rgb (R,3), g_acc (R) -> d_records of both passes (float[4] = d/d(sigma, r, g, b) raw, record
 *                                 layout; zero on padding rays) and rows 576..579 of the delta matrix `del` (columns: coarse pass,
 *                                 then the new depths); scratch: hl_render_composite_backward_scratch_bytes()
 *   hl_render_mlp_backward        one pass's d_records + activations -> its columns of the delta matrix; round 5: the five transposed-weight products with fp16x2
 *                                 operands (weights as two fp16 planes behind the fp32 image of hl_render_mlp_pack_bwd; delta tiles split in registers, scaled per ray
 *                                 and sample by a power of two into fp16's range and scaled back exactly): 0.39 -> 0.27 ms per pass; gradient bounds unchanged
 *   hl_render_plane_grads         feature deltas of both passes -> d_planes (27,H,W), overwritten: the transposed bilinear lookup;
 *                                 each workgroup owns a tile of texels and accumulates in LDS (no global atomics) in 64-bit FIXED
 *                                 POINT whose unit comes from the largest |delta| of the call: integer additions commute, so the
 *                                 result is the same bits on every run (round 5; rounding per contribution 2^-43 of that maximum
 *                                 or finer); a delta that is not finite makes the output NaN.
 *                                 scratch: hl_render_plane_grads_scratch_bytes()
 *   hl_render_mlp_pack_bwd        transposed weights for hl_render_mlp_backward (redo after every optimizer step, like
 *                                 hl_render_mlp_pack)
 *   hl_render_weight_grads        all 14 parameter gradients from the two matrices over n_cols sample points (multiple of 32), ADDED
 *                                 to the tensors of `grads` (PyTorch layouts, zero them first); fp32 products from exact
 *                                 three-way bf16 splits of both operands, fp32 accumulation (k_wgrad).  The 256 point ranges
 *                                 write their partial results to `scratch` (hl_render_weight_grads_scratch_bytes(n_cols)) and
 *                                 k_wgrad_finish sums them in a fixed order: the same bits on every run (round 5; before: float
 *                                 atomics) */
/* Canonical-space training (use_canonical_space=True with test=False; README.md:123 TightCap fitting): the deformation has no
 * parameters and the points get no gradient, so the backward is the one above with two substitutions -
 *   hl_render_eval_points_acts     hl_render_eval_points that also writes the activation matrix (forward, per pass)
 *   hl_render_plane_grads_points   hl_render_plane_grads for sample points that are not on straight rays in tri-plane space:
 *                                  pts_coarse / pts_new are the canonical points hl_deform_rays wrote for the two passes, `bounds`
 *                                  is tp_input['t_world_bounds']; scratch: hl_render_plane_grads_points_scratch_bytes() */
int hl_render_eval_points_acts(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds, const float *pts_c,
                               const float *dirs_c, int64_t n_rays, int n_samples, float *records_out, float *act, int64_t act_stride,
                               int64_t act_off, void *stream);
size_t hl_render_plane_grads_points_scratch_bytes(int64_t n_rays, int n_samples, int n_importance);
int hl_render_plane_grads_points(int H, int W, const float *bounds, const float *pts_coarse, const float *pts_new, int64_t n_rays,
                                 int n_samples, int n_importance, const float *del, int64_t del_stride, float *d_planes, void *scratch,
                                 void *stream);
typedef struct hl_render_mlp_grads {
    float *pts0_w, *pts0_b, *pts1_w, *pts1_b, *pts2_w, *pts2_b, *feat_w, *feat_b, *alpha_w, *alpha_b, *views_w, *views_b, *rgb_w,
        *rgb_b;   /* same order and shapes as hl_render_mlp_params */
} hl_render_mlp_grads;
size_t hl_render_weight_grads_scratch_bytes(int64_t n_cols);
int hl_render_weight_grads(const float *del, int64_t del_stride, const float *act, int64_t act_stride, int64_t n_cols,
                           const hl_render_mlp_grads *grads, void *scratch, void *stream);
int hl_render_composite_noise(const float *near, const float *far, const float *z_vals, const float *z_new, const float *rec_coarse,
                              const float *rec_new, const float *noise, int64_t n_rays, int n_samples, int n_importance,
                              unsigned flags, float *rgb, float *acc, float *depth, void *stream);
/* The kernel a compositing call launches (host arithmetic, no HIP call; the entries take their branch from the same functions):
 * hl_render_composite_plan for hl_render_composite (with_noise = 0) and hl_render_composite_noise (with_noise = whether `noise` is
 * given), hl_render_composite_backward_plan for hl_render_composite_backward.  HL_ERR_INVALID for sizes the entries refuse. */
#define HL_COMPOSITE_SERIAL_RAW 1   /* k_composite, a thread per ray, the raw exp2 / log2 / rcp forms of the inference paths */
#define HL_COMPOSITE_WAVE_FWD 2     /* k_composite_wave<false>, a wave per ray: noise given, n_rays <= 65536, both sample counts <= 256 */
#define HL_COMPOSITE_SERIAL_EXACT 3 /* k_composite with noise: the exact expf / log1pf forms the backward differentiates */
#define HL_COMPOSITE_WAVE_BWD 4     /* k_composite_wave<true>: both sample counts <= 256 */
#define HL_COMPOSITE_SERIAL_BWD 5   /* k_composite_bwd, a thread per ray */
int hl_render_composite_plan(int64_t n_rays, int n_samples, int n_importance, int with_noise);
int hl_render_composite_backward_plan(int n_samples, int n_importance);
size_t hl_render_mlp_bwd_packed_bytes(void);
int hl_render_mlp_pack_bwd(const hl_render_mlp_params *h_params, void *packed_bwd, void *stream);
void hl_render_train_rows(int *act_rows, int *del_rows);
int hl_render_eval_acts(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds, const float *rays_o,
                        const float *rays_d, const float *near, const float *far, const float *z, int z_tiled, int64_t n_rays,
                        int n_samples, float *records_out, float *act, int64_t act_stride, int64_t act_off, void *stream);
size_t hl_render_composite_backward_scratch_bytes(int64_t n_rays, int n_samples, int n_importance);
int hl_render_composite_backward(const float *near, const float *far, const float *z_vals, const float *z_new,
                                 const float *rec_coarse, const float *rec_new, const float *noise, const float *g_rgb,
                                 const float *g_acc, int64_t n_rays, int n_samples, int n_importance, unsigned flags,
                                 float *d_rec_coarse, float *d_rec_new, float *del, int64_t del_stride, void *scratch,
                                 void *stream);
int hl_render_mlp_backward(const void *mlp_packed, const void *mlp_bwd_packed, int H, int W, const float *bounds,
                           const float *rays_o, const float *rays_d, const float *near, const float *far, const float *z,
                           int z_tiled, int64_t n_rays, int n_samples, const float *d_records, const float *act,
                           int64_t act_stride, int64_t act_off, float *del, int64_t del_stride, int64_t del_off, void *stream);
int hl_render_plane_grads(int H, int W, const float *bounds, const float *rays_o, const float *rays_d, const float *near,
                          const float *far, const float *z_vals /* coarse rows or NULL */, const float *z_new,
                          int z_new_rows /* 1: rows (R, n_importance), faster; 0: tile-major as hl_render_importance_new wrote them */,
                          int64_t n_rays, int n_samples, int n_importance, const float *del, int64_t del_stride, float *d_planes,
                          void *scratch, void *stream);
size_t hl_render_plane_grads_scratch_bytes(int64_t n_rays);

/* Per-view ray generation on the device.  Replaces get_rays
 * (human_diffusion/SynBodyView_datasets.py:316-329), the float32 casts and the near=0 / far=1 fill of
 * sample_ray_batch (:422-433) and get_near_far (:370-403) for one pinhole camera: float64 arithmetic like the
 * reference's numpy, rounded to float32 where the reference casts.  h_Kinv = inv(K) (3,3), h_R (3,3) world->camera,
 * h_T (3), h_bounds (2,3) are HOST float64 arrays copied into the launch; outputs are device arrays of H*W rays in
 * row-major pixel order: rays_o, rays_d (R,3) (exact zeros of rays_d become 1e-8 as in the reference), near, far (R),
 * mask_at_box (R) bytes or NULL. */
int hl_camera_rays(const double *h_Kinv, const double *h_R, const double *h_T, const double *h_bounds, int H, int W,
                   float *rays_o, float *rays_d, float *near, float *far, unsigned char *mask_at_box, void *stream);
/* The same view in the arithmetic of the reference's TRAINING split (recon_NeRF/lib/if_nerf_data_utils.py:146-149, 163-167): get_near_far
 * runs on the float64 rays (float64 |ray_d|, an exact float64 zero of ray_d becomes 1e-8) and everything is rounded to float32
 * afterwards, where hl_camera_rays - like the reference's test split and SynBodyView_datasets.py - rounds the rays first.  Same
 * arguments; rays_o / rays_d are the same bits, near / far differ by a few float32 ulp.  This is what hl_ray_batch writes per sampled pixel. */
int hl_camera_rays_train(const double *h_Kinv, const double *h_R, const double *h_T, const double *h_bounds, int H, int W,
                         float *rays_o, float *rays_d, float *near, float *far, unsigned char *mask_at_box, void *stream);

/* Canonical-space deformation of query points.  Replaces Renderer.deform_target2c /
 * deform_target2c_op (human_diffusion/NeRF/renderer.py:52-132, recon_NeRF/lib/renderer.py:60-140) including the external
 * pytorch3d knn_points(K=1): world -> SMPL space with h_R (3,3) / h_Th (3) (host float32), brute-force nearest body vertex among
 * verts_smpl4 (V,4: xyz of (vertices - Th) R, w ignored), then the per-vertex row of `table` (V,36: t[3] Rinv[9] pose_off[3]
 * shape_off[3] pose_off_big[3] Rbig[9] tbig[3] pad[3], built by humanliff_amd.NeRF.deform.deform_tables) applied in the
 * reference's order.  pts / dirs (P,3) device, dirs may be NULL; outputs can_pts, can_dirs (P,3), vertex_ids (P) or NULL. */
int hl_deform_points(const float *pts, const float *dirs, const float *h_R, const float *h_Th, const float *verts_smpl4,
                     const float *table, int n_vertices, int64_t n_points, float *can_pts, float *can_dirs, int *vertex_ids,
                     void *stream);
/* Rendering in canonical space (use_canonical_space=True, renderer.py:114-132, 192-201, 242-246): the stages and the driver.
 *   hl_deform_rays             sample points o + d*z of every ray (z as in hl_render_eval) and its unit direction, deformed like
 *                              hl_deform_points -> pts_c, dirs_c: float[4] per sample (xyz, w unused), tile-major [ceil(R/32)][S][32]
 *   hl_render_eval_points      hl_render_eval on given canonical points / directions; `bounds` is tp_input['t_world_bounds']
 *   hl_render_rays_canonical   evaluate-once schedule of hl_render_rays with the two stages above in front of each evaluate pass;
 *                              workspace: hl_render_canonical_workspace_bytes() */
int hl_deform_rays(const float *rays_o, const float *rays_d, const float *near, const float *far, const float *z, int z_tiled,
                   int64_t n_rays, int n_samples, const float *h_R, const float *h_Th, const float *verts_smpl4, const float *table,
                   int n_vertices, float *pts_c, float *dirs_c, void *scratch /* 8 bytes of device memory (work counter) */, void *stream);
int hl_render_eval_points(const void *mlp_packed, const void *planes_packed, int H, int W, const float *bounds, const float *pts_c,
                          const float *dirs_c, int64_t n_rays, int n_samples, float *records_out, void *stream);
size_t hl_render_canonical_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);
int hl_render_rays_canonical(const void *mlp_packed, const void *planes_packed, int H, int W, const float *t_bounds,
                             const float *rays_o, const float *rays_d, const float *near, const float *far, const float *z_vals,
                             const float *u, int64_t n_rays, int n_samples, int n_importance, unsigned flags, const float *h_R,
                             const float *h_Th, const float *verts_smpl4, const float *table, int n_vertices, float *rgb, float *acc,
                             float *depth, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * Path 1 — tri-plane UNet denoiser + Gaussian-diffusion sampler update
 * ------------------------------------------------------------------------ */

/* Architecture hyper-parameters, as UNetModel.__init__ receives them
 * (human_diffusion/improved_diffusion/unet.py:323-343, built by script_util.py:98-150).
 * Supported: dims=2, use_scale_shift_norm True or False, cond_type="controlnet", "AdaGN", "cross_attention", "concat" (a wider in_channels) or "", dropout=0,
 * conv_resample=True; use_3d_aware False (the shipped configuration) or True (not with AdaGN). */
typedef struct hl_unet_cfg {
    int in_channels, model_channels, out_channels, num_res_blocks;
    int n_levels;
    int channel_mult[8];
    int n_attention_ds;
    int attention_ds[8];        /* downsample rates at which attention is inserted */
    int num_heads, num_heads_upsample;
    int num_classes;            /* 0: not class conditional */
    int controlnet;             /* 1: cond_type == "controlnet" */
    int adagn;                  /* 1: cond_type == "AdaGN" (x_cond projected to one more summand of the timestep embedding) */
    int cross_attn;             /* 1: cond_type == "cross_attention": SpatialTransformer blocks (spatial_transformer.py, depth 1) in place of the
                                 * AttentionBlocks, attending to one context token per image = the AdaGN projection of x_cond */
    int aware3d;                /* 1: use_3d_aware: x, x_cond and the output are (B, 3*in_channels, H, W) tri-planes; the network runs on
                                 * the three planes side by side, (B, in_channels, H, 3W), and every ResBlock of the main towers feeds
                                 * each plane the axis means of the other two (unet.py:208-214, 566-570, 613-614) */
    int no_scale_shift;         /* 1: use_scale_shift_norm=False (unet.py:216-218): emb_layers emits C values that are ADDED to the first
                                 * convolution's output before out_layers' GroupNorm, instead of 2C values that scale and shift its result */
} hl_unet_cfg;

/* Bytes of the re-laid weights (conv OIHW -> GEMM-ready rows, emb_layers stacked). */
size_t hl_unet_packed_bytes(const hl_unet_cfg *cfg);

/* Bind a state_dict (the reference's key names) and pack it.
 * names/ptrs/numels: n_tensors parallel arrays; ptrs are device fp32 tensors in the
 * reference layouts (Conv2d OIHW, Conv1d (O,I,1), Linear (O,I)).  GroupNorm affine, biases
 * and label_emb are used in place (the caller keeps them alive); everything else is copied
 * into `packed`.  Replaces UNetModel.__init__ + load_state_dict for inference. */
int hl_unet_create(const hl_unet_cfg *cfg, int n_tensors, const char *const *names, const void *const *ptrs,
                   const int64_t *numels, void *packed, void *stream, void **handle);
void hl_unet_destroy(void *handle);

size_t hl_unet_workspace_bytes(void *handle, int B, int H, int W);

/* Replaces UNetModel.forward(x, timesteps, x_cond, y) (unet.py:550-615).
 * x, x_cond, out: (B, C, H, W) fp32 NCHW; t, y: (B) int64 (y NULL if not class conditional,
 * x_cond NULL only without controlnet).  t holds ORIGINAL-schedule integer timesteps
 * (respace.py:117-122 with rescale_timesteps=False); t_float, if non-NULL, overrides it with
 * fractional timesteps (rescale_timesteps=True). */
int hl_unet_forward(void *handle, const float *x, const int64_t *t, const float *t_float, const float *x_cond,
                    const int64_t *y, float *out, int B, int H, int W, void *workspace, void *stream);

/* The control encoder (input_blocks_cond) is independent of the main encoder up to the skip sums; by default
 * hl_unet_forward runs it on an internal second HIP stream, forked from and joined back into the caller's
 * stream with events (the low-resolution layers of the two branches then fill the chip together).
 * enable = 0 issues everything on the caller's stream. */
int hl_unet_set_overlap(void *handle, int enable);

/* Arithmetic of the large convolutions - all modes keep fp32 tensors and fp32 accumulators.
 * HL_CONV_FP32 (default): fp32-class products, fp32 accumulation.  3x3 / stride-1 layers take Winograd F(4x4,3x3) on v_mfma_f32_32x32x2_f32 (36 fp32
 *   multiplies per 4x4 outputs instead of 144; interpolation points 0, +-3/4, +-3/2, inf) where 32x16-pixel x 32-channel
 *   workgroups fill the chip (the 256- and 128-pixel levels at batch 4), Winograd F(2x2,3x3) (16 per 2x2 instead of 36) on the
 *   smaller levels, everything else the direct implicit GEMM.  Round 5: every 3x3 / stride-1 layer (also behind the nearest-x2 upsample) and every
 *   1x1 / stride-1 layer with Cout a multiple of 192, Cin a multiple of 32 / 96 and enough work (3x3: from 8 workgroups' worth of 256 pixels x 192
 *   channels, split-K below 100; 1x1: from 12) is a DIRECT convolution whose fp32 products come from TWO fp16 planes per operand on
 *   v_mfma_f32_32x32x16_f16 (k_conv_h2s, k_conv1_h2s: 8x16-pixel / 128-pixel tiles, two workgroups per CU): activation x = h0 + h1 (h0 = the nearest
 *   fp16, h1 = the nearest fp16 of the residual: |x - h0 - h1| <= 2^-23 |x| while both planes are normal), weight planes nearest even,
 *   h1 w0 + h0 w1 + h0 w0 accumulated in fp32.  Round 6 - the planes are SCALE-INVARIANT: every output channel's weights are multiplied by the power of
 *   two that puts the channel's largest |w| into [2^13, 2^14) before the split (2^-22 of it whatever the magnitude: zero_module convolutions at 1e-4,
 *   unet.py:149, lose nothing), and the staged input by the power of two sx with |x| sx <= 32752 - from sqrt(sum x^2) of the tensor (the group totals
 *   its producers left; the single-op entry points form them) for a raw input, from max|gamma'| sqrt(n_group) + max|beta'| behind a fused GroupNorm -
 *   so no plane overflows or goes subnormal where the magnitude is known; both scales leave in the epilogue (powers of two: exact).  Unknown magnitude
 *   (a GroupNorm given as coefficient arrays, the attention output in front of proj_out): sx = 1, and a value beyond fp16's range becomes inf / NaN
 *   (round 5 saturated silently).  Error of the fp32 direct kernel's class at EVERY scale, checked against float64 with weights x 2^0 ... 2^-18 and
 *   activations x 2^-10 ... 2^10 (tests/test_unet_gpu.py::test_conv_fp16x2_products_are_scale_invariant: rel-L2 2.2e-7 ... 6.4e-7 against 2.0e-7 ...
 *   7.3e-7 of HL_CONV_FP32_DIRECT, bit-identical across the scales).  A GroupNorm (+ SiLU) in front of such a layer is applied
 *   while the kernel stages its input (no pass over the tensor).  The F(4x4,3x3) / F(2x2,3x3) kernels keep the layers the direct kernels do not
 *   take (the 27-channel input convolution, Cout not a multiple of 192, small single-op calls).
 * HL_CONV_FP32_MFMA: HL_CONV_FP32 without those two kernels - every product on v_mfma_f32_32x32x2_f32 (the default of rounds 3-4).
 * HL_CONV_FP32_F23: the same without F(4x4,3x3) (the arithmetic of the round-2 library).
 * HL_CONV_FP32_DIRECT: the direct implicit GEMM only - every product of the reference's sum is formed exactly once.
 * HL_CONV_BF16X3 (opt-in, direct only): each product a*b is formed on the bf16 matrix pipe from exact three-way splits
 *   a = ah+am+al, b = bh+bm+bl (8 significand bits per bf16 plane) as ah*bh + ah*bm + am*bh + ah*bl + am*bm + al*bh; the three
 *   dropped terms are <= 3*2^-24 |a*b|, the size of one fp32 rounding.
 * The modes are not bit-identical to each other; all meet the same parity bounds (tests/test_unet_gpu.py,
 * tests/test_fullsize_gpu.py: production UNet vs the CPU oracle about 5e-6 max-abs on O(0.5) outputs in every mode; against the direct mode the F(4x4) mode differs
 * by 7.9e-6 max-abs / 1.4e-6 rms, the F(2x2) mode by 6.4e-6 / 1.0e-6).
 * Only layers with Cout a multiple of 96 (the DMA tile) are affected. */
#define HL_CONV_FP32 0
#define HL_CONV_BF16X3 1
#define HL_CONV_FP32_DIRECT 2
#define HL_CONV_FP32_F23 3
/* HL_CONV_BF16 (opt-in, direct only): 16-bit MFMA arithmetic for the TRAINING path - what the reference's train scripts select with
 *   --use_amp True (train_util.py:214 autocast): every activation is rounded to bf16 (nearest even) and multiplied with the weight's two
 *   leading bf16 planes (16 significand bits), fp32 accumulation on v_mfma_f32_32x32x16_bf16; tensors stay fp32 in HBM, master weights
 *   fp32.  Relative error per product <= 2^-9; NOT an inference default.  Forward (hl_conv2d_nhwc_mode) and backward-data
 *   (hl_conv2d_nhwc_bwd_data) take it; weight gradients stay fp32. */
#define HL_CONV_BF16 4
/* HL_CONV_FP16 (opt-in): fp16 operands / fp32 accumulation (v_mfma_f32_32x32x16_f16) on the 3x3 / stride-1 layers (k_conv_h16, also behind a nearest-x2 upsample) and the 1x1 layers (k_conv1_h16) - the
 * operand precision of the reference's own convolutions on its hardware (TF32: 10 explicit significand bits) and of its autocast training;
 * every other layer as HL_CONV_FP32.  HL_CONV_BF16 takes the same kernel with bf16 operands on those layers. */
#define HL_CONV_FP16 5
#define HL_CONV_FP32_MFMA 6
int hl_unet_set_conv_mode(void *handle, int mode);

/* Instrumentation for the roofline measurement (bench.py): with profiling enabled every kernel launch
 * of hl_unet_forward is bracketed by HIP events on the caller's stream.  hl_unet_profile_read waits for
 * them and returns, per category {0 conv/GEMM, 1 GroupNorm, 2 attention, 3 embeddings+prep}, the summed
 * kernel time (ms), the algorithmic FLOPs (2*MAC) and the launch count since the last read (host arrays
 * of 4).  Not meant for the timed production path. */
int hl_unet_profile(void *handle, int enable);
int hl_unet_profile_read(void *handle, double *h_ms, double *h_flops, int64_t *h_launches);
/* same, plus the FLOPs the kernels actually issued to the matrix pipe (h_exec_flops, may be NULL): Winograd layers issue
 * 16/36 of their algorithmic multiplies, HL_CONV_BF16X3 layers six bf16 products per fp32 product. */
int hl_unet_profile_read_ex(void *handle, double *h_ms, double *h_flops, double *h_exec_flops, int64_t *h_launches);

/* The convolution shape that took the most time in the spans of the last hl_unet_profile_read(_ex): h_vals = {total ms over its launches,
 * algorithmic FLOPs per launch, FLOPs issued to the matrix pipe per launch, number of launches} (averages over the launches of the shape),
 * h_key = {kernel family (as in hl_unet_dispatch_census), resolution level, 1 if behind a nearest-x2 upsample, Cout, kernel size} - the grouping
 * of a rocprofv3 per-kernel, per-grid row (layers that differ only in the input channel count share it).  The time is the convolution kernel's own (an event behind the
 * GroupNorm pre-pass k_gn_apply(_blk) separates the two; a split-K finish pass, where there is one, is included). */
int hl_unet_profile_dominant(void *handle, double *h_vals, int *h_key);

/* Which kernel family every convolution of the LAST hl_unet_forward took: h_counts[path * 8 + level] launches, path 0 = direct
 * implicit GEMM (k_conv_dma / k_conv), 1 = Winograd F(2x2,3x3) (k_conv_wino), 2 = bf16x3 emulation (k_conv_bf3), 3 = Winograd F(4x4,3x3)
 * (k_conv_wino4); level = log2(H / H_out) of the layer's output.  Kernel selection depends on the batch size (a layer takes a Winograd
 * kernel only where its workgroups fill the chip), so parity tests use this to state WHICH dispatch they covered. */
int hl_unet_dispatch_census(void *handle, int64_t *h_counts);
/* The same with `rows` <= 5 rows of 8 levels: direct | Winograd F(2x2) | bf16x3 / 16-bit operand kernels | Winograd F(4x4) | the direct convolutions of the
 * default mode with fp16x2 products (k_conv_h2s, k_conv1_h2s: two fp16 planes per operand, three partial products, fp32 accumulation). */
int hl_unet_dispatch_census_ex(void *handle, int64_t *h_counts, int rows);

/* Fused sampler update (everything after the model call in p_sample / ddim_sample,
 * gaussian_diffusion.py:293-333, 356-388, 484-529) for EPSILON prediction with a fixed
 * variance.  coef: (T, 8) fp32 per-kept-timestep table built by the host mirror from the
 * float64 schedule: [sqrt_recip_acp, sqrt_recipm1_acp, c0, c1, c2, 1/coef1, coef2/coef1, 0] (coef1/2 = posterior_mean_coef1/2) where
 *   mode 0 (p_sample):  x0 = clip(r*x - rm1*eps); sample = (c0*x0 + c1*x) + (t!=0) * c2 * noise
 *   mode 1 (ddim):      x0 = clip(r*x - rm1*eps); e = (r*x - x0)/rm1;
 *                       sample = (x0*c0 + c1*e) + (t!=0) * c2 * noise
 *   mode 2 / 3:         as 0 / 1 with `eps` holding the already processed pred_xstart (the caller applied denoised_fn and the
 *                       clamp, gaussian_diffusion.py:293-299); `clip` is ignored
 *   mode 4 / 5:         x_{t-1} prediction (ModelMeanType.PREVIOUS_X, :300-304, 335-343): `eps` holds the model's x_{t-1}; x0 = clip(eps/coef1 -
 *                       coef2/coef1 * x); mode 4: sample = eps + noise term (the prediction is the mean); mode 5: the ddim update from x0
 *   log_variance:       NULL = fixed variance (c2 of the table); else the per-element model_log_variance of a learned-variance model
 *                       (gaussian_diffusion.py:262-276), same shape as x: the noise term of mode 0 / 2 becomes (t!=0)*exp(lv/2)*noise
 * t: (B) int64 indices into the table of T rows (a t outside [0, T) reads nothing out of bounds and turns that
 * sample's outputs into NaN; the reference raises IndexError, which the Python binding reproduces); n_per_sample = C*H*W; noise may be NULL (no noise term:
 * `sample` is then the model mean of p_mean_variance); pred_xstart may be NULL. */
int hl_diffusion_step(int mode, const float *x, const float *eps, const float *noise, const float *coef,
                      const int64_t *t, float *sample, float *pred_xstart, int64_t n_per_sample, int B, int T, int clip,
                      const float *log_variance, void *stream);

/* Likelihood evaluation (calc_bpd_loop, _prior_bpd, gaussian_diffusion.py:653-687, 774-848) and DDIM inversion (ddim_reverse_sample,
 * :531-567).  coef: the (T, 16) fp32 eval table the host mirror builds from the float64 schedule (each entry the fp32 cast of the fp64 value,
 * like _extract_into_tensor), one row per kept timestep:
 *   [0] sqrt_recip_acp  [1] sqrt_recipm1_acp  [2] posterior_mean_coef1  [3] posterior_mean_coef2  [4] 1/coef1  [5] coef2/coef1
 *   [6] posterior_log_variance_clipped  [7] log(beta)  [8] the fixed model log-variance (FIXED_LARGE / FIXED_SMALL; 0 for learned)
 *   [9] sqrt_acp  [10] sqrt(1 - acp)  [11] sqrt(acp_next)  [12] sqrt(1 - acp_next)  (both in fp32 from fp32 acp_next, as the reference;
 *   acp_next of the last row is 0)  [13] log(1 - acp)  [14..15] 0
 * t: (B) int64 row indices.  A t outside [0, T) never reads outside the table: row 0 is read and that sample's outputs become NaN (the
 * Python binding raises IndexError first, like the reference).  n_per_sample = C*H*W.  Elementwise arithmetic is in the reference's fp32
 * op order; each kernel has an f32x4 path (n % 4 == 0, 16-byte aligned pointers) and a scalar path. */
/* x_t = sqrt_acp[t] * x_start + sqrt(1 - acp[t]) * noise */
int hl_diffusion_q_sample(const float *x_start, const float *noise, const float *coef, const int64_t *t, float *x_t,
                          int64_t n_per_sample, int B, int T, void *stream);
/* One reverse DDIM step x_t -> x_{t+1} (eta = 0):
 *   mode 0:  x0 = clip(r*x - rm1*eps)      mode 1: x0 = eps (pred_xstart already processed by the caller; `clip` ignored)
 *   e = (r*x - x0) / rm1;  sample = x0 * sqrt(acp_next) + sqrt(1 - acp_next) * e;  pred_xstart (may be NULL) = x0 */
int hl_diffusion_reverse_step(int mode, const float *x, const float *eps, const float *coef, const int64_t *t, float *sample,
                              float *pred_xstart, int64_t n_per_sample, int B, int T, int clip, void *stream);
#define HL_MEAN_EPSILON 0
#define HL_MEAN_START_X 1
#define HL_MEAN_PREVIOUS_X 2
#define HL_VAR_FIXED 0
#define HL_VAR_LEARNED 1
#define HL_VAR_LEARNED_RANGE 2
/* Bytes of fp64 scratch hl_diffusion_vb_terms / hl_diffusion_prior_bpd need for B samples of n_per_sample elements. */
size_t hl_diffusion_vb_scratch_bytes(int64_t n_per_sample, int B);
/* One timestep of calc_bpd_loop after the model call.  model_out: the mean-type half of the model output, sample b at model_out + b*out_stride
 * (out_stride = n_per_sample, or 2*n_per_sample for the first half of a learned-variance model's 2C channels); model_var: the variance half
 * (NULL exactly when var_type == HL_VAR_FIXED), same stride.  Per element:
 *   x0 = EPSILON: r*x_t - rm1*out | START_X: out | PREVIOUS_X: out/coef1 - coef2/coef1 * x_t;  clip -> clamp(x0, -1, 1)
 *   mean = PREVIOUS_X: out | else coef1*x0 + coef2*x_t
 *   lv = FIXED: [8] | LEARNED: var | LEARNED_RANGE: frac*[7] + (1-frac)*[6], frac = (var + 1)/2
 *   term = t == 0: -discretized_gaussian_log_likelihood(x_start; mean, 0.5*lv) | else normal_kl(coef1*x_start + coef2*x_t, [6], mean, lv)
 *   xm = (x0 - x_start)^2;  mse = ((r*x_t - x0)/rm1 - noise)^2
 * The per-sample means over n_per_sample are summed in fp64 in a fixed order (per-workgroup partials in `scratch`, then one fixed-order pass;
 * no atomics: bit-reproducible) and written as fp32 to vb[b*ld + j] (mean term / ln 2), xstart_mse[b*ld + j], mse[b*ld + j]. */
int hl_diffusion_vb_terms(int mean_type, int var_type, int clip, const float *x_start, const float *x_t, const float *noise,
                          const float *model_out, const float *model_var, int64_t out_stride, const float *coef, const int64_t *t,
                          int64_t n_per_sample, int B, int T, float *vb, float *xstart_mse, float *mse, int64_t ld, int64_t j,
                          void *scratch, size_t scratch_bytes, void *stream);
/* prior_bpd[b] = mean over the sample of normal_kl(sqrt_acp[T-1]*x_start, log(1 - acp[T-1]), 0, 0) / ln 2, same fixed-order reduction. */
int hl_diffusion_prior_bpd(const float *x_start, const float *coef, int64_t n_per_sample, int B, int T, float *prior_bpd,
                           void *scratch, size_t scratch_bytes, void *stream);

/* Single ops of the UNet path, exposed for parity tests and profiling (NHWC fp32).
 * One convolution through the kernels of the network, planned as hl_unet_forward plans the same layer.  scratch: at least
 * hl_conv2d_scratch_bytes(...) bytes (hl_conv2d_nhwc: at HL_CONV_FP32_DIRECT), with_gn = 1 exactly when coefA / coefB are given; less is
 * refused with HL_ERR_ARG, more is ignored.  It holds the packed weights, the materialised GroupNorm input, the per-image scale of a raw
 * fp16x2 input and the split-K slabs of the plan.  The plan is always the one the layer takes with the 64 MiB of split-K room it has
 * inside hl_unet_forward; the scratch holds the slabs that plan writes (for a forward layer the larger of its plans with and without a
 * GroupNorm in front, so with_gn adds the GroupNorm input and nothing else), not the whole 64 MiB.  The queries plan the layer on the
 * host: a test switch of the dispatch (hl_debug_set_h16_min_blocks) set between a query and its call can make the call refuse.
 * Arguments no call accepts (N, H, W, Cout <= 0, Cin not a positive multiple of 16, ks not 1 or 3, stride not 1 or 2, unknown mode, stride 2
 * together with upsample, with_gn together with upsample) give 0: the call, its size queries and its plan queries read one check.  A 1x1
 * convolution with stride 2 or behind the upsample is accepted (the direct kernels take it). */
size_t hl_conv2d_scratch_bytes(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn);
/* The plan behind that size (host arithmetic, no HIP call): *h_kernel = the kernel the call launches - 0 k_conv, 1 k_conv_dma, 2 k_conv_bf3,
 * 3 k_conv_wino, 4 k_conv_wino4, 5 k_conv_wino4w, 6 k_conv_h16 / k_conv1_h16, 7 k_conv_h2s, 8 k_conv1_h2s, 9 k_conv_h2d, 10 k_conv_h2s_ph (an
 * Upsample convolution as four 2x2-tap phases); the numbers stay - *h_splits = its split-K slabs (1: none). */
int hl_conv2d_plan(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn, int *h_kernel, int *h_splits);
/* The whole of that plan: which INSTANTIATION the call launches (host arithmetic, no HIP call).  silu: the call's silu (SiLU without a
 * GroupNorm is refused, as by the call); want_stats = 1: the call is hl_conv2d_nhwc_gn, which asks the launch for the statistics of the
 * output.  h_plan: HL_PLAN_FIELDS ints, in this order (the numbers stay):
 *   [HL_PLAN_KERNEL]     the kernel, as *h_kernel of hl_conv2d_plan
 *   [HL_PLAN_SPLITS]     split-K slabs (1: none; more: k_splitk_finish[_st] sums them)
 *   [HL_PLAN_CFG]        k_conv's tile: 0 = 128 pixels x 96 channels, 1 = 128 x 32 (Cout <= 32), 2 = 64 x 64 (set for every kernel; only k_conv reads it)
 *   [HL_PLAN_TILE8]      k_conv_dma / k_conv_bf3: 1 = the 8-wave 256 x 96 tile, 0 = 4 waves on 128 x 96
 *   [HL_PLAN_GN_MODE]    the GroupNorm in front: 0 none, 1 the affine, 2 the affine + SiLU (k_conv's template mode when HL_PLAN_PRE is HL_PRE_NONE)
 *   [HL_PLAN_PRE]        HL_PRE_*: the GroupNorm(+SiLU) materialised by a pass of its own before the convolution, and in which format - none
 *                        (fused into the kernel's staging, or no GroupNorm), dense fp32 (k_gn_apply), fp32 channel-blocked [C/8][pixel][8]
 *                        (k_gn_apply_blk; k_conv_wino4<., true> and the blk form of k_conv_wino4w read it), the 16-bit image (k_gn_apply_h16;
 *                        k_conv_h16), the two-plane fp16 image (k_gn_apply_h16; k_conv_h2s)
 *   [HL_PLAN_STATS_BY]   HL_STATS_BY_*: who adds the output statistics - nobody (the consumer computes them from the tensor), the kernel's
 *                        epilogue, or the split-K finish (k_splitk_finish_st instead of k_splitk_finish)
 *   [HL_PLAN_STAT_SLOTS] what hl_conv2d_nhwc_gn returns in *h_used_stats (0 unless want_stats)
 *   [HL_PLAN_KT_PER]     k-tiles per slab */
#define HL_PLAN_KERNEL 0
#define HL_PLAN_SPLITS 1
#define HL_PLAN_CFG 2
#define HL_PLAN_TILE8 3
#define HL_PLAN_GN_MODE 4
#define HL_PLAN_PRE 5
#define HL_PLAN_STATS_BY 6
#define HL_PLAN_STAT_SLOTS 7
#define HL_PLAN_KT_PER 8
#define HL_PLAN_FIELDS 9
#define HL_PRE_NONE 0
#define HL_PRE_DENSE 1
#define HL_PRE_BLOCKED 2
#define HL_PRE_HALF 3
#define HL_PRE_TWO_PLANE 4
#define HL_STATS_BY_NONE 0
#define HL_STATS_BY_EPILOGUE 1
#define HL_STATS_BY_FINISH 2
int hl_conv2d_plan_ex(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn, int silu, int want_stats,
                      int *h_plan);
int hl_conv2d_nhwc(const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias, int Cout,
                   int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu,
                   const float *residual, float *out, void *scratch, size_t scratch_bytes, void *stream);
/* hl_conv2d_nhwc with an explicit arithmetic mode (HL_CONV_*); scratch: hl_conv2d_scratch_bytes(conv_mode, ...). */
int hl_conv2d_nhwc_mode(int conv_mode, const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias,
                        int Cout, int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu,
                        const float *residual, float *out, void *scratch, size_t scratch_bytes, void *stream);
/* ---- backward of the UNet (gaussian_diffusion.py:688-772 -> loss.backward() through unet.py:550-615) --------
 * Backward-DATA of a convolution is a forward convolution of the output gradient with the flipped, channel-transposed weights
 * (hl_conv2d_nhwc_bwd_data); stride 2 goes through hl_zero_stuff2_nhwc first, the nearest-x2 upsample through
 * hl_upsample2_backward_nhwc afterwards.  humanliff_amd/improved_diffusion/unet_train.py holds the autograd.Functions.
 *
 * Weight gradient: dW[co][ci][ky][kx] = sum_p dY[p][co] * X[p*stride + (ky,kx) - pad][ci] and db[co] = sum_p dY[p][co] with dw (Cout, Cin,
 * ks, ks) in the reference's OIHW parameter layout; x (N,H,W,Cx), dy (N,Hout,Wout,Cy) dense NHWC with Cx >= Cin, Cy >= Cout (zero-padded
 * channels are ignored); `upsample`: the convolution ran on the nearest-x2 upsampled x.  (hl_conv2d_wgrad_nhwc_ws below.) */
/* hl_conv2d_nhwc_bwd_data: d input of a convolution from d output, through the forward kernels: dy (N,Ho,Wo,Cy) dense NHWC with
 * Cy >= Cout a multiple of 16 (zero-padded channels), w the convolution's own (Cout, Cin, ks, ks) weights - read flipped and
 * channel-transposed while they are re-laid for the kernel, no flipped copy is made -, dx (N,H,W,Cx) with Cx >= Cin (channels
 * [Cin, Cx) are not written).  stride 2 (ks 3): dx is (N, 2Ho, 2Wo, Cx) - the whole zero-stuffed grid is stored, so the layer's input had
 * even H and W (an odd size has (H + 1) / 2 output rows: the caller refuses it, unet_train.py); upsample: the convolution ran on the
 * nearest-x2 image, (Ho,Wo) = (2H,2W), both even, Cx a multiple of 4 - and the 2x2 block sums are stored for all Cx channels, so there
 * the channels [Cin, Cx) come back zero.
 * scratch: hl_conv2d_bwd_data_scratch_bytes(...) of the same arguments (the zero-stuffed / upsampled gradient in front of the
 * convolution's own room); less is refused with HL_ERR_ARG, more is ignored; arguments the call refuses give 0. */
size_t hl_conv2d_bwd_data_scratch_bytes(int conv_mode, int N, int Ho, int Wo, int Cy, int Cout, int Cin, int ks, int stride, int upsample, int Cx);
/* The plan of that call (host arithmetic, no HIP call; the kernel numbers of hl_conv2d_plan): the forward convolution of the gradient,
 * Cy -> Cin channels on the (Ho, Wo) grid - (2Ho, 2Wo) for stride 2 - with the forms a backward-data call may use (never the fp16x2
 * ones; the 16-bit form in bf16 under HL_CONV_BF16).  Refuses what the call refuses. */
int hl_conv2d_bwd_data_plan(int conv_mode, int N, int Ho, int Wo, int Cy, int Cout, int Cin, int ks, int stride, int upsample, int Cx,
                            int *h_kernel, int *h_splits);
int hl_conv2d_nhwc_bwd_data(int conv_mode, const float *dy, int N, int Ho, int Wo, int Cy, const float *w_oihw, int Cout, int Cin, int ks,
                            int stride, int upsample, float *dx, int Cx, void *scratch, size_t scratch_bytes, void *stream);
/* hl_conv2d_wgrad_nhwc_ws: the weight / bias gradients, without atomics.  3x3 layers: k_conv_wgrad_t (a workgroup owns a 64x64 channel block of
 * dW for all nine taps; dY rows and input patch of an 8x8-pixel tile staged in LDS once); 1x1 layers: k_conv_wgrad_1x1 (192 x 64 channel
 * block, 64-pixel tiles).  Per-slab partial blocks go to `scratch` and k_wgrad_finish sums them in a fixed order: dw / db are plainly
 * stored (no need to zero them) and bit-reproducible.  Needs Cx, Cy multiples of 4 and `scratch` of
 * hl_conv2d_wgrad_scratch_bytes(...) bytes (0 = this geometry has no kernel: channel counts that are not multiples of 4, or a 1x1
 * convolution with stride 2 / behind an upsample - hl_conv2d_wgrad_nhwc_ws refuses those; the atomics-based entry of rounds 2-3 is gone). */
size_t hl_conv2d_wgrad_scratch_bytes(int N, int H, int W, int Cx, int Cy, int ks, int stride, int upsample, int Cout, int Cin);
int hl_conv2d_wgrad_nhwc_ws(const float *x, int N, int H, int W, int Cx, const float *dy, int Cy, int ks, int stride, int upsample,
                            float *dw, int Cout, int Cin, float *db, void *scratch, size_t scratch_bytes, void *stream);
/* The same with an arithmetic mode: HL_CONV_FP16 / HL_CONV_BF16 round both operands to 16 bits and accumulate in fp32
 * (v_mfma_f32_32x32x16, k_conv_wgrad_h16) on the 3x3 / stride-1 layers; every other layer and mode as hl_conv2d_wgrad_nhwc_ws. */
int hl_conv2d_wgrad_nhwc_ws_mode(int conv_mode, const float *x, int N, int H, int W, int Cx, const float *dy, int Cy, int ks, int stride,
                                 int upsample, float *dw, int Cout, int Cin, float *db, void *scratch, size_t scratch_bytes, void *stream);
/* y (N,HW,C dense) = silu ? silu(x*A + B) : x*A + B with the per-(n,c) affine of hl_groupnorm_coef; x has a channel pitch. */
int hl_gn_apply_nhwc(const float *x, long x_pitch, int N, int HW, int C, const float *coefA, const float *coefB, int silu, float *y,
                     void *stream);
/* backward of y = silu?(x*A + B): with du = dout * silu'(x*A + B) (or dout), S[n][c] = (sum_p du, sum_p du*x), written (N,C,2);
 * per-workgroup partial sums in the caller's scratch (hl_gn_backward_scratch_bytes) added in a fixed order - no atomics, the same
 * bits on every run; then dx = k1[n,c]*du + k2[n,c]*x + k3[n,c] (+ dx_add), the (N,C) coefficients being the caller's small
 * tensor algebra on S, the group statistics and the affine parameters (unet_train.py). */
size_t hl_gn_backward_scratch_bytes(int N, int HW, int C);
int hl_gn_backward_reduce(const float *x, long x_pitch, const float *dout, int N, int HW, int C, const float *coefA, const float *coefB,
                          int silu, float *S, void *scratch, size_t scratch_bytes, void *stream);
int hl_gn_backward_apply(const float *x, long x_pitch, const float *dout, int N, int HW, int C, const float *coefA, const float *coefB,
                         int silu, const float *k1, const float *k2, const float *k3, const float *dx_add, float *dx, void *stream);
/* The two as the training path uses them (unet_train.py), the (N,C) algebra between the passes in a kernel of its own:
 * forward   y = silu?( GroupNorm32(x) [* (1 + scale) + shift] ), x / y dense (N,H,W,C); scale_shift (N,2C) = [scale | shift] or NULL
 *           (unet.py:203-206); also returns the affine coefA / coefB (N,C) and gstat (N,32,2) = (mean, rstd) per group for the backward.
 *           scratch: hl_groupnorm_scratch_bytes(N) (also hl_groupnorm_coef's and hl_groupnorm_train_forward_eps's).
 * backward  dx (may be NULL), dgamma / dbeta (C) (written, not accumulated), dscale_shift (N,2C) (iff scale_shift); scratch:
 *           hl_groupnorm_train_backward_scratch_bytes(N, H*W, C).  Deterministic (fixed-order sums). */
size_t hl_groupnorm_scratch_bytes(int N);
size_t hl_groupnorm_train_backward_scratch_bytes(int N, int HW, int C);
int hl_groupnorm_train_forward(const float *x, int N, int H, int W, int C, const float *gamma, const float *beta, const float *scale_shift,
                               int silu, float *coefA, float *coefB, float *gstat, float *y, void *scratch, size_t scratch_bytes, void *stream);
int hl_groupnorm_train_backward(const float *x, const float *dout, int N, int H, int W, int C, const float *coefA, const float *coefB, int silu,
                                const float *gstat, const float *gamma, const float *beta, const float *scale_shift, float *dx,
                                float *dgamma, float *dbeta, float *dscale_shift, void *scratch, size_t scratch_bytes, void *stream);
/* dx (N,H,W,C) = sums of the 2x2 blocks of d_up (N,2H,2W,C): backward of the nearest-x2 upsample (unet.py:77). */
int hl_upsample2_backward_nhwc(const float *d_up, int N, int H, int W, int C, float *dx, void *stream);
/* z (N,2Ho,2Wo,C): z[2y][2x] = dy[y][x], zero elsewhere - backward-data of a stride-2 3x3 conv = flipped 3x3 conv of z. */
int hl_zero_stuff2_nhwc(const float *dy, int N, int Ho, int Wo, int C, float *z, void *stream);

/* ---- training kernels of the 3-D-aware and cross-attention UNets (csrc/hl_unet_train_xf.hip; unet_train.py) ----------------------
 * All fp32, enqueue-only (no host syncs, no allocations), fixed-order sums without float atomics: the same bits on every run.
 *
 * Tri-plane aggregation of the 3-D-aware ResBlock (unet.py:208-214).  g (N,H,3W,C) dense NHWC = the GroupNorm affine output (scale /
 * shift applied, no SiLU) with the planes xy | xz | zy side by side, H == W, C % 4 == 0.
 * forward   out (N,H,3W,3C) = silu(cat[g_p, m1_p, m2_p]) per plane p, with rowmean(q)[y] = mean over the W columns of plane q,
 *           colmean(q)[x] = mean over its H rows:  xy: [g, rowmean(xz), colmean(zy)],  xz: [g, rowmean(xy), rowmean(zy)],
 *           zy: [g, colmean(xy), colmean(xz)].  Also writes the means, rmean (N,3,H,C) and cmean (N,3,W,C), for the backward.
 * backward  dg (N,H,3W,C) from dout (N,H,3W,3C): the own slot times silu'(g), plus, for every mean, the sum of its slot's gradient
 *           along the broadcast axis times silu'(mean) / W (or / H), broadcast back onto the plane it came from.
 *           scratch: hl_triplane_agg_backward_scratch_bytes(N, H, W, C). */
size_t hl_triplane_agg_backward_scratch_bytes(int N, int H, int W, int C);
int hl_triplane_agg_forward(const float *g, int N, int H, int W, int C, float *rmean, float *cmean, float *out, void *stream);
int hl_triplane_agg_backward(const float *dout, const float *g, const float *rmean, const float *cmean, int N, int H, int W, int C, float *dg,
                             void *scratch, size_t scratch_bytes, void *stream);
/* nn.LayerNorm(C) over the channels of each pixel, x / y / dy / dx dense (npix, C).
 * forward   y = (x - mean) * rstd * gamma + beta, rstd = 1 / sqrt(var + eps) (biased variance); stat (npix, 2) = (mean, rstd).
 * backward  dx (may be NULL) = rstd * (gd - mean_c(gd) - xh * mean_c(gd * xh)), gd = dy * gamma, xh = (x - mean) * rstd;
 *           dgamma = sum_p dy * xh, dbeta = sum_p dy (C each, written, not accumulated).  C % 4 == 0, C <= 1024;
 *           scratch: hl_layernorm_backward_scratch_bytes(npix, C). */
int hl_layernorm_train_forward(const float *x, int64_t npix, int C, const float *gamma, const float *beta, float eps, float *y, float *stat,
                               void *stream);
size_t hl_layernorm_backward_scratch_bytes(int64_t npix, int C);
int hl_layernorm_train_backward(const float *x, const float *dy, const float *stat, int64_t npix, int C, const float *gamma, float *dx,
                                float *dgamma, float *dbeta, void *scratch, size_t scratch_bytes, void *stream);
/* GEGLU (spatial_transformer.py:37-44): in (npix, 2F) = [u | gate], exact erf GELU.
 * forward   out (npix, F) = u * gelu(gate).
 * backward  din (npix, 2F) = [d * gelu(gate) | d * u * (Phi(gate) + gate * phi(gate))]. */
int hl_geglu_forward(const float *in, int64_t npix, int F, float *out, void *stream);
int hl_geglu_backward(const float *in, const float *dout, int64_t npix, int F, float *din, void *stream);
/* hl_groupnorm_train_forward with the GroupNorm's eps as an argument (SpatialTransformer.norm: eps 1e-6, spatial_transformer.py:66-67);
 * the same outputs, so hl_groupnorm_train_backward is its backward unchanged. */
int hl_groupnorm_train_forward_eps(const float *x, int N, int H, int W, int C, const float *gamma, const float *beta, const float *scale_shift,
                                   int silu, float eps, float *coefA, float *coefB, float *gstat, float *y, void *scratch, size_t scratch_bytes,
                                   void *stream);

/* hl_conv2d_nhwc_mode followed by the GroupNorm32 affine of its OUTPUT (nn.py:17-19,100: y = out*A[n,c] + B[n,c] for the layer
 * that normalises `out` next): the statistics come from the epilogue of the kernel that stored `out` (fixed-point group totals added
 * with integer atomics: order-free, bit-reproducible) - the tensor is not read again; *h_used_stats returns nonzero when the epilogue
 * emitted them, 0 when the kernel
 * path taken emits none and the statistics were computed from the tensor instead.  scratch: hl_conv2d_gn_scratch_bytes(...), the
 * arguments of hl_conv2d_scratch_bytes (the output's totals and a GroupNorm pass's scratch in front of the convolution's own room).
 * Accuracy: the epilogue totals are sums of raw x and x^2 - within 4x the error of the reference's fp32 F.group_norm (+ 2e-6) while the stored tensor's groups sit at
 * mean/std <= 10, (mean/std)^2 beyond (1.5e-4 at 25, 2.2e-3 at 80) (csrc/hl_stats.h). */
size_t hl_conv2d_gn_scratch_bytes(int conv_mode, int N, int H, int W, int Cin, int Cout, int ks, int stride, int upsample, int with_gn);
int hl_conv2d_nhwc_gn(int conv_mode, const float *in, int N, int H, int W, int Cin, const float *w_oihw, const float *bias, int Cout,
                      int ks, int stride, int upsample, const float *coefA, const float *coefB, int silu, const float *residual,
                      float *out, const float *gamma, const float *beta, float *next_coefA, float *next_coefB, int *h_used_stats,
                      void *scratch, size_t scratch_bytes, void *stream);
/* GroupNorm32 of x folded to y = x*A[n,c] + B[n,c] (nn.py:17-19,100; emb = the ResBlock's [scale | shift] rows, unet.py:203-206).  Accuracy: the statistics are taken about a
 * pivot (the group's first value), so x*A + B stays within 4x the error of the reference's fp32 F.group_norm (+ 2e-6) against float64 up to mean/std = 100 and for
 * constant groups; scratch: hl_groupnorm_scratch_bytes(N). */
int hl_groupnorm_coef(const float *x, int N, int H, int W, int C, const float *gamma, const float *beta,
                      const float *emb /* (N,2C) or NULL */, float *coefA, float *coefB, void *scratch,
                      size_t scratch_bytes, void *stream);
int hl_attention_nhwc(const float *qkv, int N, int T, int C, int heads, float *out, void *stream);
/* The attention as hl_unet_forward runs it in `conv_mode`: HL_CONV_FP32 (the default) forms both products (scores, probabilities x values) from fp16x2 operands on
 * v_mfma_f32_32x32x16_f16 where the kernel has that form (head sizes 96 and 192 on short sequences: the UNet's 32-, 16- and 8-pixel levels); every other mode = hl_attention_nhwc
 * (fp32 MFMA).  Round 6: the V tiles are staged under a running power-of-two scale, so the result follows any scaling of V exactly (2^-14 ... 2^10 tested bit for bit); Q and K
 * are split as they are (their error enters the scores absolutely and the softmax flattens it). */
int hl_attention_nhwc_mode(int conv_mode, const float *qkv, int N, int T, int C, int heads, float *out, void *stream);
/* Backward of hl_attention_nhwc (QKVAttention, unet.py:255-274, under train_util.py:200-246): qkv as in the forward, out = the forward's
 * output (N,T,C; required non-NULL, no longer read: D below comes from P and dP), dout = its gradient -> dqkv (N,T,3C).  fp32 MFMA, probabilities recomputed
 * (flash-style), every output summed by one wave in a fixed order (deterministic).  scratch: hl_attention_backward_scratch_bytes() (per query: row maximum,
 * 1/row sum, D = sum_j P_ij dP_ij; head sizes that are not a multiple of 32 materialise P and dS there instead). */
size_t hl_attention_backward_scratch_bytes(int N, int T, int C, int heads);
int hl_attention_nhwc_backward(const float *qkv, const float *out, const float *dout, int N, int T, int C, int heads, float *dqkv,
                               void *scratch, size_t scratch_bytes, void *stream);
/* timestep_embedding (nn.py:103-121): t int64 (B) or t_float fp32 (B) -> out (B, dim), dim even */
int hl_timestep_embedding(const int64_t *t, const float *t_float, int B, int dim, float *out, void *stream);

/* Test switch: the number of workgroups from which the convolution dispatch takes k_conv_h16 in the 16-bit modes (default 48);
 * v < 0 restores the default.  The unit tests run the kernel on single tiles with it. */
int hl_debug_set_h16_min_blocks(long v);
/* test switch of the single-convolution entry points (hl_conv2d_nhwc*): where the power-of-two scale of a raw input of the fp16x2 kernels comes from.
   0 (default): an exact abs-max pass over the input (tensor_absmax); 1: the fixed-point group totals (sum x^2) - what the producers' epilogues leave inside
   hl_unet_forward - formed here by one pass (tensor_totals), so that the network's scale source can be tested on single layers. */
int hl_debug_set_single_op_scale_source(int from_totals);
/* test switch of the attention's work distribution: query tiles per workgroup of the key-split fp16x2 kernel at head size 96 (1 or 2), and the placement of the
   workgroups of one (image, head) on one XCD (1 off, 2 on); 0 (default) leaves either to the dispatch rule of hl::attention.  Every choice gives the same bits;
   the tests run the small shapes on each. */
int hl_debug_set_attention_tiling(int query_tiles, int placement);

/* sample_pdf's uniforms on the device, bit for bit (replaces `u = torch.rand(...)` on the CPU generator + upload, NeRF/renderer.py:545):
 * continues the mt19937 stream of ATen's CPU generator from `state` (624 words, device) at position `pos` (words of the current block
 * already drawn; 624 = block used up, also the freshly seeded generator) and writes the next n floats u = (word & (2^24 - 1)) * 2^-24 to
 * out; state_out (625 words, device) receives the state and position behind the last number - the host side advances its generator
 * with it (humanliff_amd/NeRF/cpu_rng.py).  One workgroup; enqueue-only. */
int hl_mt19937_uniform(const uint32_t *state, int pos, float *out, int64_t n, uint32_t *state_out, void *stream);
/* test switch: the largest number of words one walk launch of hl_mt19937_uniform produces (default 2^28: the walk addresses its output through a 32-bit buffer
 * range; longer requests continue from the state the piece before left).  words <= 0 restores the default.  The unit tests run the chaining with small pieces. */
int hl_debug_set_mt19937_piece(int64_t words);

/* ---- mesh extraction (mcubes.smooth + mcubes.marching_cubes behind extract_geometry, NeRF/renderer.py:290-321) ----------
 * Contract: DESIGN.md "Mesh extraction".  Volumes are (nx, ny, nz) C order (x slowest) with nx*ny*nz*5 < 2^31.  The host reads
 * the device `counts` between the phases to size the next buffers; every reduction is integer or fixed-order (bit-reproducible).
 *
 * Constrained smoothing (Lempitsky 2010 as PyMCubes' smooth_constrained):
 *   hl_smooth_prepare: binarize vol > 0 (fp32, or fp64 if is_fp64), exact signed distance d (edt(b) - 0.5 on b, -edt(~b) + 0.5
 *     off b) into d_out (fp64 volume); counts[0] = band size (|d| <= band_radius), counts[1] = voxels with vol > 0.
 *   hl_smooth_band (ws as left by hl_smooth_prepare): the nb band variables - lin (int32 voxel index), nbr (int32 6 x nb: slot of
 *     the -x, +x, -y, +y, -z, +z band neighbour or -1), start value x = d, bounds lower / upper.
 *   hl_smooth_sweeps: n_sweeps damped (w = 1/2) projected Jacobi sweeps on A = Q^T Q in place on x, then (energy != NULL)
 *     energy[0] = x^T A x / 2 of the result; n_sweeps = 0 gives the energy alone.
 *   hl_smooth_scatter: out[lin[s]] = x[s]. */
size_t hl_smooth_workspace_bytes(int nx, int ny, int nz);
int hl_smooth_prepare(const void *vol, int is_fp64, int nx, int ny, int nz, double band_radius, double *d_out, int64_t *counts,
                      void *ws, size_t ws_bytes, void *stream);
int hl_smooth_band(const double *d, int nx, int ny, int nz, double band_radius, int64_t nb, int32_t *lin, int32_t *nbr, double *x,
                   double *lower, double *upper, void *ws, size_t ws_bytes, void *stream);
size_t hl_smooth_sweep_scratch_bytes(int64_t nb);
int hl_smooth_sweeps(const int32_t *nbr, const double *lower, const double *upper, int64_t nb, int n_sweeps, double *x, double *energy,
                     void *scratch, size_t scratch_bytes, void *stream);
int hl_smooth_scatter(const double *x, const int32_t *lin, int64_t nb, double *out, void *stream);
/* Marching cubes at `iso` on an fp64 volume (corner above when value > iso):
 *   hl_mc_count: classify every voxel and scan; counts[0] = vertices V, counts[1] = triangles T.
 *   hl_mc_emit (ws as left by hl_mc_count): verts fp64 (V,3) in index coordinates, ordered by edge key
 *     ((i*ny + j)*nz + k)*3 + axis; tris int64 (T,3), by cube then case-table order, normals toward the above side.
 *   hl_mc_case_table: host copy of the baked table, h_tris 256 x hl_mc_max_triangles() x 3 cube edges (-1 padded), h_ntri 256. */
size_t hl_mc_workspace_bytes(int nx, int ny, int nz);
int hl_mc_count(const double *vol, int nx, int ny, int nz, double iso, int64_t *counts, void *ws, size_t ws_bytes, void *stream);
int hl_mc_emit(const double *vol, int nx, int ny, int nz, double iso, double *verts, int64_t *tris, void *ws, size_t ws_bytes, void *stream);
int hl_mc_max_triangles(void);
int hl_mc_case_table(int8_t *h_tris, uint8_t *h_ntri);
/* Finishing an extracted mesh (extensions beside the reference contract; DESIGN.md "Mesh extraction", "Finishing the mesh").
 *   hl_mc_vertex_normals (ws as left by hl_mc_count at the same vol / iso): unit normals fp64 (n_verts,3) in hl_mc_emit's vertex
 *     order.  Vertex on the lattice edge a -> b at t = (iso - f_a)/(f_b - f_a): n_idx = (1-t) g(a) + t g(b), g the central difference
 *     (one-sided at a volume face), n = normalize(n_idx / ext); h_ext: 3 HOST doubles, the world extent per axis, or NULL (1,1,1).
 *     A zero or non-finite vector gives (0,0,0).  keys: n_verts int32 of device scratch, left holding the edge keys voxel*3 + axis.
 * Connected components of the solid side, solid = !(value > iso), 26-connectivity:
 *   hl_cc_label: labels int32 (nx,ny,nz), 0 off the solid side, 1..n on it, numbered by the smallest linear index of each
 *     component; counts[0] = n, counts[1] = link / flatten rounds run.  Relaunches until a round changes nothing and reads the
 *     device flag in between, so it SYNCHRONISES the stream; HL_ERR_RUNTIME if 40 rounds do not settle it.
 *   hl_cc_sizes: sizes[l-1] = voxels with label l (integer atomics).
 *   hl_cc_filter: out = vol, except that a voxel whose label l has keep[l-1] == 0 gets iso + |v - iso|, or the next double above
 *     iso where that is not above iso (out may be vol).
 * Vertex colours through hl_render_eval_points with n_samples = 1:
 *   hl_mesh_pack_points: (n_verts,3) fp32 points and directions -> float[4] rows, padded to a multiple of 32 rows.
 *   hl_mesh_unpack_colors: its records -> rgb fp32 (n_verts,3) = sigmoid of the raw colour, rgb8 (or NULL) = round(clip(rgb,0,1)*255). */
int hl_mc_vertex_normals(const double *vol, int nx, int ny, int nz, double iso, const double *h_ext, int64_t n_verts, int32_t *keys,
                         double *normals, void *ws, size_t ws_bytes, void *stream);
size_t hl_cc_workspace_bytes(int nx, int ny, int nz);
int hl_cc_label(const double *vol, int nx, int ny, int nz, double iso, int32_t *labels, int64_t *counts, void *ws, size_t ws_bytes,
                void *stream);
int hl_cc_sizes(const int32_t *labels, int64_t n_voxels, int64_t n_labels, int64_t *sizes, void *stream);
int hl_cc_filter(const double *vol, const int32_t *labels, const uint8_t *keep, int64_t n_voxels, int64_t n_labels, double iso, double *out,
                 void *stream);
int hl_mesh_pack_points(const float *pts, const float *dirs, int64_t n_verts, float *pts4, float *dirs4, void *stream);
int hl_mesh_unpack_colors(const float *records, int64_t n_verts, float *rgb, uint8_t *rgb8, void *stream);

/* ---- fused optimizer tail (train_util.TrainLoop.optimize_normal: _log_grad_norm, clip_grad_value_, AdamW, update_ema) -------------
 * Contract: DESIGN.md "Training loop".  fp32 tensors; the host packs a table once per parameter list and keeps it on the device.
 *   hl_adamw_chunks: number of HL_ADAMW_CHUNK-element chunks of the list (-1 on a bad list); hl_adamw_table_bytes: its table size.
 *   hl_adamw_table_pack: writes the table into HOST memory (the caller copies it to the device): ptrs holds 8 pointers per tensor,
 *     p, g, m, v, e0..e3 (g NULL: no gradient, the tensor gets its EMA updates only; e_k unused for k >= n_ema, n_ema <= 4).
 *   hl_adamw_step: one launch over the table.  Per element: the unclipped g*g into the chunk's fp64 partial (scratch, nchunks
 *     doubles, fixed order), g clamped to [-clip, clip] when clip > 0 (NaN stays NaN; .grad is not written), AdamW in torch's
 *     multi-tensor op order with the host's scalars (wd_scale = 1 - lr*wd, bc2_sqrt = sqrt(1 - beta2^step),
 *     neg_step_size = -lr / (1 - beta1^step)), then e_k = e_k * r_k + (1 - r_k) * p; ema_rates = {r_0, 1 - r_0, r_1, 1 - r_1, ...}.
 *   hl_adamw_sum_partials: one workgroup sums the n partials in a fixed order into out[0] (fp64, device).  Both enqueue-only. */
#define HL_ADAMW_CHUNK 16384
int64_t hl_adamw_chunks(const int64_t *numel, int ntensors);
size_t hl_adamw_table_bytes(int ntensors, int64_t nchunks);
int hl_adamw_table_pack(int ntensors, const int64_t *numel, void *const *ptrs, int n_ema, void *host_table, size_t table_bytes);
size_t hl_adamw_scratch_bytes(int64_t nchunks);
int hl_adamw_step(const void *table, int ntensors, int64_t nchunks, int n_ema, const float *ema_rates, float clip, float wd_scale,
                  float one_minus_beta1, float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float neg_step_size,
                  void *scratch, size_t scratch_bytes, void *stream);
int hl_adamw_sum_partials(const void *scratch, int64_t n, double *out, void *stream);

/* ---- tail of a tri-plane fitting iteration (recon_NeRF/run_nerf_batch.py:256-272: TV / L1 regularisers, Adam on tri_planes, clamp_) ----
 * Contract: DESIGN.md "Fitting loop"; csrc/hl_fit.hip.  fp32, contiguous, enqueue-only on `stream`, caller-owned scratch.
 *   hl_fit_reg: planes and grad are nplanes (= batch x 27) images of H x W (H, W >= 2), the gathered plane sets and the gradient
 *     the render backward left for them.  sums[0..2] (fp64, device) = sum |x[h] - x[h+1]|, sum |x[w] - x[w+1]|, sum |x| (fp32
 *     differences, fp64 sums in a fixed order); grad += cx (sign(x - x_dn) - sign(x_up - x)) + cy (the same along W) + cl sign(x),
 *     sign(0) = 0, sign(NaN) = NaN, a missing neighbour contributing nothing; cx, cy, cl are the host's coef / n as floats.
 *     scratch: hl_fit_reg_scratch_bytes (the workgroups' partials).
 *   hl_fit_adam_planes: torch's multi-tensor Adam (weight_decay 0; the scalars as for hl_adamw_step) over the whole parameter of
 *     num_instances x num_layers slices of slice_numel elements.  The gradient of a slice is 0 + the entries b of grad (bs x
 *     slice_numel) with (instance_idx[b], layer_idx[b]) == the slice, added in batch order; the two index arrays are int64 in DEVICE
 *     memory and are read by the kernel only (negative indices wrap, a pair out of range selects nothing).  clamp != 0: then
 *     p = clamp(p, -1, 1).  bs <= HL_FIT_MAX_BATCH. */
#define HL_FIT_CHUNK 16384
#define HL_FIT_REG_CHUNK 4096
#define HL_FIT_MAX_BATCH 64
size_t hl_fit_reg_scratch_bytes(int64_t nplanes, int H, int W);
int hl_fit_reg(const float *planes, float *grad, int64_t nplanes, int H, int W, float cx, float cy, float cl, double *sums, void *scratch,
               size_t scratch_bytes, void *stream);
int hl_fit_adam_planes(float *param, float *exp_avg, float *exp_avg_sq, const float *grad, const int64_t *instance_idx,
                       const int64_t *layer_idx, int bs, int num_instances, int num_layers, int64_t slice_numel, float one_minus_beta1,
                       float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float neg_step_size, int clamp, void *stream);

/* ---- held-out view scores (recon_NeRF/lib/all_test.py:19-42, 175-188: psnr_metric, ssim_metric, to8b) ----
 * Contract: DESIGN.md "Evaluation"; csrc/hl_metrics.hip.  Contiguous, enqueue-only on `stream`, caller-owned workspace.
 *   pred, gt: (V, H, W, 3) fp32, only read; mask: (V, H, W) uint8, nonzero = inside (mask_at_box).  Both images count as 0 outside
 *   the mask.  Per view one record: mse = mean of (pred - gt)^2 over the 3 count masked values (fp32 difference, float64 from the
 *   square on), psnr = -10 log10(mse), the mask's bounding rectangle (cv2.boundingRect; all 0 for an empty mask), and ssim =
 *   skimage's structural_similarity on the crop (7 x 7 uniform window per channel, sample covariance, K1 0.01, K2 0.03, the mean
 *   over the crop's interior, then over the channels; float64, fixed summation order).  ssim is NaN when w < 7 or h < 7.
 *   data_range: skimage's R.  flags: reserved, 0.  pred_u8 / gt_u8 (V, H, W, 3) uint8, each optional: (255 clip(x, 0, 1)) truncated,
 *   of the masked prediction and of the unmasked ground truth.  workspace: hl_image_metrics_workspace_bytes. */
typedef struct hl_metrics_record {
    double mse, psnr, ssim;
    int32_t count, x, y, w, h, reserved;
} hl_metrics_record;
size_t hl_image_metrics_workspace_bytes(int V, int H, int W);
int hl_image_metrics(const float *pred, const float *gt, const unsigned char *mask, int V, int H, int W, double data_range, unsigned flags,
                     unsigned char *pred_u8, unsigned char *gt_u8, hl_metrics_record *results, void *workspace, size_t workspace_bytes,
                     void *stream);

/* ---- LPIPS(net='vgg', version='0.1') forward (the reference's loss_fn_vgg, recon_NeRF/lib/all_test.py) ----
 * Contract: DESIGN.md 4f "LPIPS"; csrc/hl_lpips.hip.  Contiguous fp32, enqueue-only on `stream`, caller-owned workspace, exact fp32
 * products.  The network: x = (in - shift) / scale per channel; torchvision VGG-16 features[0:30] (13 3 x 3 / pad 1 convolutions with
 * bias + ReLU, widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512, a 2 x 2 floor max-pool at each |); the taps are the
 * last ReLU of each block (tap k is h >> k by w >> k); per tap d_k = mean_{y,x} sum_c lin_k[c] (n(f0) - n(f1))^2 with
 * n(f) = f / (sqrt(sum_c f^2) + 1e-10), in float64 and a fixed order; the score is d_1 + ... + d_5.
 *   params (HOST struct of DEVICE pointers): conv_w[l] is layer l's weight packed as (ceil(Cin / 16), Cout, 9, 16) - channel chunk,
 *     output channel, tap ky * 3 + kx, channel within the chunk, zero where the channel is >= Cin (layer 0: Cin 3); conv_b[l] (Cout);
 *     lin[k] (C_k); shift, scale: the scaling layer's constants, by value.
 *   hl_lpips_features: the trunk of N images - in0 (B, 3, h, w) alone (in1 NULL, N = B) or followed by in1 (B, 3, h, w) (N = 2 B).  The
 *     taps stay in the workspace as NHWC tensors (N, h_k, w_k, C_k) at the offsets hl_lpips_tap_shape gives for (N, h, w).
 *   hl_lpips: the trunk of the 2 B images and the head; out (B, 6) float64: d_1 .. d_5 and their sum per pair.  The inputs are only read.
 *   16 <= h, w <= 16384; workspace: hl_lpips_workspace_bytes(N, h, w) with N the number of images through the trunk (0: bad shape). */
#define HL_LPIPS_CONVS 13
#define HL_LPIPS_TAPS 5
typedef struct hl_lpips_params {
    const float *conv_w[HL_LPIPS_CONVS];
    const float *conv_b[HL_LPIPS_CONVS];
    const float *lin[HL_LPIPS_TAPS];
    float shift[3], scale[3];
} hl_lpips_params;
size_t hl_lpips_workspace_bytes(int N, int h, int w);
int hl_lpips_tap_shape(int N, int h, int w, int k, size_t *offset_bytes, int *hk, int *wk, int *channels);
int hl_lpips_features(const hl_lpips_params *params, const float *in0, const float *in1, int B, int h, int w, void *workspace,
                      size_t workspace_bytes, void *stream);
int hl_lpips(const hl_lpips_params *params, const float *in0, const float *in1, int B, int h, int w, double *out, void *workspace,
             size_t workspace_bytes, void *stream);

/* ---- training ray batches from resident views (recon_NeRF/lib/if_nerf_data_utils.py:87-170: sample_ray_batch, split == 'train') ----
 * Contract: DESIGN.md 4g; csrc/hl_ray_batch.hip.  Contiguous device arrays unless marked h_ (host); enqueue-only on `stream`.
 *   hl_camera_table_row: HOST.  One row of the camera table (HL_CAMERA_ROW float64: inv(K) 9, R 9, T 3, the camera centre -(R^T T) 3,
 *     the bounds padded by 0.01 6) from the arguments of that call, derived exactly as it derives them.
 *   hl_ray_views_prepare: per view, from corners (V, 8, 2) int32 - the 8 projected bound corners (x, y) in get_bound_corners' order,
 *     rounded on the host like np.round(project(...)).astype(int), |value| < 2^30 - and body (V, H, W) uint8 (non-zero where msk == 1):
 *     bound_mask = the union of get_bound_2d_mask's six quads, a pixel being set when it lies inside or on the boundary of the closed
 *     quad (exact integer arithmetic; cv2.fillPoly's own outline pixels could not be compared).  Class 0 = bound & body, class 1 =
 *     bound & ~body.  bitmaps (V, 2, H, ceil(W / 64)) uint64: bit x % 64 of word x / 64; row_table (V, 2, H + 1) int32: the exclusive
 *     prefix of a class's set bits per row, the total at [H].
 *   hl_ray_batch: one workgroup per entry b of image_idx (bs) int64.  images (V, H, W, 3) float32, or uint8 when images_u8 != 0 (then
 *     rgb = (float)u8 / 255.0f).  Round r with m rows missing takes n_body = (int)((double)m * ratio) candidates of class 0, then
 *     m - n_body of class 1; candidate `slot` of a class is that class's k-th pixel in row-major (np.argwhere) order, k =
 *     picks[b][r][class][slot] with picks (bs, max_rounds, 2, n_rays) int32, or with picks NULL k = mulhi(x, count), x the first word of
 *     Philox4x32-10 with key (seed low, seed high ^ step high) and counter (slot, b, 2 r + class, step low).  Its ray is the one
 *     hl_camera_rays_train writes for that pixel; candidates whose ray crosses the padded box exactly twice are appended in candidate order
 *     until n_rays rows are filled or max_rounds rounds are done.  Outputs per entry: rgb, ray_o, ray_d (n_rays, 3), near, far,
 *     bkgd_msk (1 = class 0) (n_rays) float32, mask_at_box (n_rays) uint8, coord (n_rays, 2) int32 (y, x); rows not filled are zeros
 *     with near 0 and far 1; n_valid (bs) int32 = rows filled, or -1 for an image_idx outside [0, V) or a pick outside its class. */
#define HL_CAMERA_ROW 30
int hl_camera_table_row(const double *h_Kinv, const double *h_R, const double *h_T, const double *h_bounds, double *h_row);
int hl_ray_views_prepare(const int32_t *corners, const unsigned char *body, int64_t V, int H, int W, uint64_t *bitmaps, int32_t *row_table,
                         void *stream);
int hl_ray_batch(const int64_t *image_idx, int bs, const void *images, int images_u8, const uint64_t *bitmaps, const int32_t *row_table,
                 const double *cameras, int64_t V, int H, int W, int n_rays, double ratio, const int32_t *picks, uint64_t seed, uint64_t step,
                 int max_rounds, float *rgb, float *ray_o, float *ray_d, float *near, float *far, float *bkgd_msk,
                 unsigned char *mask_at_box, int32_t *coord, int32_t *n_valid, void *stream);

/* ---- posing the body model: linear blend skinning, world bounds and the deformation tables (smpl/smpl_numpy.py SMPL.__call__,
 *      SynBodyView_datasets.py:141-182 prepare_input, and the per-vertex tables of NeRF/deform.py: deform_tables) ----
 * Contract: DESIGN.md "Body model"; csrc/hl_body.hip.  Contiguous fp32 device arrays, enqueue-only on `stream`, nothing allocated,
 * every sum in a fixed order (no float atomics): the same inputs give the same bits, alone or inside a batch of frames.
 * V vertices, 2 <= J <= 64 joints, P = 9 (J - 1) pose features, 1 <= S <= Sp <= 16 shape coefficients, F >= 1 frames.
 *   hl_body_pack (once per model): v_template (V,3), shapedirs (V,3,sd_cols) of which the first Sp columns are kept, posedirs (V,3,P),
 *     J_regressor (J,V), weights (V,J) -> packed, hl_body_packed_bytes(V, J, Sp) bytes, as floats in this order:
 *       posedirs (P,3,V) | shapedirs (Sp,3,V) | weights (J,V) | v_template (3,V) | J_regressor v_template (J,3) |
 *       J_regressor shapedirs (J,3,Sp)
 *     - coefficient-major, so a thread per vertex reads neighbouring addresses in neighbouring lanes.
 *   hl_body_pose: parents (J) int32 with parents[i] < i for i >= 1 (parents[0] is not read).  poses (F,3J) axis-angle; shapes (S) with
 *     shapes_stride 0 (shared) or (F,S) with shapes_stride S; rt: per frame 12 floats, the row-major 3x3 R and then Th, rt_stride 0 or 12.
 *     big (V,16), optional: a big-pose row per vertex as big_out writes it; needed for `table`.  Outputs, each optional (NULL):
 *       vertices (F,V,3) world = v_smpl R^T + Th;  joints (F,J,3) posed joints in the world;  bounds (F,2,3) min / max of the frame's
 *       vertices, - / + 0.05, y once more by 0.05 (needs vertices);  verts4 (F,V,4) = (vertices - Th) R, w = 0;  table (F,V,36), the row
 *       of hl_deform_points: t[3] Rinv[9] pose_off[3] shape_off[3] pose_off_big[3] Rbig[9] tbig[3] pad[3];
 *       big_out (F,V,16): blended R[9] t[3] pose_off[3] pad[1].
 *     workspace: hl_body_pose_workspace_bytes(J, F) bytes; afterwards it holds A (F,J,16), the joints' 4x4 transforms with the rest-joint
 *     term removed, followed by the pose features (F,P).  hl_body_chunk_frames(): frames a workgroup of the skinning pass keeps in
 *     registers per pass over posedirs. */
size_t hl_body_packed_bytes(int V, int J, int Sp);
int hl_body_pack(const float *v_template, const float *shapedirs, int sd_cols, const float *posedirs, const float *J_regressor,
                 const float *weights, int V, int J, int Sp, float *packed, void *stream);
int hl_body_chunk_frames(void);
size_t hl_body_pose_workspace_bytes(int J, int F);
int hl_body_pose(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                 int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                 float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, void *stream);
/* hl_body_pose with the margins of `bounds` as arguments: - / + margin on every axis, then y once more by y_margin (two fp32
 * subtractions in that order; neither may be negative).  hl_body_pose is this call with 0.05f, 0.05f; the TightCap dataset pads with
 * 0.05f, 0.1f (recon_NeRF/lib/TightCap_dataset.py:165-168 of the reference). */
int hl_pose_body_margins(const float *packed, const int32_t *parents, int V, int J, int Sp, int S, int F, const float *poses, const float *shapes,
                         int shapes_stride, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                         float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin, float y_margin,
                         void *stream);

/* ---- posing an SMPL-X body: SMPLX.forward + lbs of the smplx package (recon_NeRF/smplx/body_models.py:1188-1242, smplx/lbs.py), the
 *      dataset's R / Th and bounds (SynBody_dataset.py:182-192) and the renderer's per-vertex tables ----
 * Contract: DESIGN.md 4k; csrc/hl_body.hip (the X = true kernels).  The conventions of hl_body_pose hold (fp32, fixed order, enqueue-only, nothing allocated).
 * V vertices, 2 <= J <= 64 joints, P = 9 (J - 1), 1 <= S <= 32 coefficients (betas followed by expression), F >= 1 frames.
 *   hl_smplx_pack (once per model): as hl_body_pack, with TWO sets of S shape directions taken from shapedirs (V,3,sd_cols):
 *       set 1: columns [0, num_betas) followed by [expr_start, expr_start + num_expr) - shapes the body;
 *       set 2: columns [0, S) - what the renderer's canonical-space tables use (NeRF/renderer.py:87, 364 of the reference).
 *     With expr_start == num_betas the sets coincide and set 2 is not stored (two_sets = 0 below).  packed, as floats:
 *       posedirs (P,3,V) | set 1 (S,3,V) | weights (J,V) | v_template (3,V) | J_regressor v_template (J,3) | J_regressor set 1 (J,3,S)
 *       [ | set 2 (S,3,V) | J_regressor set 2 (J,3,S) ]      - hl_smplx_packed_bytes(V, J, S, two_sets) bytes.
 *   hl_smplx_pose: poses (F,3J): the full pose, pose_mean added; coef (F,S); transl (F,3) or NULL, added to the skinned vertices and
 *     joints before R / Th; rt, rt_stride, big, margins and the outputs as hl_pose_body_margins.  vertices, joints, bounds and verts4
 *     come from set 1; the table's t, shape_off (and its big-pose rows, posed with zero coefficients) from set 2 and without transl;
 *     Rinv and pose_off are common to both.  With table == NULL set 2 is not evaluated.
 *     workspace: hl_smplx_pose_workspace_bytes(J, F) bytes; afterwards A (F,J,16) of set 1, the translation columns of set 2 (F,J,4),
 *     the pose features (F,P).  Sizes outside the limits are refused before any launch: within them the skinning pass's staged frames
 *     (hl_smplx_chunk_frames() of them) fit the default 64 KB of LDS. */
size_t hl_smplx_packed_bytes(int V, int J, int S, int two_sets);
int hl_smplx_pack(const float *v_template, const float *shapedirs, int sd_cols, int num_betas, int expr_start, int num_expr,
                  const float *posedirs, const float *J_regressor, const float *weights, int V, int J, float *packed, void *stream);
int hl_smplx_chunk_frames(void);
size_t hl_smplx_pose_workspace_bytes(int J, int F);
int hl_smplx_pose(const float *packed, const int32_t *parents, int V, int J, int S, int two_sets, int F, const float *poses, const float *coef,
                  const float *transl, const float *rt, int rt_stride, const float *big, float *vertices, float *joints, float *bounds,
                  float *verts4, float *table, float *big_out, void *workspace, size_t workspace_bytes, float margin, float y_margin,
                  void *stream);

/* ---- raw dataset views -> ViewStore arrays (recon_NeRF/lib/SynBody_dataset.py:266-278: imread / 255, img[msk == 0] = 0,
 *      cv2.resize INTER_AREA of the image, INTER_NEAREST of the mask) ----
 * Contract: DESIGN.md 4i; csrc/hl_view_ingest.hip.  The resize rule of one axis, src -> dst <= src, scale = src / dst in float64:
 *   area: output d covers [f1, f2) = [d scale, d scale + scale), cell = min(scale, src - f1), s1 = ceil(f1), s2 = min(floor(f2), src - 1),
 *     s1 = min(s1, s2); taps in this order: (s1 - 1, (s1 - f1) / cell) if s1 - f1 > 1e-3; (s, 1 / cell) for s1 <= s < s2;
 *     (s2, min(min(f2 - s2, 1), cell) / cell) if f2 - s2 > 1e-3.  Weights are rounded to float32.  Agreement with cv2 itself is unverified.
 *   nearest: min(floor(d scale), src - 1).
 * HOST functions (no device work):
 *   hl_area_max_taps: the most taps an output can have, ceil(src / dst) + 1 (0 for bad sizes or dst > src).
 *   hl_area_taps: idx_out, w_out (dst, max_taps) and count_out (dst); unused slots are (0, 0.0f).  Fails if an output needs more than max_taps.
 *   hl_nearest_taps: idx_out (dst).
 *   hl_view_ingest_table: one axis packed for the kernel with T = hl_area_max_taps, hl_view_ingest_table_words(src, dst) int32 words:
 *     count (dst) | nearest (dst) | idx (dst, T) | the bits of the float32 weights (dst, T).
 * hl_view_ingest (enqueue-only): img_u8 (V, Hs, Ws, 3) and msk_u8 (V, Hs, Ws) uint8, xtab = the packed table of Ws -> W and ytab of Hs -> H
 *   on the device (not read, and may be NULL, when H == Hs and W == Ws) -> out_image (V, H, W, 3) float32 = sum over the row taps of
 *   beta * (sum over the column taps of alpha * p) in table order, p = msk != 0 ? (float)u8 / 255.0f : 0.0f, and out_body (V, H, W) uint8 =
 *   the nearest source mask pixel != 0.  The four arrays must be 16-byte aligned.  No atomics; a view's bits do not depend on V.
 *   H <= Hs, W <= Ws, H and V <= 65535, and a column reduction whose 256-output tile fits 64 KiB of LDS per source row (Ws / W up to ~60). */
int hl_area_max_taps(int src, int dst);
int hl_area_taps(int src, int dst, int max_taps, int32_t *idx_out, float *w_out, int32_t *count_out);
int hl_nearest_taps(int src, int dst, int32_t *idx_out);
size_t hl_view_ingest_table_words(int src, int dst);
int hl_view_ingest_table(int src, int dst, int32_t *h_table);
int hl_view_ingest(const unsigned char *img_u8, const unsigned char *msk_u8, int V, int Hs, int Ws, int H, int W, const int32_t *xtab,
                   const int32_t *ytab, float *out_image, unsigned char *out_body, void *stream);
/* hl_view_ingest_layers (enqueue-only; recon_NeRF/lib/TightCap_dataset.py:233-298 of the reference): hl_view_ingest for views
 *   whose cloth layer is composed from one photograph img_u8 (V, Hs, Ws, 3) and five mask planes full, person, top, bottom, shoes, each
 *   (V, Hs, Ws) uint8 and binary as "byte != 0"; layers (V) int32 on the device, values 0 .. 3 (others are clamped).  With
 *   s = person + the garments the layer wears (0: top, bottom, shoes; 1: top, shoes; 2: shoes), the source pixel of a layer < 3 is, first
 *   match: full == 0 -> 0;  s >= 2 -> the skin colour (0.607186f, 0.49289057f, 0.43795943f);  person == 0 and s == 1 -> 0;  otherwise
 *   (float)u8 / 255.0f - and its source mask is "any channel != 0".  Layer 3: full ? (float)u8 / 255.0f : 0, mask = full.  out_image is
 *   hl_view_ingest's reduction of that source (same tables, same order of sums), out_body the nearest pixel of that mask; for H == Hs and
 *   W == Ws both are the composed source itself.  A plane a view's layer does not wear is never read for that view; person, top, bottom
 *   and shoes may be NULL when no view of the batch reads them (a NULL plane that is read counts as all zero).  img_u8, the planes and the
 *   outputs must be 16-byte aligned.  Limits as for hl_view_ingest.  No atomics; a view's bits do not depend on V. */
int hl_view_ingest_layers(const unsigned char *img_u8, const unsigned char *full, const unsigned char *person, const unsigned char *top,
                          const unsigned char *bottom, const unsigned char *shoes, const int32_t *layers, int V, int Hs, int Ws, int H, int W,
                          const int32_t *xtab, const int32_t *ytab, float *out_image, unsigned char *out_body, void *stream);

/* ---- animating an extracted mesh: bind its vertices to a posed body once, repose them for any frames (an extension beside the
 *      reference) ----
 * Contract: DESIGN.md "Animating the mesh"; csrc/hl_mesh_animate.hip.  Contiguous device arrays, enqueue-only on `stream`, nothing
 * allocated, fp32 with every sum in a fixed order and no atomics: a frame has the same bits alone or inside a batch.  `rows` are the
 * forward rows hl_body_pose / hl_smplx_pose write as big_out, (V,16) per frame: R[9] t[3] pose_off[3] pad[1]; `verts4` their verts4;
 * `rt` 12 floats per frame, the row-major R and then Th.  N mesh vertices (N == 0: HL_OK, nothing launched), 1 <= K <= 8 neighbours,
 * K <= V, V >= 1, F >= 1: other sizes are refused before any launch.  rows and verts4 must be 16-byte aligned.
 *   hl_mesh_bind, against ONE frame (verts4 (V,4), rows (V,16), rt (12), transl (3) or NULL of that frame): for mesh vertex x (points (N,3), world) with
 *     optional world normal n (normals (N,3) or NULL): q = (x - Th) R;  the K body vertices of smallest d = (dx dx + dy dy) + dz dz,
 *     ordered by (d, index) ascending;  w_k = 1 / (d_k + 1e-8f) over their sum;  M = sum_k w_k R_k,  c = sum_k w_k (R_k po_k + t_k);
 *     u = M^-1 ((q - transl) - c) (inverse by cofactors; verts4 holds transl, the rows do not);  m = normalize(M^T (n R)), zero for a zero or non-finite vector (and for normals == NULL).
 *     -> ids int32 (N,K), weights (N,K), rest (N,3) = u, rest_normals (N,3) = m or NULL.
 *   hl_mesh_repose, F frames (rows (F,V,16); rt with rt_stride 0 or 12; transl (F,3) or NULL - what hl_smplx_pose adds after skinning):
 *     M_f, c_f as above from rows[f];  y = M_f u + c_f (+ transl[f]);  vertices (F,N,3) = R y + Th;  normals (F,N,3) or NULL =
 *     R normalize(cof(M_f) m), the cofactor matrix (nothing is divided; zero stays zero; needs rest_normals);  bounds (F,2,3) or NULL =
 *     min / max of the frame's vertices, - / + margin, y once more by y_margin (hl_pose_body_margins' arithmetic), through `scratch` of
 *     hl_mesh_repose_scratch_bytes(N, F) bytes (not read when bounds is NULL). */
int hl_mesh_bind(const float *points, const float *normals, int64_t N, const float *verts4, const float *rows, int V, const float *rt,
                 const float *transl, int K, int32_t *ids, float *weights, float *rest, float *rest_normals, void *stream);
size_t hl_mesh_repose_scratch_bytes(int64_t N, int F);
int hl_mesh_repose(const int32_t *ids, const float *weights, const float *rest, const float *rest_normals, int64_t N, int K, const float *rows,
                   int V, int F, const float *rt, int rt_stride, const float *transl, float *vertices, float *normals, float *bounds,
                   float margin, float y_margin, void *scratch, size_t scratch_bytes, void *stream);

/* ---- rasterising a mesh: z-buffer and shading (an extension beside the reference, which has no mesh renderer) ----
 * Contract: DESIGN.md "Rasterising the mesh"; csrc/hl_mesh_raster.hip.  Contiguous device arrays, enqueue-only on `stream`, nothing
 * allocated.  F images; vertices (vertex_frames,N,3) fp32 world with vertex_frames 1 (shared by all images) or F; triangles (T,3)
 * int32; normals (normal_frames,N,3) or NULL (flat normals), normal_frames 1 or vertex_frames; colors uint8 (N,3) or NULL (0.7 grey).
 * h_cams: a HOST float64 table, HL_RASTER_CAM_ROW values per camera: K (3,3), inv(K) (3,3), R (3,3) world->camera, T (3), row-major;
 * cam_stride HL_RASTER_CAM_ROW (F cameras) or 0 (one camera for all images).  Its rows reach the device as launch arguments.
 *   project: cam = (R v) + T, p = K cam, sx = p.x / p.z, sy = p.y / p.z in float64, snapped to 1/256 pixel; pixel centres are integer
 *     coordinates as in hl_camera_rays.  A vertex is invalid when a coordinate is not finite, cam.z <= znear or |sx|, |sy| > 2^19.
 *   cover: exact int64 edge functions with a one-sided rule on edges, fp32 perspective depth 1 / ((b0/z0 + b1/z1) + b2/z2), one
 *     64-bit atomicMin of (depth bits << 32 | triangle) per covered pixel; triangles with an invalid vertex, zero area, a culled
 *     winding or an index outside [0, N) are skipped - the last sets bit 0 of *status (device int32, cleared first; may be NULL).
 *     No near-plane clipping.  Boxes of more than hl_mesh_raster_small_box() pixels are drawn by up to 16 waves each in a second launch.
 *   resolve -> rgb_map (F,H,W,3), acc_map (F,H,W) 0 / 1, normal_map (F,H,W,3) world, depth_map (F,H,W) camera z (= the ray parameter of
 *     hl_camera_rays' rays), triangle_id int32 (F,H,W) or NULL (-1: background), barycentrics (F,H,W,3) or NULL (perspective-correct
 *     weights of the triangle's vertices 0, 1, 2).  Background: zeros, rgb 1 with HL_RASTER_WHITE_BKGD.  HL_RASTER_HEADLIGHT: rgb times
 *     |n . r| with r the unit ray direction of the pixel.
 * scratch: hl_mesh_raster_scratch_bytes(N, T, F, H, W) bytes, 16-byte aligned, in this order: camera rows F x 288 bytes; vertex records
 *     F x N x 16 bytes {int32 X, int32 Y, float z, uint32 flags}; z-buffer F x H x W x 8 bytes (rounded up to 16); 16 bytes holding the
 *     large list's uint64 counter; the large list, min(T F, 2^20) entries of 16 bytes {uint32 triangle, image, box pixels, 0}.  0 for refused sizes.
 * Refused before any launch (HL_ERR_INVALID): N, T, F, H or W < 1, F > 65535, N, T or H W >= 2^31, bad frame counts, strides, flags, znear. */
#define HL_RASTER_CAM_ROW 30
#define HL_RASTER_WHITE_BKGD 1u
#define HL_RASTER_HEADLIGHT 2u
#define HL_RASTER_CULL_BACK 4u
#define HL_RASTER_CULL_FRONT 8u
int hl_mesh_raster_small_box(void);
size_t hl_mesh_raster_scratch_bytes(int64_t N, int64_t T, int F, int H, int W);
int hl_mesh_raster(const float *vertices, int vertex_frames, int64_t N, const int32_t *triangles, int64_t T, const float *normals, int normal_frames,
                   const unsigned char *colors, const double *h_cams, int cam_stride, int F, int H, int W, double znear, unsigned flags,
                   float *rgb_map, float *acc_map, float *normal_map, float *depth_map, int32_t *triangle_id, float *barycentrics, int32_t *status,
                   void *scratch, size_t scratch_bytes, void *stream);

/* ---- simplifying a mesh: cell clustering with quadrics (an extension beside the reference, which meshes coarsely instead) ----
 * Contract: DESIGN.md "Simplifying the mesh"; csrc/hl_mesh_simplify.hip.  Contiguous device arrays, enqueue-only on `stream`, nothing
 * allocated.  vertices fp64 (N,3) world; triangles int32 (T,3); normals fp64 (N,3) or NULL; colors uint8 (N,3) or NULL.  h_cell, h_origin:
 * 3 HOST doubles each.  Geometry is float64 in cell units q = (v - origin) / cell; a vertex with a non-finite coordinate or one below
 * the origin belongs to no cell; every sum is an int64 in fixed point at 2^30 per unit, so results do not depend on scheduling.
 *   hl_mesh_simplify_bounds: bounds[0..2] / [3..5] = componentwise min / max of the valid vertices (+inf / -inf when there is none);
 *     h_origin may be NULL (every finite vertex is valid).  bounds: HL_SIMPLIFY_BOUNDS_WORDS device doubles (the rest holds partials).
 *     The host takes origin = min when none is given and the extents g = floor((max - origin) / cell) + 1 per axis.
 *   hl_mesh_simplify_count: marks the occupied cells of the g grid and ranks them; counts[0] = clusters.  *status (device int32) is
 *     cleared first; bit 0: a vertex without a cell.  counts: 6 device int64, cleared first (the odd entries are the scans' high
 *     halves and stay 0).
 *   hl_mesh_simplify_emit (scratch as left by hl_mesh_simplify_count, `clusters` = its counts[0], at most 2^21): counts[2] = surviving
 *     triangles T', counts[4] = output vertices V'.  out_vertices fp64, out_normals fp64 (unit or zero), out_colors uint8: (V',3), room
 *     for `clusters` rows, in ascending cell-key order; out_triangles int64 (T',3), room for T rows, in input order, smallest index
 *     first, orientation kept; vertex_map int64 (N): the output vertex of every input vertex, or -1.  A triangle with a vertex without
 *     a cell or an index outside [0, N) (status bit 1; never dereferenced) is dropped, as is one with two corners in one cell and every
 *     repetition of an oriented triple of cells after the one of smallest index.  Status bit 2: the duplicate table ran out of probes.
 * scratch: hl_mesh_simplify_scratch_bytes(N, T, gx, gy, gz) bytes, 16-byte aligned; it begins with the cluster id of every vertex,
 *     int32 (N) (-1: none), rounded up to 16 bytes, then the accumulators int64 (min(N, cells, 2^21), HL_SIMPLIFY_ACC_WORDS): count,
 *     position x y z, normal x y z, colour r g b, quadric xx xy xz yy yz zz xd yd zd dd.  0 for refused sizes.
 * Refused before any launch (HL_ERR_INVALID): N or T < 1 or >= 2^31, a cell that is not positive and finite, a non-finite origin, an
 *     extent < 1, more than 2^31 cells, more than 2^21 clusters. */
#define HL_SIMPLIFY_BOUNDS_BLOCKS 1024
#define HL_SIMPLIFY_BOUNDS_WORDS (6 + 6 * HL_SIMPLIFY_BOUNDS_BLOCKS)
#define HL_SIMPLIFY_ACC_WORDS 20
int hl_mesh_simplify_bounds(const double *vertices, int64_t N, const double *h_origin, double *bounds, void *stream);
size_t hl_mesh_simplify_scratch_bytes(int64_t N, int64_t T, int64_t gx, int64_t gy, int64_t gz);
int hl_mesh_simplify_count(const double *vertices, int64_t N, int64_t T, const double *h_cell, const double *h_origin, int64_t gx, int64_t gy, int64_t gz,
                           int64_t *counts, int32_t *status, void *scratch, size_t scratch_bytes, void *stream);
int hl_mesh_simplify_emit(const double *vertices, const double *normals, const unsigned char *colors, int64_t N, const int32_t *triangles, int64_t T,
                          const double *h_cell, const double *h_origin, int64_t gx, int64_t gy, int64_t gz, int64_t clusters, double *out_vertices,
                          double *out_normals, unsigned char *out_colors, int64_t *out_triangles, int64_t *vertex_map, int64_t *counts, int32_t *status,
                          void *scratch, size_t scratch_bytes, void *stream);

/* ---- measuring mesh distance: the exact closest triangle, surface samples, score sums (an extension beside the reference) ----
 * Contract: DESIGN.md "Measuring mesh distance"; csrc/hl_mesh_distance.hip.  Contiguous device arrays, enqueue-only on `stream`, nothing
 * allocated.  vertices fp64 (N,3) world; triangles int32 (T,3); h_origin: 3 HOST doubles, the lower corner of the mesh's bounds
 * (hl_mesh_simplify_bounds); h: the side of the cubic cells; gx gy gz = floor((max - origin) / h) + 1 per axis.  All geometry is float64
 * relative to the origin.  A triangle with an index outside [0, N) (status bit 0; never dereferenced) or a non-finite corner (bit 1) is
 * dropped; a query with a non-finite coordinate (bit 2) gets sqdist NaN and triangle -1.
 *   hl_mesh_distance_areas: prefix[i] = sum over j < i of a_j, a_j = llrint((|cross(b - a, c - a)| / 2) / unit), 0 for a dropped triangle;
 *     counts[0] | counts[1] << 32 = the total (2 device int64).  blocks: device scratch of ((T + 4095) / 4096) * 8 bytes.
 *   hl_mesh_distance_count: gathers the triangle records, counts the references of every cell and scans them: counts[0] | counts[1] << 32 =
 *     references in all, counts[2] = wide triangles (a box of more than HL_DISTANCE_WIDE_CELLS cells: kept in a list every query tests, in
 *     index order), counts[3] = valid triangles.  counts: 4 device int64, *status a device int32, both cleared first.
 *   hl_mesh_distance_fill (scratch as left by the count stage, n_refs = its reference total, at most 2^31): refs int32 (n_refs), caller-owned.
 *   hl_mesh_distance_query (n_wide = counts[2], at most HL_DISTANCE_MAX_WIDE; max_distance +inf for none): per query sqdist, distance =
 *     sqrt(sqdist), triangle int32, barycentric (Q,3), point (Q,3) world, and with normals (Q,3) normal_dot (Q) (both or neither).  A query
 *     farther than max_distance gets +inf and -1.  *status is or-ed into, not cleared.
 *   hl_mesh_distance_sample (prefix and total from the areas stage, total >= 1): sample s of S lies in the triangle that holds position
 *     floor((s + 0.5) / S * total) of the prefix, at the barycentrics of the R2 sequence's term seed * 2^32 + s + 1.
 *   hl_mesh_distance_reduce: out[0..15] = sum of distance, sum of sqdist, sum of the finite normal_dot, their count, max distance, count of
 *     finite distances, two spare, then the counts of distance <= threshold[k]; non-finite distances count nowhere.  out:
 *     HL_DISTANCE_REDUCE_WORDS device doubles (the rest holds partials); h_thresholds: HOST doubles.  Fixed order: the same bits every run.
 * scratch: hl_mesh_distance_scratch_bytes(T, gx, gy, gz) bytes, 16-byte aligned, every part rounded up to 16 bytes: the records, fp64
 *     (T, HL_DISTANCE_RECORD_WORDS): a b c relative to the origin and a zero; the flags int32 (T): 0 dropped, 1 registered, 2 wide; the cell
 *     starts uint32 (cells + 1); the fill cursors uint32 (cells); the wide list int32 (HL_DISTANCE_MAX_WIDE); the scans' block sums.  0 for
 *     refused sizes.
 * Refused before any launch (HL_ERR_INVALID): N, T, Q or S < 1 or >= 2^31, a cell that is not positive and finite, a non-finite origin, an
 *     extent < 1, more than 2^27 cells, more than 2^31 references, more than HL_DISTANCE_MAX_WIDE wide triangles, more than 8 thresholds. */
#define HL_DISTANCE_WIDE_CELLS 4096
#define HL_DISTANCE_MAX_WIDE 65536
#define HL_DISTANCE_RECORD_WORDS 10
#define HL_DISTANCE_REDUCE_BLOCKS 1024
#define HL_DISTANCE_REDUCE_FIELDS 16
#define HL_DISTANCE_REDUCE_WORDS (HL_DISTANCE_REDUCE_FIELDS + HL_DISTANCE_REDUCE_FIELDS * HL_DISTANCE_REDUCE_BLOCKS)
size_t hl_mesh_distance_scratch_bytes(int64_t T, int64_t gx, int64_t gy, int64_t gz);
int hl_mesh_distance_areas(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, double unit, int64_t *prefix,
                           int64_t *counts, void *blocks, size_t blocks_bytes, void *stream);
int hl_mesh_distance_count(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy,
                           int64_t gz, int64_t *counts, int32_t *status, void *scratch, size_t scratch_bytes, void *stream);
int hl_mesh_distance_fill(int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy, int64_t gz, int32_t *refs, int64_t n_refs, void *scratch,
                          size_t scratch_bytes, void *stream);
int hl_mesh_distance_query(const double *points, const double *normals, int64_t Q, int64_t T, const double *h_origin, double h, int64_t gx, int64_t gy,
                           int64_t gz, const int32_t *refs, int64_t n_refs, int64_t n_wide, double max_distance, double *sqdist, double *distance,
                           int32_t *triangle, double *barycentric, double *point, double *normal_dot, int32_t *status, const void *scratch,
                           size_t scratch_bytes, void *stream);
int hl_mesh_distance_sample(const double *vertices, int64_t N, const int32_t *triangles, int64_t T, const double *h_origin, const int64_t *prefix,
                            int64_t total, int64_t S, uint64_t seed, double *points, int64_t *triangle, double *barycentric, double *normals, void *stream);
int hl_mesh_distance_reduce(const double *distance, const double *sqdist, const double *normal_dot, int64_t Q, const double *h_thresholds, int n_thresholds,
                            double *out, void *stream);

/* ---- FID: pytorch-fid's InceptionV3 pool3 features and the float64 moments of a feature set ----
 * Contract: DESIGN.md 4l "FID"; csrc/hl_fid.hip.  Contiguous fp32 images, enqueue-only on `stream`, caller-owned workspace and state,
 * exact fp32 products, no atomics: the same bits every run, and an image's features do not depend on the batch it is in.  The
 * architecture has not been checked against pytorch-fid's own weights.
 *   hl_fid_layer: row i of the layer table (the HL_FID_LAYERS BasicConv2d in the order the forward runs them): its state-dict name
 *     ("Mixed_5b.branch1x1"; at most 39 characters) and desc[8] = Cin, Cout, kH, kW, sH, sW, pH, pW.
 *   params: per layer, BatchNorm (eps 1e-3) folded in by the caller: conv_w[l] packed as (kH kW, ceil(Cin / 16), CoutP, 16) - tap, chunk of
 *     16 input channels, output channel, channel within the chunk - with CoutP = Cout rounded up to 32 and zeros in all padding; conv_b[l]
 *     (Cout).  16-byte aligned.
 *   hl_fid_features: in (N, 3, h, w) in [0, 1], only read.  resize: bilinear to 299 x 299 (align_corners = False, no antialiasing);
 *     normalize: 2 x - 1.  The four block outputs stay in the workspace as NHWC tensors (N, h_k, w_k, C_k), C_k = 64, 192, 768, 2048 (the
 *     last one 1 x 1: the pool3 features), at the offsets hl_fid_block_shape gives for (N, h, w, resize); out (N, 2048), if not NULL,
 *     receives the pool3 features as well.
 *   1 <= N <= 4096; h, w <= 16384, and >= 75 without resize; workspace: hl_fid_workspace_bytes(N, h, w, resize) (0: bad shape).
 *   Moments: state = HL_FID_STATE_BYTES, zeroed by the caller before the first update: S (2048, 2048) float64, of which the 64 x 64
 *     tiles on and above the diagonal are kept, then s (2048) float64.  hl_fid_moments_update adds the n rows of features (n, 2048)
 *     strictly in order: s[i] += x[i], S[i][j] += x[i] x[j], the product and the sum rounded separately - so the state does not depend
 *     on how the images were split into updates.  The caller keeps the count.  hl_fid_moments_finalize(count >= 2): mu = s / count,
 *     sigma[i][j] = (S[i][j] - (count mu[i]) mu[j]) / (count - 1) for i <= j, each operation rounded separately, mirrored below the diagonal. */
#define HL_FID_LAYERS 94
#define HL_FID_DIMS 2048
#define HL_FID_STATE_BYTES ((size_t)HL_FID_DIMS * HL_FID_DIMS * 8 + (size_t)HL_FID_DIMS * 8)
typedef struct hl_fid_params {
    const float *conv_w[HL_FID_LAYERS];
    const float *conv_b[HL_FID_LAYERS];
} hl_fid_params;
int hl_fid_layer(int i, char *name, int name_bytes, int *desc);
size_t hl_fid_workspace_bytes(int N, int h, int w, int resize);
int hl_fid_block_shape(int N, int h, int w, int resize, int k, size_t *offset_bytes, int *hk, int *wk, int *channels);
int hl_fid_features(const hl_fid_params *params, const float *in, int N, int h, int w, int resize, int normalize, float *out, void *workspace,
                    size_t workspace_bytes, void *stream);
int hl_fid_moments_update(void *state, const float *features, int n, void *stream);
int hl_fid_moments_finalize(const void *state, int64_t count, double *mu, double *sigma, void *stream);

/* ---- Feature metrics: KID, k-NN radii and the precision / recall manifold pass on two feature sets, pairwise in float64 ----
 * Contract: DESIGN.md 4m "Feature metrics"; csrc/hl_feature_metrics.hip.  x (N, D), y (M, D) row-major fp32, any N, M, D >= 1, only read;
 * enqueue-only on `stream`, caller-owned workspace of hl_feat_workspace_bytes(op, N, M, S, m, split) bytes (0: bad sizes), 16-byte aligned.
 *   g(a, b) = sum_k (double)a_k (double)b_k, added for k = 0 .. D - 1 in that order, one rounding per k (the fp32 product is exact): a
 *     function of the two rows' contents alone, symmetric bit for bit, the same bits every run.  d2(a, b) = max(0, (g(a,a) + g(b,b)) - 2 g(a,b)),
 *     each operation rounded separately: exactly 0 for bit-equal rows.
 *   hl_feat_pairwise: out (N, M) float64 = g (HL_FEAT_GRAM) or d2 (HL_FEAT_D2).
 *   hl_feat_kid: x_index, y_index (S, m) int32 rows of x and of y (an index outside its set counts as a row of zeros; the caller checks).
 *     k(a, b) = (g(a,b) / D + 1)^3, each operation rounded separately.  Per subset: sxx = sum_{i != j} k(x_i, x_j), syy likewise, sxy =
 *     sum_{i, j} k(x_i, y_j) (i, j positions in the subset), as 64 x 64 tile partials in the workspace added in the fixed order of
 *     hl_reduce.h; out[s] = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2.  2 <= m <= min(N, M), 1 <= S <= 65535.
 *   hl_feat_knn_radii: r2[i] = the k-th smallest d2(x_i, x_j) over j != i (by position: a duplicate row stays, at 0).  1 <= k <=
 *     HL_FEAT_MAX_K, k < N.  The columns are cut into `split` chunks (<= 0: the library's rule, hl_feat_split) whose k-lists a second
 *     kernel merges; the result does not depend on the split.
 *   hl_feat_manifold: hits_fake[j] = #{i : d2(r_i, f_j) <= r2_real[i]} (M) int32, hits_real[i] = #{j : d2(r_i, f_j) <= r2_fake[j]} (N) int32,
 *     nearest_real[i] = min_j d2(r_i, f_j) (N) float64; all three are initialised here.  `split` as above. */
#define HL_FEAT_MAX_K 8
#define HL_FEAT_GRAM 0
#define HL_FEAT_D2 1
#define HL_FEAT_OP_PAIRWISE 0
#define HL_FEAT_OP_KID 1
#define HL_FEAT_OP_KNN 2
#define HL_FEAT_OP_MANIFOLD 3
size_t hl_feat_workspace_bytes(int op, int64_t N, int64_t M, int64_t S, int64_t m, int split);
int hl_feat_split(int64_t rows, int64_t cols, int split);
int hl_feat_pairwise(const float *x, int64_t N, const float *y, int64_t M, int64_t D, int kind, double *out, void *workspace, size_t workspace_bytes,
                     void *stream);
int hl_feat_kid(const float *x, int64_t N, const float *y, int64_t M, int64_t D, const int32_t *x_index, const int32_t *y_index, int64_t S, int64_t m,
                double *out, void *workspace, size_t workspace_bytes, void *stream);
int hl_feat_knn_radii(const float *x, int64_t N, int64_t D, int k, int split, double *r2, void *workspace, size_t workspace_bytes, void *stream);
int hl_feat_manifold(const float *real, int64_t N, const float *fake, int64_t M, int64_t D, const double *r2_real, const double *r2_fake, int split,
                     int32_t *hits_fake, int32_t *hits_real, double *nearest_real, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HUMANLIFF_HIP_H */
