/*
 * sixdgs.h -- C ABI of the MI355X-native 6DGS pose-estimation hot path (lib6dgs_hip.so).
 *
 * The reference (mbortolon97/6dgs) has NO FFI on this path: it is pure Python/PyTorch behind three
 * callables (generate_all_possible_rays, IdentificationModule.test_image, test_pose_estimation).
 * This header is the boundary a maintainer would bind from those callables (ctypes stub shown in
 * INTEGRATION.md); every entry point names the reference code it replaces (paths relative to the
 * reference root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer into caller-owned memory (the PyTorch caching allocator in
 *    the shipped host shim) unless the name starts with h_; the library allocates nothing
 *    persistent and keeps no mutable global state;
 *  - all tensors are fp32 row-major contiguous, indices int64, masks uint8, as in the reference;
 *  - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and re-entrant;
 *  - scratch memory comes from the caller: query *_workspace_bytes, pass `ws` (256-B aligned);
 *  - return value: 0 = ok, <0 = SIXDGS_E_* argument error, >0 = hipError_t of a failed launch.
 *    No exceptions cross the ABI.  The Python shim raises RuntimeError on non-zero (the only
 *    exception type the reference driver catches, pretrain_eval_attention.py:243-244);
 *  - ragged outputs are written into caller-sized buffers and their length is returned through a
 *    device int64 (the caller syncs to read it, as the reference does at sampling.py:145).
 */
#ifndef SIXDGS_H
#define SIXDGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIXDGS_ABI_VERSION 10   /* 10: sixdgs_splat_views / sixdgs_splat_views_workspace_bytes (synthetic query views: the scene's Gaussians as z-buffered flat discs); 9: sixdgs_score_backward_split / sixdgs_score_backward_split_workspace_bytes (the scorer backward split over ray groups); 8: sixdgs_score_backward / sixdgs_score_backward_workspace_bytes (backward of the scorer for training); 7: sixdgs_image_prep (uint8 -> resized, cropped, normalised planar fp32 in one pass); 6: sixdgs_tok_pack / sixdgs_tok_linear (dense products of the backbone stage on packed weight planes, with LayerNorm / GELU / residual fusion), sixdgs_tok_attention, sixdgs_im2col, sixdgs_u8_to_planar; the three-plane bf16 key format and its scorer kernel removed (sixdgs_split_planes, sixdgs_key_planes_bytes gone; key planes exist as scaled fp16 only); 5: sixdgs_scorer_weights carries the composite layer w4k / b4k / m4k (k_proj folded into ray-MLP layer 4 on the key-cache path), sixdgs_select_begin / _sample_stats take h_n_tok (token packing of the select sweep); 4: the select path's slack derived from |q| |k| (sixdgs_key_planes_norm_max; q + d_key_norm_max arguments) and its ray-sharded form (sample_stats / prepare / topk_u, d_uk, allow_fewer), tile maxima of U (u_tile_max); 3: sixdgs_score_select + sixdgs_select_* stages (top-k without materialised logits); 2: plane-format scorer entry points, pass1/pass2, grid kNN, split-K, distance target */
#define SIXDGS_E_BADARG (-1)
#define SIXDGS_E_WORKSPACE (-2)
#define SIXDGS_E_UNSUPPORTED (-3)

#define SIXDGS_D 384        /* embed dim (backbone.py:17, identification_module.py:44-46) */
#define SIXDGS_RAY_IN 141   /* RayPreprocessor input width (ray_preprocessor.py:15) */
#define SIXDGS_RAY_IN_PAD 144
#define SIXDGS_HID 512      /* featureC (identification_module.py:16-18) */
#define SIXDGS_TOK_IN 398   /* img_num_features + 14 (identification_module.py:20) */
#define SIXDGS_MAX_TOKENS 256

typedef void* sixdgs_stream_t;

/* How the fp32 contractions are evaluated on the matrix cores (results agree to fp32 rounding):
 *   F32     v_mfma_f32_32x32x2_f32: exact fp32 fma chain, 157 TFLOP/s peak;
 *   BF16X6  each fp32 operand split into 3 bf16 planes, the 6 leading cross terms accumulated in fp32 by
 *           v_mfma_f32_32x32x16_bf16: per-product error <= 2^-26 (below fp32 rounding), 2.67x less
 *           matrix-pipe time. */
#define SIXDGS_MMA_DEFAULT (-1)
#define SIXDGS_MMA_F32 0
#define SIXDGS_MMA_BF16X6 1
/*   F16X3   (scorer logits only) every 128-row tile of an operand scaled by a power of two and split into 2 fp16 planes,
 *           3 cross terms on v_mfma_f32_32x32x16_f16: measured error 1.0e-7 sum|a||b| (below the fp32 chain), half the
 *           MFMA work of BF16X6 and fp32-sized operands; the dense layers run BF16X6 in this mode.
 *   DEFAULT = F16X3 (scorer) + BF16X6 (dense layers). */
#define SIXDGS_MMA_F16X3 2
/*   F16X3_L32  as F16X3, but the logits travel between the two scorer passes as fp32 (1 KiB per ray and image).  F16X3
 *           stores them as 24-bit fixed point of (lane maximum - logit), resolution 2^-19 (absolute error <= 2^-20 per logit,
 *           the fp32 rounding of a logit of magnitude 16; measured effect on the scores <= 5e-7 relative): 768 B per ray and
 *           image through HBM twice, the largest data stream of the path.  The grid ends at 2^24 - 1 steps: a logit more than
 *           32 below the lane maximum (the largest logit of that token among the lane's 64 rays of the 128-ray tile) is stored
 *           as that maximum minus 32.  The score of such a ray is therefore too LARGE, never too small: by at most
 *           e^-32 * sum_t max_{r' in the 128-ray tile of r} softmax_r'(token t), i.e. e^-32 of the tile's largest term per token.
 *           Such rays carry no weight in the pose; with a single token and a logit spread beyond 32 the ORDER among rays of that
 *           size can differ from F16X3_L32's (tests/test_gpu_two_pass_edges.py: test_clamp). */
#define SIXDGS_MMA_F16X3_L32 3

/* Optional kernel timing, owned by the caller (the library stays stateless): zero-initialise, pass to
 * the *_ex entry points; each launch of the dominant kernel is bracketed by a pair of HIP events on
 * the launch stream and its algorithmic FLOP count recorded.  sixdgs_profile_collect waits for the
 * events, sums milliseconds and FLOPs, destroys the events and resets the struct. */
#define SIXDGS_PROFILE_SLOTS 128
typedef struct sixdgs_profile {
  int count;
  void* start[SIXDGS_PROFILE_SLOTS];
  void* stop[SIXDGS_PROFILE_SLOTS];
  double flops[SIXDGS_PROFILE_SLOTS];
  double bytes[SIXDGS_PROFILE_SLOTS];
} sixdgs_profile;
int sixdgs_profile_collect(sixdgs_profile* prof, double* ms_total, double* flops_total, double* bytes_total, int* launches);

int sixdgs_abi_version(void);
const char* sixdgs_error_string(int status);

/* ---------------------------------------------------------------------------------------------
 * Scene-side geometry (once per scene) -- replaces pose_estimation/sampling.py:127-267
 * ------------------------------------------------------------------------------------------- */

/* a2: mask_degraded_ellipsoids (quadricell.py:171-188) on scale = exp(log_scale)
 * (scene/gaussian_model.py:125-127).  mask[i] = total_rings(i) < target_points. */
int sixdgs_mask_degraded(const float* log_scale /*[N,3]*/, int64_t n, int target_points, uint8_t* mask /*[N]*/,
                         sixdgs_stream_t stream);

/* a5: sym_eig_3x3 (sym_eig_3x3.py:246-307), eigenvectors in the columns of vecs (may be NULL). */
int sixdgs_sym_eig_3x3(const float* mats /*[n,3,3]*/, int64_t n, float* vals /*[n,3]*/, float* vecs /*[n,3,3]*/,
                       sixdgs_stream_t stream);

/* a4: compute_normals (sampling.py:62-113): k nearest neighbours of each query in `cloud` (self
 * included), centred scatter matrix, smallest-eigenvalue eigenvector, sign by majority vote.
 * Brute force, exact; ties in distance -> lowest index.  knn (may be NULL) receives the neighbour
 * indices sorted by distance.  k <= 32. */
int sixdgs_normals_knn(const float* query /*[nq,3]*/, int64_t nq, const float* cloud /*[E,3]*/, int64_t e, int k,
                       float* normals /*[nq,3]*/, int64_t* knn /*[nq,k] or NULL*/, sixdgs_stream_t stream);
/* The same result (neighbour lists and normals bit for bit) through a uniform grid: O(E) instead of O(E^2), for
 * full-scene emission (the reference only ever runs a4 on 1000 ellipsoids).  Workspace: counting-sort buffers. */
size_t sixdgs_normals_knn_grid_workspace_bytes(int64_t e);
int sixdgs_normals_knn_grid(const float* query, int64_t nq, const float* cloud, int64_t e, int k, float* normals, int64_t* knn,
                            void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* a1+a6+a7+a10, quadricell emitter (quadricell.py:191-386 with direction_mode="isocell", SH colour
 * sampling.py:116-124,225-251).  Ellipsoid j of the emission set is Gaussian sel[j] (sel == NULL:
 * j itself); its rays are written contiguously in ellipsoid -> ring -> cell order.
 *   phase 1 (count): d_counts[j] = rays kept for ellipsoid j, d_offsets[j] = exclusive prefix,
 *                    d_total[0] = total rays, d_total[1] = total cells before the hemisphere mask;
 *   phase 2 (write): fills ori/dir/rgb/src (src = Gaussian index of each ray) using d_offsets.
 * f_dc [N,1,3] and f_rest [N,ncoef-1,3] are the raw SH tensors (gaussian_model.py:146-150).
 * `normals` [E,3] are per emission-set ellipsoid. */
/* `scale` is [N,3]: the raw log-scales of the 3DGS checkpoint when scale_is_log != 0 (the kernel
 * applies exp, gaussian_model.py:125-127), already-activated semi axes otherwise. */
int sixdgs_emit_quadricell_count(const float* xyz, const float* scale, int scale_is_log, const float* rot,
                                 const int64_t* sel, int64_t e, const float* normals, int target_points,
                                 int table_res, int64_t* d_counts /*[E]*/, int64_t* d_offsets /*[E]*/,
                                 int64_t* d_total /*[2]*/, sixdgs_stream_t stream);
int sixdgs_emit_quadricell_write(const float* xyz, const float* scale, int scale_is_log, const float* rot,
                                 const float* f_dc, const float* f_rest, int sh_degree, int n_coef,
                                 const int64_t* sel, int64_t e, const float* normals, int target_points,
                                 int table_res, const int64_t* d_offsets, float* ori, float* dir, float* rgb,
                                 int64_t* src, sixdgs_stream_t stream);
/* a6 alone (cell centres in the local frame + ellipsoid id), used by the parity tests:
 * count -> d_counts/d_offsets/d_total[0]; then centres. */
int sixdgs_quadricell_cell_counts(const float* scale /*[E,3] activated*/, int64_t e, int target_points,
                                  int64_t* d_counts, int64_t* d_offsets, int64_t* d_total, sixdgs_stream_t stream);
int sixdgs_quadricell_centers(const float* scale /*[E,3] activated*/, int64_t e, int target_points, int table_res,
                              const int64_t* d_cell_offsets /*[E]*/, float* points, int64_t* ellipsoid_id,
                              sixdgs_stream_t stream);

/* a8: isocell_distribution(ray_target, N0, isrand=-1) (isocell.py:6-84).  Returns the number of
 * directions N0*ceil(sqrt(target/N0))^2 via *h_count when dirs == NULL. */
int sixdgs_isocell_distribution(int ray_target, int n0, float* dirs /*[K,3]*/, int64_t* h_count,
                                sixdgs_stream_t stream);
/* a9: rotate_isocell (isocell.py:171-222): out[e][k] = Rodrigues(z -> normal_e) * dirs[k];
 * NaN when the normal is (anti)parallel to z, as the reference. */
int sixdgs_rotate_isocell(const float* dirs, int64_t k, const float* normals, int64_t e, float* out /*[E,K,3]*/,
                          sixdgs_stream_t stream);
/* iso-cell emitter for "every Gaussian" mode (BASELINE.json configs "64/256 isocell rays per
 * ellipsoid"; not on the reference's live path): ray (j,k): dir = rotate_isocell(dirs[k], n_j),
 * ori = centre_j + the ellipsoid surface point along dir, rgb = SH colour at -dir.  E*K rays. */
int sixdgs_emit_isocell(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* f_dc,
                        const float* f_rest, int sh_degree, int n_coef, const int64_t* sel, int64_t e,
                        const float* normals, const float* dirs, int64_t k, float* ori, float* dir, float* rgb,
                        int64_t* src, sixdgs_stream_t stream);
/* a10 alone: evaluate_viewdirs_color (sampling.py:116-124) for sh [R,3,ncoef] */
int sixdgs_eval_sh_color(const float* sh, int n_coef, const float* dirs, int64_t r, int sh_degree, float* rgb,
                         sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Synthetic query views (ABI 10): the scene's Gaussians as flat, z-buffered discs.  A stand-in view
 * generator whose images depend on the camera the way a real scene's do -- NOT the 3DGS rasteriser
 * (no blending, no anisotropic footprint, no anti-aliasing, no gradients).  All arithmetic in fp32:
 *  1. per view and Gaussian i: p = W xyz_i + t with [W | t] the view's w2c; skipped unless p.z > near_z;
 *  2. u = fx p.x / p.z + cx, v = fy p.y / p.z + cy, r = max(extent * max(semi axes of i) * fx / p.z, 0.7072)
 *     (the floor: every visible Gaussian covers at least the pixel its centre falls into);
 *  3. i covers pixel (x, y) when (x + 0.5 - u)^2 + (y + 0.5 - v)^2 <= r^2; the whole disc has depth p.z;
 *  4. a pixel's winner is the covering Gaussian of smallest p.z, equal p.z -> smaller index: the same
 *     input gives the same bytes on every call;
 *  5. colour of the winner: round(255 min(c, 1)) per channel, c = the emitters' SH colour (a10: + 0.5, clamped
 *     at 0) for view direction normalize(xyz_i - camera centre) -- the colour of a ray that leaves
 *     Gaussian i towards the camera.  Pixels without a winner get `background`; with channels == 4 alpha
 *     is 255 on covered pixels and 0 elsewhere;
 *  6. winner (may be NULL) receives the winning index, -1 where there is none.
 * The scene arrays are the emitters' (scale [N,3], logs when scale_is_log != 0; f_dc [N,1,3], f_rest
 * [N,n_coef-1,3]); cams and background are DEVICE arrays; n < 2^31, width, height <= 16384, views <= 65535,
 * extent > 0, near_z >= 0.  Workspace: the 64-bit depth buffer and one packed colour per view and Gaussian. */
size_t sixdgs_splat_views_workspace_bytes(int64_t n, int views, int width, int height);
int sixdgs_splat_views(const float* xyz, const float* scale, int scale_is_log, const float* f_dc, const float* f_rest,
                       int sh_degree, int n_coef, int64_t n,
                       const float* cams /*[views][16]: w2c rows 0..2 (12 floats), fx, fy, cx, cy*/, int views, int width,
                       int height, int channels /*3 or 4*/, float extent, float near_z,
                       const float* background /*[3], in [0,1]*/, uint8_t* image /*[views][height][width][channels]*/,
                       int32_t* winner /*[views][height][width] or NULL*/, void* ws, size_t ws_bytes,
                       sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scene views by the alpha-blended 3DGS forward rasteriser (additive in ABI 10; its gradients: sixdgs_raster_views_backward below).  With
 * cx = width / 2, cy = height / 2 this is the image of the reference's rasteriser call in gaussian_renderer/__init__.py
 * (prefiltered = False, SHs converted inside).  The tile is 16 x 16 pixels and is PART OF THE DEFINITION: the grid is
 * gx = ceil(width / 16), gy = ceil(height / 16).  All arithmetic in fp32.  Per view (one row of cams) and Gaussian i:
 *   1. p = W xyz_i + t with [W | t] the view's w2c; culled unless p.z > 0.2;
 *   2. Sigma = R S S^T R^T, R = the rotation of rot_i = (w, x, y, z) (normalised, as the emitters do), S = diag(scale_modifier s_i),
 *      s_i = exp(scale_i) when scale_is_log != 0, scale_i otherwise;
 *   3. tanx = width / (2 fx), tany = height / (2 fy); tx = clamp(p.x / p.z, +-1.3 tanx) p.z, ty likewise;
 *      J = [[fx / p.z, 0, -fx tx / p.z^2], [0, fy / p.z, -fy ty / p.z^2]]; cov = (J W) Sigma (J W)^T;
 *      a = cov00 + 0.3, b = cov01, c = cov11 + 0.3;
 *   4. det = a c - b^2, culled when det == 0; conic = (c / det, -b / det, a / det);
 *   5. mid = (a + c) / 2, lambda = mid + sqrt(max(0.1, mid^2 - det)), radius = ceil(3 sqrt(lambda)) (stored saturated at 2^30);
 *   6. centre u = fx p.x / p.z + cx, v = fy p.y / p.z + cy; the centre of pixel (x, y) is (x + 0.5, y + 0.5);
 *   7. tile rectangle on (u - 0.5, v - 0.5): x0 = clamp(int((u - 0.5 - radius) / 16), 0, gx),
 *      x1 = clamp(int((u - 0.5 + radius + 15) / 16), 0, gx), y0 and y1 likewise with gy (int() truncates towards zero); culled when
 *      (x1 - x0)(y1 - y0) == 0.  Gaussian i CONTRIBUTES ONLY TO PIXELS OF TILES IN [x0, x1) x [y0, y1);
 *   8. colour = the emitters' SH colour (a10: + 0.5, clamped below at 0, not above) for direction normalize(xyz_i - camera centre);
 *   9. o = sigmoid(opacity_i) when opacity_is_logit != 0, opacity_i otherwise;
 *  10. per pixel the contributing Gaussians are ordered by ascending bits of p.z, equal bits -> the smaller index first;
 *  11. blend: T = 1, C = 0, then in that order: d = (u - x - 0.5, v - y - 0.5),
 *      power = -0.5 (conic.x d.x^2 + conic.z d.y^2) - conic.y d.x d.y; skip when power > 0; alpha = min(0.99, o exp(power)); skip when
 *      alpha < 1/255; T' = T (1 - alpha); when T' < 1e-4 stop (this Gaussian is not added); otherwise C += colour alpha T, T = T'.
 *      Pixel = C + T background, alpha = 1 - T.
 * Outputs, each may be NULL: image_f32 [views][height][width][4] (rgb, 1 - T); image_u8 [views][height][width][channels], channels 3 or
 * 4, round(255 clamp(., 0, 1)); radii [views][n] int32, 0 = culled.  The same input gives the same bytes on every call, and a view's
 * image does not depend on the other views of the call.
 *
 * A (view, Gaussian) pair takes one INSTANCE per tile of its rectangle.  The caller sizes the instance buffers with max_instances
 * (>= 1); `instances` (device, may be NULL) receives the number the scene needs.  When that exceeds max_instances nothing is written
 * out of bounds, the later kernels read the count on the device and return, and the images are unspecified (radii are still written):
 * call again with max_instances >= *instances.  The sort always runs over max_instances slots, so a tight value is also the fast one.
 * Limits: n < 2^31, views <= 65535, width, height <= 16384, views gx gy < 2^31, max_instances < 2^31, scale_modifier > 0.
 * sixdgs_raster_views_workspace_bytes is answered without touching a GPU (0 for sizes outside the limits): the per-(view, Gaussian)
 * records (64 B), the tile ranges, two key and two index buffers of max_instances (24 B per instance) and the temporary storage of
 * the library scan and sort, reserved by a bound (1 MiB + 2 B per record, 1 MiB + 16 B per instance); if the installed rocPRIM asks
 * for more the call returns SIXDGS_E_WORKSPACE.  SIXDGS_E_BADARG without a launch for argument errors; views == 0 returns 0; with n == 0
 * the image is the background.  prof (may be NULL) receives one slot per stage: project, scan, emit, sort, ranges, blend. */
size_t sixdgs_raster_views_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances);
int sixdgs_raster_views(const float* xyz, const float* scale, int scale_is_log, const float* rot /*[N,4] (w,x,y,z)*/,
                        const float* opacity /*[N]*/, int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree,
                        int n_coef, int64_t n, const float* cams /*[views][16]: w2c rows 0..2 (12 floats), fx, fy, cx, cy*/,
                        int views, int width, int height, float scale_modifier, const float* background /*[3] device*/,
                        float* image_f32, uint8_t* image_u8, int channels /*3 or 4*/, int32_t* radii, int64_t max_instances,
                        int64_t* instances /*[1] device or NULL*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                        sixdgs_profile* prof);

/* ---------------------------------------------------------------------------------------------
 * The rasteriser's backward (additive in ABI 10): the derivative of image_f32 of sixdgs_raster_views by every Gaussian parameter and
 * by the camera rows.  Given grad_image [views][height][width][4] = dL / d image_f32 (rgb and 1 - T), each output is the sum over views
 * and pixels of grad_image . d image_f32 / d theta, where image_f32 is the function of steps 1 - 11 above with EVERY DISCRETE OUTCOME
 * HELD AT WHAT THE FORWARD TOOK: the culls of steps 1, 4 and 7; the radius and the tile rectangle (a Gaussian has no gradient from
 * pixels outside its rectangle); the order of step 10; the two skips and the stop of step 11.  The Gaussian that triggers the stop, and
 * everything behind it, gets nothing from that pixel; the T in C + T background and in 1 - T is the T before the stopping Gaussian.
 * Continuous clamps differentiate as clamps, with derivative 0 where they act: min(0.99, o exp(power)); the +-1.3 tan clamp of
 * p.x / p.z and p.y / p.z in step 3 (tx then depends on p.z only through the product, and on fx through tanx); max(colour + 0.5, 0);
 * the 1e-12 floors of the quaternion normalisation and of the view direction.  Differentiated through: both quaternion normalisations
 * of step 2; the normalisation of the view direction, so the colour's dependence on xyz and on the camera centre -W^T t counts; exp of
 * the scale when scale_is_log; the sigmoid when opacity_is_logit.  scale_modifier and background are constants; behaviour exactly at a
 * clamp's edge is unspecified; the uint8 image has no gradient.  All arithmetic in fp32.
 *
 * Per pixel, with 1 - T taken as a fourth channel of colour 1 and background 0, so that channel_ch = sum_j c_j,ch alpha_j T_j +
 * T_fin bg_ch over the Gaussians j the pixel blended (T_j = the T before j, T_fin = the final T) and g = the pixel's grad_image:
 *   dL / d alpha_j = sum_ch g_ch (c_j,ch T_j - R_j,ch / (1 - alpha_j)),  R_j,ch = sum_{k > j} c_k,ch alpha_k T_k + T_fin bg_ch,
 *   dL / d c_j,ch  = g_ch alpha_j T_j for the three real channels,
 * walked back to front: R accumulates, T_j = T_{j+1} / (1 - alpha_j).  Where alpha_j is not clamped, d alpha_j / d o = exp(power) and
 * d alpha_j / d power = alpha_j; power gives d u, d v and d conic.  Per (view, Gaussian) these nine numbers (d u, d v, 3 conic, d o,
 * 3 colour) are summed over the pixels of a tile in a fixed tree (the 256 pixels in 4 groups of 64 rows-of-16 order, within a group
 * x += x_(l xor s), s = 32 .. 1, then the groups in order; a group none of whose pixels blended j is left out), then over the tiles of
 * the rectangle in rectangle order, then chained through steps 9 .. 1 to the parameters.
 *
 * Outputs, each may be NULL, WRITTEN, NOT ACCUMULATED: d_xyz [n,3]; d_scale [n,3] with respect to the array as given (log or not);
 * d_rot [n,4]; d_opacity [n] (logit or not); d_f_dc [n,1,3]; d_f_rest [n,n_coef-1,3] (zeros for coefficients above sh_degree);
 * d_cams [views][16]: the 12 w2c entries as free numbers, then fx, fy, cx, cy.  A Gaussian that contributes to no pixel gets exact zeros.
 * SAME INPUT, SAME BYTES: no floating-point atomics anywhere.  VIEWS DO NOT MIX: row v of d_cams is the same bits whether view v is
 * differentiated alone or in a batch (per view: Gaussians in blocks of 256, the fixed tree inside a block, then the blocks in order),
 * and a Gaussian's gradient over a batch is its per-view gradients, each chained to parameter space within its view, added in ascending
 * view order: ((g_0 + g_1) + g_2) ...
 *
 * fwd_ws is the workspace of a COMPLETED sixdgs_raster_views call with the same scene, cams, sizes, scale_modifier and max_instances,
 * whose instance count fitted, not written since (whether that call produced an image does not matter).  The backward reads from it the
 * per-(view, Gaussian) records, the rectangles, the scanned offsets, the tile ranges and the sorted indices (the forward leaves a word
 * in it that says which of its two index buffers holds them) -- no second sort; the library stays stateless and fwd_ws is not
 * written.  If the recorded total exceeds max_instances the kernels read that on the device and return; the outputs are then
 * unspecified.  views == 0 returns 0; n == 0 writes zero d_cams.  Limits and argument errors are the forward's, plus NULL grad_image /
 * fwd_ws and too small a fwd_ws_bytes: SIXDGS_E_BADARG / SIXDGS_E_WORKSPACE without touching a GPU.  Two calls on the same inputs may
 * run concurrently on different streams with different ws.  Workspace (answered without a GPU, 0 outside the limits): 36 B per
 * instance (max_instances x 9 floats) + 64 B per view and block of 256 Gaussians.  prof (may be NULL) receives one slot per stage:
 * blend_bwd, project_bwd, cams. */
size_t sixdgs_raster_views_backward_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances);
int sixdgs_raster_views_backward(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity,
                                 int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n,
                                 const float* cams, int views, int width, int height, float scale_modifier,
                                 const float* background /*[3] device*/, const float* grad_image /*[views][height][width][4]*/,
                                 int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes, float* d_xyz, float* d_scale,
                                 float* d_rot, float* d_opacity, float* d_f_dc, float* d_f_rest, float* d_cams /*[views][16]*/,
                                 void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof);

/* ---------------------------------------------------------------------------------------------
 * Every Gaussian's contribution to views (additive in ABI 10): what step 11 of sixdgs_raster_views computes per (pixel, Gaussian) and
 * drops -- alpha T -- kept per (view, Gaussian), with the number of pixels that added the Gaussian and the number it stopped.  A direct
 * measurement: no gradient, no colour, no clamp in the way.  All arithmetic in fp32.
 *
 * fwd_ws is the workspace of a COMPLETED sixdgs_raster_views call with the same n, views, width, height and max_instances, whose
 * instance count fitted, not written since (whether that call produced an image does not matter; the scene and cams are in fwd_ws
 * already and are not passed again).  For view v and pixel (x, y) inside the image the walk of step 11 is repeated operation by
 * operation over the same ordered list, so that every skip and the stop fall exactly where the forward's did:
 *   1. d, power, the skip when power > 0, alpha = min(0.99, o exp(power)), the skip when alpha < 1/255, T' = T (1 - alpha);
 *   2. when T' < 1e-4 the pixel stops: Gaussian j is counted as a STOP of this pixel and adds nothing;
 *   3. otherwise the pixel ADDS j: w = alpha T, one fp32 product, T the value before j; then T = T'.
 * Per (view v, Gaussian i), over the pixels of the tiles of i's rectangle (step 7):
 *   weight_vi = the sum of w.  Within a tile in the backward's fixed tree: the 256 pixels in 4 groups of 64 in rows-of-16 order, within
 *               a group x += x_(l xor s), s = 32 .. 1, then the groups in order; a pixel that does not add i (skipped, stopped, or
 *               outside the image) counts as 0.f.  Then the tiles in rectangle order, from 0.f;
 *   peak_vi   = the largest w (exact: it does not depend on any order), 0.f when there is none;
 *   pixels_vi = the number of pixels that added i (int32);   stops_vi = the number of pixels i stopped (int32).
 * Outputs, each may be NULL, [n] arrays, READ, UPDATED AND WRITTEN BACK over the views in ascending order, like sixdgs_densify_stats --
 * the caller zeroes them, and a result does not depend on how the views are cut into calls:
 *   weight (fp32)  ((weight + weight_v0) + weight_v1) ...        peak (fp32)   max(peak, peak_v)
 *   pixels (int64) += pixels_v       stops (int64) += stops_v    seen (int32)  += (pixels_v > 0)
 * and per view, WRITTEN, NOT ACCUMULATED: view_weight [views][n] fp32 = weight_vi, view_pixels [views][n] int32 = pixels_vi; a culled
 * (view, Gaussian) gets exact zeros in both and changes no accumulator.
 * SAME INPUT, SAME BYTES on every call: one owner per instance slot and per output, no floating-point atomics, no atomics at all.  VIEWS
 * DO NOT MIX: view_weight[v], view_pixels[v] and view v's terms are the same bits whether v is walked alone or in a batch.  fwd_ws IS
 * NOT WRITTEN.  If the recorded instance total exceeds max_instances the kernels read that on the device and return with EVERY OUTPUT
 * UNTOUCHED (the per-view rows included).
 * Limits and argument errors are the forward's, plus a NULL fwd_ws (SIXDGS_E_BADARG), misaligned outputs (4 bytes, the int64 arrays 8)
 * and a workspace smaller than sixdgs_raster_views_workspace_bytes / sixdgs_raster_contrib_workspace_bytes say (SIXDGS_E_WORKSPACE):
 * all answered without touching a GPU.  views == 0 or n == 0 returns 0; so does a call with every output NULL.
 * sixdgs_raster_contrib_workspace_bytes is answered without a GPU and is 0 outside the limits: 16 B per instance (max_instances slots of
 * sum, max, adds and stops), rounded up to 256.  One 256-thread workgroup per tile and view, one pixel per lane, the list staged through
 * LDS in rounds of 256; after a round, thread k writes the round's k-th instance's own slot -- every slot exactly once, zeros in rounds
 * behind the point where every pixel of the tile has stopped; then one lane per Gaussian sums its slots.  prof (may be NULL) receives
 * one slot per stage: walk, gather.
 *
 * sixdgs_scene_contrib measures many views as one call.  Scene arrays, flags, sh_degree and scale_modifier as sixdgs_raster_views takes
 * them; cams [views][16].  No image is formed, so there is no background.  It zeroes status[0] and instances_needed[0] -- NOT the
 * accumulators, which are the caller's as above --, then for each chunk of up to `chunk` (>= 1) consecutive rows of cams enqueues on
 * `stream`, through the entry points as they are: sixdgs_raster_views of the chunk's rows with no image and no radii (project, scan,
 * emit, sort and ranges; the blend does not run; the count stays on the device), sixdgs_raster_contrib into the accumulators and -- when
 * given -- the chunk's rows of view_weight / view_pixels, and a record: instances_needed[0] = max(instances_needed[0], count); if
 * count > max_instances, bit 1 of status[0] is set and that chunk leaves the accumulators and its per-view rows as they were; other
 * chunks are unaffected.  No host synchronisation, no device-to-host copy, no allocation; when it returns, the work is enqueued.  Given a
 * capacity that fits, every output is the same bits for every chunk.  Limits and errors are the parts'; views == 0 returns 0, n == 0
 * after the zeroing.  sixdgs_scene_contrib_workspace_bytes is answered without a GPU and is 0 outside the limits: the two parts'
 * workspaces at `chunk` views and the count, each piece rounded up to 256 B. */
size_t sixdgs_raster_contrib_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances);
int sixdgs_raster_contrib(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                          float* weight /*[n]*/, float* peak /*[n]*/, int64_t* pixels /*[n]*/, int64_t* stops /*[n]*/,
                          int32_t* seen /*[n]*/, float* view_weight /*[views][n] or NULL*/, int32_t* view_pixels /*[views][n] or NULL*/,
                          void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof);
size_t sixdgs_scene_contrib_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances);
int sixdgs_scene_contrib(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                         const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams /*[views][16]*/,
                         int views, int width, int height, float scale_modifier, int chunk, int64_t max_instances, float* weight,
                         float* peak, int64_t* pixels, int64_t* stops, int32_t* seen, float* view_weight, int32_t* view_pixels,
                         int32_t* status /*[1]*/, int64_t* instances_needed /*[1]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth maps of views (additive in ABI 10): how far away what a pixel of sixdgs_raster_views shows is -- the blend of step 11 with the
 * Gaussians' camera depth p.z in the place of a colour (`expected`), the depth at which the pixel's transmittance falls below one half
 * (`median`, with the Gaussian that takes it there), 1 - T, and the world point of the pixel's ray at either depth.  All arithmetic in
 * fp32, no contraction into fused multiply-adds.
 *
 * fwd_ws is the workspace of a COMPLETED sixdgs_raster_views call with the same n, views, width, height and max_instances, whose
 * instance count fitted, not written since (whether that call produced an image does not matter; the scene is in fwd_ws already and is
 * not passed again); it is not written here.  For view v and pixel (x, y) inside the image the walk of step 11 is repeated operation by
 * operation over the same ordered list -- d, power, the skip when power > 0, alpha_j = min(0.99, o exp(power)), the skip when
 * alpha_j < 1/255, T' = T (1 - alpha_j), the stop when T' < 1e-4 -- so that every skip and the stop fall exactly where the forward's
 * did.  z_j is the float whose bits the forward stored for the Gaussian (step 1's p.z, the sort key of step 10).  With T = 1, D = 0 and
 * no median to begin with, for each Gaussian j the pixel ADDS (neither skipped nor the stopper), in order:
 *   1. D += (z_j alpha_j) T, T the value before j: the colour channels' form with c = z_j;
 *   2. if no median has been taken yet and T' < 0.5: median = z_j, median_index = i_j, the Gaussian's index in the scene;
 *   3. T = T'.
 * The stop cannot swallow a median: the Gaussian that takes T from >= 0.5 to below it has T' >= 0.5 (1 - 0.99) = 0.005 > 1e-4, so it
 * is always added.  As the backward takes 1 - T for a fourth colour channel of colour 1, D is a fifth of colour z_j and background 0.
 * Outputs, each may be NULL, [views][height][width], WRITTEN, NOT ACCUMULATED, one owner per element:
 *   expected      fp32  D, UN-NORMALISED: the depth channel of the blend; expected / alpha is the mean depth of what the pixel saw;
 *   median        fp32  and median_index int32: 0.f and -1 where T never fell below 0.5;
 *   alpha         fp32  1 - T of the end of the walk: THE SAME BITS as channel 3 of the forward's image_f32;
 *   points        fp32  [views][height][width][3]: the world point on the pixel's ray at camera depth d, d = median (points_kind 0) or
 *                 expected / alpha (points_kind 1).  With the view's row of cams = [W | t], fx, fy, cx, cy (the forward's row; cams is
 *                 needed only for points and may be NULL otherwise): r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1), q = d r - t,
 *                 X = W^T q, each of the three dot products as (a + b) + c in index order.  Exact (0, 0, 0) where the pixel has no depth of
 *                 that kind: median_index < 0, respectively alpha == 0.  Validity is those two and is not encoded in the point.
 * SAME INPUT, SAME BYTES on every call: no atomics at all.  VIEWS DO NOT MIX: a view's maps are the same bits whether it is walked alone
 * or in a batch.  Pixels of a ragged last tile that lie outside the image are never written.  If the recorded instance total exceeds
 * max_instances the kernel reads that on the device and returns with EVERY OUTPUT UNTOUCHED.  views == 0 returns 0; n == 0 writes the
 * values of a pixel with an empty list: 0, 0, -1, 0 and zero points; a call with every output NULL returns 0 without a launch.
 * Limits and argument errors are the forward's, plus points_kind outside {0, 1}, a NULL fwd_ws, points without cams and misaligned
 * outputs or cams (4 bytes): SIXDGS_E_BADARG; a fwd_ws_bytes below sixdgs_raster_views_workspace_bytes or a ws_bytes below
 * sixdgs_raster_depth_workspace_bytes: SIXDGS_E_WORKSPACE; all answered without touching a GPU.  The walk needs no workspace of its own:
 * sixdgs_raster_depth_workspace_bytes, answered without a GPU, is 256 inside the limits and 0 outside them, and ws (256-byte aligned) is
 * not written.  One 256-thread workgroup per tile and view, one pixel per lane, the list staged through LDS in rounds of 256 (conic and
 * opacity, centre, z, index: 8 KB).  prof (may be NULL) receives one slot: walk.
 *
 * sixdgs_scene_depth renders the maps of many views as one call.  Scene arrays, flags, sh_degree and scale_modifier as
 * sixdgs_raster_views takes them; cams [views][16]; the five outputs over all views, and optionally image_u8
 * [views][height][width][channels] (channels 3 or 4) -- the forward's own uint8 image over `background` ([3] device, needed only with
 * image_u8), so that the colours of a point cloud come from the same pass.  It zeroes status[0] and instances_needed[0], then for each
 * chunk of up to `chunk` (>= 1) consecutive rows of cams enqueues on `stream`, through the entry points as they are:
 * sixdgs_raster_views of the chunk's rows into the chunk's rows of image_u8 (without image_u8: no image, its blend does not run; the
 * count stays on the device), sixdgs_raster_depth into the chunk's rows of the outputs, and a record: instances_needed[0] =
 * max(instances_needed[0], count); if count > max_instances, bit 1 of status[0] is set and that chunk's rows of every output, image_u8
 * included, are left as they were; other chunks are unaffected.  No host synchronisation, no device-to-host copy, no allocation; when
 * it returns, the work is enqueued.  Given a capacity that fits, every output is the same bytes for every chunk.  Limits and errors are
 * the parts'; views == 0 returns 0.  sixdgs_scene_depth_workspace_bytes is answered without a GPU and is 0 outside the limits: the two
 * parts' workspaces at `chunk` views and the count, each piece rounded up to 256 B. */
size_t sixdgs_raster_depth_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances);
int sixdgs_raster_depth(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                        const float* cams /*[views][16] or NULL*/, float* expected /*[views][height][width]*/,
                        float* median /*[views][height][width]*/, int32_t* median_index /*[views][height][width]*/,
                        float* alpha /*[views][height][width]*/, float* points /*[views][height][width][3]*/,
                        int points_kind /*0 median, 1 expected / alpha*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                        sixdgs_profile* prof);
size_t sixdgs_scene_depth_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances);
int sixdgs_scene_depth(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                       const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams /*[views][16]*/,
                       int views, int width, int height, float scale_modifier, const float* background /*[3] device or NULL*/, int chunk,
                       int64_t max_instances, float* expected, float* median, int32_t* median_index, float* alpha, float* points,
                       int points_kind, uint8_t* image_u8 /*or NULL*/, int channels /*3 or 4*/, int32_t* status /*[1]*/,
                       int64_t* instances_needed /*[1]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The photometric loss of render-and-compare (additive in ABI 10): per view loss_v = (1 - lambda) L1 + lambda (1 - SSIM) between an
 * image a and a target b, and grad_image = grad_loss[v] d loss_v / d a.  It is the reference's training objective (train.py:119 with
 * lambda_dssim = 0.2; utils/loss_utils.py: 11 x 11 Gaussian window, sigma 1.5, padding 5, one group per channel).  All arithmetic in
 * fp32, no contraction into fused multiply-adds.  Per view v and channel c in {r, g, b}:
 *   1. a = image[v][y][x][c], image fp32 [views][height][width][image_stride], image_stride 3 or 4 (4: sixdgs_raster_views' image_f32;
 *      the fourth channel is never read);
 *   2. b = target[v][y][x][c]: fp32 [views][height][width][target_stride], target_stride 3 or 4 (target_is_u8 == 0), or uint8
 *      [views][height][width][3] with b = float(u) / 255.0f (target_is_u8 == 1, target_stride 3);
 *   3. w[11] = SIXDGS_SSIM_WINDOW below: the fp32 roundings of exp(-(i - 5)^2 / 4.5) / sum, normalised in fp64;
 *   4. blur(f)(x, y) = sum_j w[j] h(x, y + j - 5), h(x, y) = sum_k w[k] f(x + k - 5, y): first along x, then along y, each sum
 *      started with its term 0 and continued in ascending index; f counts as ZERO outside the image, h is formed from that;
 *   5. mu1 = blur(a), mu2 = blur(b), s1 = blur(a a) - mu1 mu1, s2 = blur(b b) - mu2 mu2, s12 = blur(a b) - mu1 mu2;
 *   6. A1 = 2 (mu1 mu2) + C1, A2 = 2 s12 + C2, B1 = (mu1 mu1 + mu2 mu2) + C1, B2 = (s1 + s2) + C2, C1 = 1e-4f, C2 = 9e-4f;
 *      m = (A1 A2) / (B1 B2);
 *   7. per pixel the channels are added r, g, b: (m_r + m_g) + m_b and likewise |a - b|.  The pixels of a 16 x 16 tile (the
 *      rasteriser's grid gx = ceil(width / 16), gy = ceil(height / 16); pixels outside the image count as 0) are added in a fixed tree:
 *      the 256 pixels in 4 groups of 64 in rows-of-16 order, within a group x += x_(l xor s), s = 32 .. 1, then the groups in order;
 *      then the tiles of the view in row-major order, one after the other.  With n = float(3 height width):
 *      l1_v = sum |a - b| / n, ssim_v = sum m / n, loss_v = (1 - lambda) l1_v + lambda (1 - ssim_v).
 * The gradient is the standard two-pass one.  With blur(a a) and blur(a b) held, per pixel and channel
 *   d_s1 = -(m / B2),  d_s12 = (2 A1) / (B1 B2),
 *   d_mu1 = (((2 mu2) A2) / (B1 B2) - ((2 mu1) m) / B1) - ((2 mu1) d_s1 + mu2 d_s12)
 * are the derivatives of m by s1, s12 and mu1 (the last one total: through B1, A1 and through s1, s12).  These three maps are stored;
 * the window is symmetric, so the same blur with the same zero rule is the adjoint, and
 *   X = (blur(d_mu1) + (2 a) blur(d_s1)) + b blur(d_s12),
 *   grad_image[v][y][x][c] = g_v (((1 - lambda) / n) sign(a - b) - (lambda / n) X),  sign(0) = 0, g_v = grad_loss[v] (NULL: 1).
 * With image_stride 4 the fourth channel of grad_image is written as exact zero.
 *
 * Outputs, each may be NULL, WRITTEN, NOT ACCUMULATED: loss [views]; parts [views][2] = (l1_v, ssim_v); grad_image, the image's shape.
 * With grad_image NULL neither the maps nor the second pass run and the smaller workspace suffices; with all three NULL nothing runs.
 * SAME INPUT, SAME BYTES on every call: no floating-point atomics.  VIEWS DO NOT MIX: loss[v], parts[v] and grad_image[v] are the
 * same bits whether view v is passed alone or in a batch.  Nothing is read outside the arrays as declared, and the fourth channel of a
 * stride-4 image or target is not read at all.  image, target (fp32), grad_loss and the outputs are 4-byte aligned, ws 256-byte.
 * Limits: 1 <= width, height <= 16384, views <= 65535, views gx gy < 2^31, lambda in [0, 1] (so finite).  Argument errors:
 * SIXDGS_E_BADARG; too small a workspace: SIXDGS_E_WORKSPACE; both without touching a GPU.  views == 0 returns 0.
 * sixdgs_photometric_loss_workspace_bytes is answered without a GPU and is 0 outside the limits: 8 B per tile and view, plus, with
 * want_grad, 36 B per pixel and view (the three maps of three channels, planar).  prof (may be NULL) receives one slot per stage:
 * moments (steps 1 - 6 and the tile sums), sums (step 7; only with loss or parts), gradient (only with grad_image). */
#define SIXDGS_SSIM_WINDOW                                                                                              \
  {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f, 0.213005543f, 0.109360687f, \
   0.0360007733f,  0.00759875821f, 0.00102838012f}
size_t sixdgs_photometric_loss_workspace_bytes(int views, int width, int height, int want_grad);
int sixdgs_photometric_loss(const float* image /*[views][height][width][image_stride]*/, int image_stride /*3 or 4*/,
                            const void* target, int target_is_u8, int target_stride /*3 or 4; 3 with uint8*/, int views, int width,
                            int height, float lambda, const float* grad_loss /*[views] device or NULL*/, float* loss /*[views]*/,
                            float* parts /*[views][2]*/, float* grad_image, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                            sixdgs_profile* prof);

/* ---------------------------------------------------------------------------------------------
 * The pose arithmetic of render-and-compare refinement (additive in ABI 10): a rigid motion delta[v] = (dt, w) -- translation, then
 * axis-angle -- applied AFTER a view's starting w2c, its exact derivative, Adam on the six numbers, and the bookkeeping of the best
 * iterate.  All arithmetic in fp32, no contraction into fused multiply-adds; one thread per view, one owner per output, no atomics;
 * views never mix: row v of every output is the same bits whether view v is passed alone or in a batch.
 *
 * COMPOSE.  start[v] = 16 floats: w2c rows 0..2 = [R | t] (12 floats, row-major 3 x 4), then fx, fy, cx, cy.
 *   1. x = (w0 w0 + w1 w1) + w2 w2 (= theta^2); K = [w]x = [[0, -w2, w1], [w2, 0, -w0], [-w1, w0, 0]];
 *   2. a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3.  For x < 1: Horner in x over k = 5 .. 0 with the fp32
 *      coefficients (-1)^k / (2k + 1)!, (-1)^k / (2k + 2)!, (-1)^k / (2k + 3)! (each the fp32 quotient of 1 and the factorial):
 *      a = 1 + x (-1/6 + x (1/120 + x (-1/5040 + x (1/362880 + x (-1/39916800))))) and likewise b from 1/2, c from 1/6; the first
 *      dropped term is below 2e-10 of the value.  For x >= 1: th = sqrt(x), s = sin th, h = sin(th / 2), a = s / th,
 *      b = (2 (h h)) / x, c = (th - s) / (x th) -- no cancellation in b, and th - s keeps at least th / 6;
 *   3. every 3 x 3 product is three terms added in index order, (p_i0 q_0j + p_i1 q_1j) + p_i2 q_2j; K2 = K K;
 *      dR_ij = ((i == j ? 1 : 0) + a K_ij) + b K2_ij;
 *   4. rows[v] = [dR R | dR t + dt | fx fy cx cy]: the 3 x 4 product dR [R | t] as in 3, then dt added to its fourth column.
 *   delta = 0 returns start bit for bit (for finite start; a -0 entry comes back as +0).
 *
 * CHAIN RULE.  G = the 3 x 4 part of d_rows[v] = dL / d rows[v] (its intrinsics entries are ignored), [R | t] of start[v]:
 *   d dt = G[:, 3];  A_ir = ((G_i0 R_r0 + G_i1 R_r1) + G_i2 R_r2) + G_i3 t_r;  M = A dR^T (as in 3);
 *   tau = (M_21 - M_12, M_02 - M_20, M_10 - M_01);  k1 = w x tau, k2 = w x k1 (cross products: u1 v2 - u2 v1, ...);
 *   d w_i = (tau_i - b k1_i) + c k2_i.  This is the exact derivative of COMPOSE.
 *
 * ADAM (torch.optim.Adam's plain form), step t = step + 1, per entry g of the six:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) (g g);  delta = delta - (lr / c1) (m / (sqrt(v) / c2 + eps)),
 *   c1 = 1 - beta1^t and c2 = sqrt(1 - beta2^t) formed by the host in double from the float arguments and rounded to float.
 *
 * sixdgs_pose_compose writes rows [views][16] from start [views][16] and delta [views][6] (rows must not be start).
 *
 * sixdgs_pose_step is step `step` (>= 0) of a refinement: `rows` holds iterate `step`, loss [views] its loss, d_rows [views][16]
 * dL / d rows (not read, may be NULL, with evaluate_only = 1).  With count = *instances (0 when instances is NULL), per view v:
 *   1. view 0 alone: instances_needed[0] = max(instances_needed[0], count);
 *   2. if count > max_instances, bit 1 of status[v] is set.  While bit 1 is set NOTHING of a step is recorded: history_row[v] = NaN
 *      and the view returns -- the images of an overflowed step are unspecified, so every view is frozen from then on;
 *   3. history_row[v] = loss[v]; if loss[v] < best_loss[v] (strict: the first minimum is kept; never true for NaN):
 *      best_loss[v] = loss[v], best_step[v] = step, best_rows[v] = rows[v];
 *   4. if loss[v] or -- without evaluate_only -- any of the 12 w2c entries of d_rows[v] is not finite, bit 0 of status[v] is set.
 *      A view with bit 0 set is frozen: delta, m, v and rows no longer change (steps 1 - 3 go on);
 *   5. otherwise, without evaluate_only: CHAIN RULE, ADAM, and rows[v] = COMPOSE(start[v], delta[v]), the next iterate.
 * The caller owns the state and starts it as delta = m = v = 0, rows = COMPOSE(start, 0), best_loss = +inf, best_step = 0,
 * best_rows = start, status = 0, instances_needed = 0.  history_row is the caller's history + step * views.
 * Limits: views <= 65535, 1 <= max_instances < 2^31, lr > 0 finite, beta1, beta2 in [0, 1), eps >= 0 finite.  SIXDGS_E_BADARG without a
 * launch for argument errors (a NULL array, rows == start, rows == best_rows included); views == 0 returns 0. */
int sixdgs_pose_compose(const float* start /*[views][16]*/, const float* delta /*[views][6]*/, int views, float* rows /*[views][16]*/,
                        sixdgs_stream_t stream);
int sixdgs_pose_step(const float* start /*[views][16]*/, const float* loss /*[views]*/, const float* d_rows /*[views][16] or NULL*/,
                     const int64_t* instances /*[1] device or NULL*/, int64_t max_instances, int views, int step, int evaluate_only,
                     float lr, float beta1, float beta2, float eps, float* delta /*[views][6]*/, float* m /*[views][6]*/,
                     float* v /*[views][6]*/, float* rows /*[views][16] in: iterate step, out: iterate step + 1*/,
                     float* best_loss /*[views]*/, int32_t* best_step /*[views]*/, float* best_rows /*[views][16]*/,
                     float* history_row /*[views]*/, int32_t* status /*[views]*/, int64_t* instances_needed /*[1]*/,
                     sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Render-and-compare pose refinement as one call (additive in ABI 10).  Starts the state as sixdgs_pose_step describes, then for
 * s = 0 .. steps enqueues on `stream`, in this order and through the entry points above as they are:
 *   1. sixdgs_raster_views of the current rows (float image only; the instance count is left on the device);
 *   2. sixdgs_photometric_loss against the target (lambda; with grad_image, grad_loss = 1, except at s = steps);
 *   3. sixdgs_raster_views_backward with only d_cams wanted (skipped at s = steps);
 *   4. sixdgs_pose_step (evaluate_only at s = steps) with that count, max_instances and history + s * views.
 * So iterate s is evaluated at step s, steps Adam updates are made, and history has steps + 1 rows.  The call makes no host
 * synchronisation, no device-to-host copy and no allocation; the library stays stateless; when it returns, the work is enqueued.
 * Scene arrays, flags, scale_modifier and background (device [3]) as sixdgs_raster_views takes them; start_rows [views][16] as cams;
 * the target in the three forms sixdgs_photometric_loss takes, of size width x height.
 * Outputs (device, all required except delta): best_rows [views][16], best_loss [views], best_step [views] int32, history
 * [steps + 1][views], delta [views][6] = the last iterate's motion (may be NULL), status [views] (bit 0: not finite, bit 1: capacity),
 * instances_needed [1] = the largest instance count seen.  When max_instances was too small at some step, bit 1 is set in every
 * status[v], that step and all later ones record nothing (their history rows are NaN; best_* are those of the steps before,
 * best_step = 0 and best_rows = start_rows when it was step 0): call again with max_instances >= instances_needed[0].
 * SAME INPUT, SAME BYTES; row v of every output is the same bits whether view v is refined alone or in a batch, given a capacity that
 * fits.  Limits are the parts': the rasteriser's sizes, lambda in [0, 1], 1 <= steps, the Adam limits of sixdgs_pose_step.
 * SIXDGS_E_BADARG for argument errors, SIXDGS_E_WORKSPACE for too small a workspace, both without touching a GPU; views == 0 returns 0.
 * sixdgs_refine_poses_workspace_bytes is answered without a GPU and is 0 outside the limits: the three parts' workspaces (the loss's
 * with the gradient), two float images of views x height x width x 4, and 204 B of state per view (rows, d_rows, loss, delta, m, v) plus the count, each
 * piece rounded up to 256 B. */
size_t sixdgs_refine_poses_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances);
int sixdgs_refine_poses(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity,
                        int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n,
                        const float* start_rows /*[views][16]*/, int views, int width, int height, float scale_modifier,
                        const float* background /*[3] device*/, const void* target, int target_is_u8, int target_stride, float lambda,
                        int steps, float lr, float beta1, float beta2, float eps, int64_t max_instances, float* best_rows, float* best_loss,
                        int32_t* best_step, float* history, float* delta /*or NULL*/, int32_t* status, int64_t* instances_needed, void* ws,
                        size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Coarse-to-fine pose refinement (additive in ABI 10): the targets of a level schedule, the hand-over of a camera from one level to
 * the next, and the whole schedule as one call.  The rules are csrc/pyramid_rules.h's.
 *
 * LEVEL GEOMETRY.  A level of downscale d of a W x H query has w = W / d by h = H / d pixels (integer division); pixel (x, y) is the
 * mean of the d x d block of the query whose corner is (ox + x d, oy + y d), with ox = (W - w d) / 2 and oy = (H - h d) / 2: the
 * centred crop to a multiple of d.  Its intrinsics are fx / d, fy / d, (cx - ox) / d, (cy - oy) / d, with d, ox and oy converted to
 * fp32 first.  1 <= d <= 256.
 *
 * TARGET VALUE of level pixel (x, y), channel c, from the block's bytes u.  The sums are exact integers; the fp32 expression is
 * evaluated as written, without contraction into fused multiply-adds.
 *   without compositing:  S = sum u_c;  value = float(S) / float(255 d d).
 *   with compositing (four channels; a = the fourth):  S1 = sum u_c u_a,  S2 = sum (255 - u_a),  k = 255.0f * background[c] (once);
 *     value = (float(S1) + k * float(S2)) / (65025.0f * float(d d)).
 * With d <= 256, S, S2 and 255 d d stay below 2^24 (exact in fp32) and S1 <= 255^2 2^16 < 2^32 fits 32 unsigned bits.
 *
 * sixdgs_target_pyramid reads images uint8 [views][height][width][channels] (channels 3 or 4) and writes, for each of `levels` (1 .. 8)
 * downscales h_downscale[l] (HOST array), the level's target fp32 [views][h][w][3] to h_out[l] (HOST array of device pointers, 4-byte
 * aligned).  composite = 1 needs channels == 4 and h_background (HOST [3], finite, read at the call); with composite = 0 the fourth
 * channel of a four-channel image is never read.  One launch per level of one streaming kernel: per input row a workgroup's bytes are
 * one contiguous run, read one byte at a time up to the first 16-byte boundary, 16 bytes per lane from there, and byte-wise behind the
 * last boundary; nothing outside the crop is read; one owner per output, no atomics.  SAME INPUT, SAME BYTES; a view's target does not
 * depend on the other views of the call.  Limits: views <= 65535, width, height <= 32768.  SIXDGS_E_BADARG without a launch for
 * argument errors: levels outside 1 .. 8, a d outside 1 .. 256 or with h or w of 0, a NULL or misaligned output.  views == 0 returns 0.
 *
 * sixdgs_pose_rebase: rows_out[v] = (the 12 w2c entries of rows_in[v], intrinsics[v][4]), a copy of bits (rows_out may be rows_in).
 *
 * sixdgs_refine_poses_levels runs a schedule of `levels` (1 .. 8) levels, coarse to fine, and reads nothing back.  Scene arrays, flags,
 * scale_modifier, background (device [3]) and lambda as sixdgs_refine_poses takes them; start_rows [views][16] carry the LAST level's
 * intrinsics.  Per level l, all HOST arrays: h_width[l], h_height[l], h_steps[l] (>= 1), h_lr[l], h_target[l] (device fp32
 * [views][h_height[l]][h_width[l]][3]), h_intrinsics[l] (device [views][4]) and h_max_instances[l].  It enqueues:
 *   1. the input's loss: sixdgs_raster_views of start_rows at the last level, sixdgs_photometric_loss without a gradient.
 *      loss_input[v] is that loss; status[v] starts as 0.  If the instance count exceeds h_max_instances[levels - 1], loss_input[v]
 *      is NaN and status[v] starts with bit 1 set.
 *   2. for l = 0 .. levels - 1: start_l = sixdgs_pose_rebase(l == 0 ? start_rows : level l - 1's best_rows, h_intrinsics[l]); then
 *      exactly the loop of sixdgs_refine_poses from start_l on h_target[l] with h_steps[l], h_lr[l] and h_max_instances[l], where
 *      delta, m, v, best_loss, best_step and best_rows start fresh (as sixdgs_pose_step describes) and status is CARRIED from the
 *      level before.  So a capacity overflow at one level freezes every later step of every later level, whose history rows are NaN,
 *      and a view frozen by bit 0 stays frozen.  The level's history rows are history + (sum over l' < l of (h_steps[l'] + 1)) * views.
 *      instances_needed[l] (all start as 0) is the largest instance count seen at level l, the count of 1. included in the last.
 *   3. kept_input[v] = NOT (best_loss[levels - 1][v] < loss_input[v]) -- a NaN on either side and a tie keep the input --;
 *      out_rows[v] = kept_input[v] ? start_rows[v] : the last level's best_rows[v].
 * Outputs (device): out_rows [views][16] (not start_rows), loss_input [views], kept_input [views] int32, best_loss and best_step
 * [levels][views], instances_needed [levels] int64, history [sum (h_steps[l] + 1)][views], status [views].
 * SAME INPUT, SAME BYTES; row v of every output is the same bits whether view v is refined alone or in a batch, given capacities that
 * fit.  SIXDGS_E_BADARG for argument errors, SIXDGS_E_WORKSPACE for too small a workspace, both without touching a GPU; views == 0
 * returns 0.  sixdgs_refine_poses_levels_workspace_bytes is answered without a GPU and is 0 outside the limits: the largest of the
 * levels' sixdgs_refine_poses_workspace_bytes, plus two sets of camera rows [views][16] (a level's start and its best), each piece
 * rounded up to 256 B. */
int sixdgs_target_pyramid(const uint8_t* images, int views, int height, int width, int channels, int composite,
                          const float* h_background /*host [3] or NULL*/, int levels, const int32_t* h_downscale /*host [levels]*/,
                          float* const* h_out /*host [levels] of device pointers*/, sixdgs_stream_t stream);
int sixdgs_pose_rebase(const float* rows_in /*[views][16]*/, const float* intrinsics /*[views][4]*/, int views, float* rows_out /*[views][16]*/,
                       sixdgs_stream_t stream);
size_t sixdgs_refine_poses_levels_workspace_bytes(int64_t n, int views, int levels, const int32_t* h_width, const int32_t* h_height,
                                                  const int64_t* h_max_instances);
int sixdgs_refine_poses_levels(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity,
                               int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n,
                               const float* start_rows /*[views][16]*/, int views, float scale_modifier, const float* background /*[3] device*/,
                               float lambda, int levels, const int32_t* h_width, const int32_t* h_height, const int32_t* h_steps,
                               const float* h_lr, const float* const* h_target, const float* const* h_intrinsics,
                               const int64_t* h_max_instances, float beta1, float beta2, float eps, float* out_rows, float* loss_input,
                               int32_t* kept_input, float* best_loss, int32_t* best_step, int64_t* instances_needed, float* history,
                               int32_t* status, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Adam over a scene's Gaussians and the opacity reset (additive in ABI 10): the optimiser's side of fitting a set of Gaussians to
 * posed views (the reference's train.py:94-122 and scene/gaussian_model.py:230-282; n is fixed within a call -- the densification
 * round that changes it is sixdgs_densify, further down).  All arithmetic in fp32, no contraction into fused multiply-adds; one owner
 * per output, no floating-point atomics, the same bytes on every call.
 *
 * GROUPS.  Six, in this order everywhere: xyz [n,3], f_dc [n,1,3], f_rest [n,n_coef-1,3], opacity [n], scale [n,3], rot [n,4]:
 * 11 + 3 n_coef floats per Gaussian.  m and v are each ONE buffer of n (11 + 3 n_coef) floats, group after group in that order, so the
 * slices start at 0, 3n, 6n, 3n (n_coef + 1), 3n (n_coef + 1) + n and 3n (n_coef + 2) + n floats.
 *
 * sixdgs_gaussian_adam updates the six parameter arrays in place from their six gradient arrays: Adam's step t = step + 1 (the ADAM
 * of sixdgs_pose_step, with the group's rate), per entry with gradient g:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) (g g);  p = p - (lr[k] / c1) (m / (sqrt(v) / c2 + eps)),
 *   c1 = 1 - beta1^t and c2 = sqrt(1 - beta2^t) formed by the host in double from the float arguments and rounded to float;
 *   lr [6] is a HOST array, read at the call.
 * Rules:
 *   1. a group whose gradient pointer is NULL is frozen: its parameters and its slice of m and v are not touched, bit for bit (its
 *      parameter pointer may then be NULL as well); with n_coef == 1 the f_rest group is empty and both its pointers are ignored;
 *   2. lr[k] == 0 is legal and still updates m and v, as torch.optim.Adam does;
 *   3. an entry whose gradient is not finite keeps p, m and v, and bit 0 of status[0] is set;
 *   4. with count = *instances (instances may be NULL: no check): if count > max_instances the step changes nothing at all and sets
 *      bit 1 of status[0] -- the gradients of an overflowed rasteriser call are unspecified;
 *   5. status[0] is read on entry: once bit 1 is set, later calls change nothing.  The caller starts status[0] as 0.
 * Bits are set with an integer atomic OR.  One launch covers all groups: workgroups walk a flat index over the groups' entries, with
 * 16-byte accesses where a group's four pointers (parameter, gradient, its m and v slices) are all 16-byte aligned and 4-byte accesses
 * otherwise; the arithmetic is per entry, so the bits do not depend on the alignment.
 * Limits: n < 2^31, 1 <= n_coef <= 16, 0 <= step, lr[k] >= 0 finite, beta1, beta2 in [0, 1), eps >= 0 finite, 1 <= max_instances < 2^31.
 * SIXDGS_E_BADARG without a launch for argument errors: a NULL lr, m, v or status, a NULL parameter pointer whose gradient pointer is
 * not NULL (a NULL f_rest with n_coef > 1 when its gradient is given included), m == v, a misaligned array (4 bytes; instances 8).
 * n == 0 returns 0.
 *
 * sixdgs_opacity_reset is the reference's reset_opacity on the array and on the optimiser's state: per Gaussian, with x its opacity,
 *   a = 1 / (1 + exp(-x)) when opacity_is_logit != 0, x otherwise;  o = min(a, ceiling);
 *   opacity = log(o / (1 - o)) when opacity_is_logit != 0, o otherwise;  m_opacity = v_opacity = 0
 * (m_opacity, v_opacity: the opacity slices of m and v, each may be NULL).  ceiling in (0, 1); n == 0 returns 0; SIXDGS_E_BADARG
 * without a launch otherwise. */
int sixdgs_gaussian_adam(int64_t n, int n_coef, int step, float* xyz, float* f_dc, float* f_rest, float* opacity, float* scale, float* rot,
                         const float* d_xyz, const float* d_f_dc, const float* d_f_rest, const float* d_opacity, const float* d_scale,
                         const float* d_rot, float* m, float* v, const float* lr /*[6] host*/, float beta1, float beta2, float eps,
                         const int64_t* instances /*[1] device or NULL*/, int64_t max_instances, int32_t* status /*[1] device*/,
                         sixdgs_stream_t stream);
int sixdgs_opacity_reset(float* opacity /*[n]*/, int64_t n, int opacity_is_logit, float* m_opacity /*[n] or NULL*/,
                         float* v_opacity /*[n] or NULL*/, float ceiling, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fitting a scene's Gaussians to posed views as one call (additive in ABI 10).  The scene arrays are MUTABLE and updated in place; n is
 * fixed for the whole call (a fit that densifies is cut into sixdgs_fit_scene_steps calls around sixdgs_densify).  The call first
 * zeroes m, v, status[0] and instances_needed[0], then for
 * s = 0 .. steps - 1 enqueues on `stream`, in this order and through the entry points above as they are:
 *   1. the step's views h_view[s][0 .. batch): with batch == 1 pointer offsets into cams and the target, no copy; otherwise
 *      device-to-device copies of the batch's camera rows and target views into the workspace, in slot order (duplicates allowed);
 *   2. sixdgs_raster_views at sh_degree h_sh_degree[s] (float image only; the instance count is left on the device);
 *   3. sixdgs_photometric_loss with the gradient, grad_loss NULL: the objective is the sum of the batch's per-view losses;
 *   4. sixdgs_raster_views_backward with exactly the outputs of the groups set in group_mask (bit k = group k in the order xyz, f_dc,
 *      f_rest, opacity, scale, rot) and no d_cams;
 *   5. history[s][b] = the loss of slot b; instances_needed[0] = max(instances_needed[0], count).  If count > max_instances, bit 1 of
 *      status[0] is set; while bit 1 is set the row is NaN instead;
 *   6. sixdgs_gaussian_adam with step s, the rates h_lr[s][6] and that count; a group cleared in group_mask is frozen;
 *   7. when h_reset[s] != 0: sixdgs_opacity_reset with reset_ceiling on the array and the opacity slices of m and v, skipped once bit 1
 *      is set (it runs whether or not the opacity group is in group_mask).
 * h_view [steps][batch] int32, h_lr [steps][6], h_sh_degree [steps] int32 and h_reset [steps] uint8 are HOST arrays, read at the call.
 * The call makes no host synchronisation, no device-to-host copy and no allocation; the library stays stateless; when it returns, the
 * work is enqueued.  SAME INPUT, SAME BYTES.  Scene arrays, flags, scale_modifier and background (device [3]) as sixdgs_raster_views
 * takes them; cams [views][16]; the target in the three forms sixdgs_photometric_loss takes, views images of width x height.
 * Outputs (device): the scene arrays; m, v (caller-owned, n (11 + 3 n_coef) floats each); history [steps][batch]; status [1] (bit 0: a
 * gradient entry was not finite and was left out, bit 1: capacity); instances_needed [1] = the largest instance count seen.  When
 * max_instances was too small at some step, that step and all later ones change nothing and their history rows are NaN: the scene, m
 * and v are as they were after the last good step; call again, from the scene as it was before the call, with
 * max_instances >= instances_needed[0].
 * Limits are the parts': the rasteriser's sizes with views = batch, 1 <= views <= 65535, 1 <= batch, lambda in [0, 1], 1 <= steps, the
 * limits of sixdgs_gaussian_adam and sixdgs_opacity_reset, 0 < group_mask < 64, h_sh_degree[s] in [0, 3] with
 * (h_sh_degree[s] + 1)^2 <= n_coef.  SIXDGS_E_BADARG for argument errors -- a view index outside [0, views) and a reset asked for
 * without opacity_is_logit included --, SIXDGS_E_WORKSPACE for too small a workspace, both without touching a GPU.
 * sixdgs_fit_scene_workspace_bytes is answered without a GPU and is 0 outside the limits: the three parts' workspaces at `batch` views
 * (the loss's with the gradient), two float images of batch x height x width x 4, the gathered camera rows, the gathered targets
 * (reserved for the widest form, 16 B per pixel), the losses, the count, and the six gradient arrays (n (11 + 3 n_coef) floats), each
 * piece rounded up to 256 B. */
size_t sixdgs_fit_scene_workspace_bytes(int64_t n, int n_coef, int batch, int width, int height, int64_t max_instances);
int sixdgs_fit_scene(float* xyz, float* scale, int scale_is_log, float* rot, float* opacity, int opacity_is_logit, float* f_dc, float* f_rest,
                     int n_coef, int64_t n, const float* cams /*[views][16]*/, int views, int width, int height, float scale_modifier,
                     const float* background /*[3] device*/, const void* target, int target_is_u8, int target_stride, float lambda, int steps,
                     int batch, const int32_t* h_view /*[steps][batch] host*/, const float* h_lr /*[steps][6] host*/,
                     const int32_t* h_sh_degree /*[steps] host*/, const uint8_t* h_reset /*[steps] host*/, int group_mask, float beta1,
                     float beta2, float eps, float reset_ceiling, int64_t max_instances, float* m, float* v, float* history /*[steps][batch]*/,
                     int32_t* status /*[1]*/, int64_t* instances_needed /*[1]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Adaptive density control (additive in ABI 10): the statistics the reference gathers per iteration (train.py:152-160,
 * scene/gaussian_model.py:628-632), one round of its densify_and_prune (gaussian_model.py:539-624) and the fit's loop body with
 * caller-kept state, so that a fit can run with a changing n.  All arithmetic in fp32, no contraction into fused multiply-adds; one
 * owner per output, no floating-point atomics, the same bytes on every call.
 *
 * sixdgs_densify_stats reads the workspace of a completed sixdgs_raster_views (fwd_ws), the workspace of a completed
 * sixdgs_raster_views_backward on the same arguments that wrote at least one output (bwd_ws), neither written since, and the forward's
 * radii [views][n]; it writes nothing to the workspaces.  One lane per Gaussian i, views v in ascending order.  A (v, i) whose tile
 * rectangle is not empty -- exactly when radii[v][i] > 0, the reference's visibility_filter -- contributes:
 *   1. du, dv = the sums of entries 0 and 1 of its instance slots, from 0.f in slot order: the bits the backward chained to the
 *      parameters (dL / d of the centre's pixel coordinates u, v);
 *   2. a = (0.5f width) du, b = (0.5f height) dv, g = sqrtf(a a + b b): the norm of the gradient by the NDC position, which the
 *      reference's threshold 0.0002 is tuned to (the upstream rasteriser scales its pixel gradient by 0.5 W, 0.5 H; that submodule is
 *      not part of the reference tree, so THIS is the definition);
 *   3. grad_accum[i] += g;  denom[i] += 1 (int32);  max_radii[i] = max(max_radii[i], radii[v][i]).
 * A Gaussian that covers tiles but blends into no pixel counts as visible with g = 0, as in the reference.  grad2d [views][n][2] (may
 * be NULL) receives the raw (du, dv): written, not accumulated, exact zeros where the rectangle is empty.  If the recorded instance
 * total exceeds max_instances, or status (int32 [1] device, may be NULL) has bit 1 set, the kernel changes nothing (grad2d included).
 * SIXDGS_E_BADARG / SIXDGS_E_WORKSPACE for argument and workspace errors (the rasteriser's size limits; a NULL or misaligned array;
 * a workspace smaller than sixdgs_raster_views_workspace_bytes / _backward_workspace_bytes say) without touching a GPU; views == 0
 * or n == 0 returns 0.
 *
 * sixdgs_densify is ONE ROUND, out of place: from the six arrays (group order of sixdgs_gaussian_adam), m, v at n, the three
 * statistics and noise [n][2][3] -- standard normals SUPPLIED BY THE CALLER, so the library holds no random-number generator -- into
 * the six arrays and m_out, v_out at n_out rows, in caller buffers of n_cap rows (n_cap (11 + 3 n_coef) floats for m_out, v_out, laid out
 * group after group for n_out rows: the kernels read n_out on the device to place the slices).
 * THRESHOLDS.  The host converts each once, in double, into the domain the array is stored in, and rounds to float:
 *   t_dense from (double) percent_dense * (double) extent, t_world from 0.1 * (double) extent: log() of it when scale_is_log;
 *   t_opacity from p = min_opacity: log(p / (1 - p)) when opacity_is_logit (-inf for p = 0).
 * All comparisons are on STORED values, so classification uses no transcendental.
 * RULES, per Gaussian i:  avg = denom > 0 ? grad_accum / (float) denom : 0;  smax = max_k scale_k (fmaxf);  big = smax > t_dense;
 *   clone = avg >= grad_threshold && !big;  split = avg >= grad_threshold && big.  grad_threshold > 0 is required, so that, as in the
 *   reference (whose split pass sees a zero gradient for the clones just made), a fresh clone is never split.
 * CANDIDATES, in the reference's order: originals that are not split, ascending i; clones, ascending source (exact copies);
 *   children copy 0 of the split sources, ascending source; children copy 1.
 * CHILD of source i, copy j:  xyz + R (sigma * z), R = the rotation matrix of rot_i (normalised twice, as the rasteriser does),
 *   sigma_k = expf(scale_k) (the stored value when not log), z = noise[i][j], out_r = xyz_r + ((R_r0 y_0 + R_r1 y_1) + R_r2 y_2) with
 *   y_k = sigma_k z_k;  scale - 0.470003629f (= logf(1.6), the reference's / (0.8 * 2)) when log, scale / 1.6f otherwise;
 *   everything else copied from the source.
 * PRUNE.  Every candidate is tested on its own stored values: opacity < t_opacity; when prune_big != 0 also max_k scale > t_world;
 *   when prune_big != 0 and screen_size > 0 also max_radii[i] > screen_size, for originals only (clones and children count as 0).
 *   DEVIATION: the reference zeroes max_radii2D in densification_postfix before it prunes (gaussian_model.py:537, :619), so its
 *   screen-size test never fires; screen_size = 0 is the reference's behaviour.
 * COMPACTION.  Survivors are compacted in candidate order (rocPRIM exclusive scan of integer flags).  A surviving original keeps its
 *   rows of m and v; clones and children get zeros.
 * counts [4] (int64, device) = n_out, clones, split sources, candidates pruned (n + clones + splits - n_out).  If n_out > n_cap,
 * nothing is written except counts and bit 1 of status[0] (integer atomic OR; status is not read); n_cap >= 2 n always fits.
 * Limits: those of sixdgs_gaussian_adam; 0 <= n_cap < 2^31; grad_threshold, percent_dense, extent > 0 finite; 0 <= min_opacity < 1;
 * screen_size >= 0.  SIXDGS_E_BADARG (a NULL or misaligned array, an output that is its input, m_out == v_out) and
 * SIXDGS_E_WORKSPACE without touching a GPU; n == 0 writes counts = 0.  sixdgs_densify_workspace_bytes is answered without a GPU
 * (0 outside n < 2^31): two uint32 arrays of 4 n + 1 and the scan's temporary storage, reserved by bound.
 *
 * sixdgs_fit_scene_steps is the loop body of sixdgs_fit_scene with caller-kept state: it does NOT zero m, v, status[0] or
 * instances_needed[0].  Per step s as sixdgs_fit_scene's 1 - 7, with:
 *   - h_stats[s] != 0 (host [steps], NULL = never): behind 5, sixdgs_densify_stats on the step's workspaces and radii (kept in this
 *     call's workspace) into grad_accum, denom, max_radii, with status -- statistics are not accumulated once bit 1 is set;
 *   - h_update[s] == 0 (host [steps], NULL = every step updates): step s makes no Adam update and Adam's counter does not advance;
 *     the u-th update of the call is sixdgs_gaussian_adam's step first_adam_step + u.
 * sixdgs_fit_scene is the zeroing followed by this function with all updates on, no statistics and first_adam_step = 0.
 * sixdgs_fit_scene_steps_workspace_bytes = sixdgs_fit_scene_workspace_bytes plus the radii [batch][n] int32 (0 outside the limits). */
int sixdgs_densify_stats(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                         const void* bwd_ws, size_t bwd_ws_bytes, const int32_t* radii /*[views][n]*/, float* grad_accum /*[n]*/,
                         int32_t* denom /*[n]*/, int32_t* max_radii /*[n]*/, float* grad2d /*[views][n][2] or NULL*/,
                         const int32_t* status /*[1] device or NULL*/, sixdgs_stream_t stream);
size_t sixdgs_densify_workspace_bytes(int64_t n);
int sixdgs_densify(int64_t n, int n_coef, const float* xyz, const float* f_dc, const float* f_rest, const float* opacity, const float* scale,
                   const float* rot, int scale_is_log, int opacity_is_logit, const float* m, const float* v, const float* grad_accum /*[n]*/,
                   const int32_t* denom /*[n]*/, const int32_t* max_radii /*[n]*/, const float* noise /*[n][2][3]*/, float grad_threshold,
                   float percent_dense, float extent, float min_opacity, int prune_big, int screen_size, int64_t n_cap, float* xyz_out,
                   float* f_dc_out, float* f_rest_out, float* opacity_out, float* scale_out, float* rot_out, float* m_out, float* v_out,
                   int64_t* counts /*[4] device*/, int32_t* status /*[1] device*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
size_t sixdgs_fit_scene_steps_workspace_bytes(int64_t n, int n_coef, int batch, int width, int height, int64_t max_instances);
int sixdgs_fit_scene_steps(float* xyz, float* scale, int scale_is_log, float* rot, float* opacity, int opacity_is_logit, float* f_dc,
                           float* f_rest, int n_coef, int64_t n, const float* cams /*[views][16]*/, int views, int width, int height,
                           float scale_modifier, const float* background /*[3] device*/, const void* target, int target_is_u8,
                           int target_stride, float lambda, int steps, int batch, const int32_t* h_view, const float* h_lr,
                           const int32_t* h_sh_degree, const uint8_t* h_reset, const uint8_t* h_update /*[steps] host or NULL*/,
                           const uint8_t* h_stats /*[steps] host or NULL*/, int first_adam_step, int group_mask, float beta1, float beta2,
                           float eps, float reset_ceiling, int64_t max_instances, float* m, float* v, float* history, int32_t* status,
                           int64_t* instances_needed, float* grad_accum, int32_t* denom, int32_t* max_radii, void* ws, size_t ws_bytes,
                           sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Starting a scene from a point cloud (additive in ABI 10): the mean squared distance of every point to its three nearest other
 * points, from which GaussianModel.create_from_pcd (scene/gaussian_model.py:189-228) takes the isotropic start scale
 * log(sqrt(max(d2, 1e-7))); the reference's distCUDA2 (submodules/simple-knn).  An EXACT search, not an approximate one.
 * PAIR DISTANCE.  For points i != j -- distinct by index, not by position --
 *   d2(i, j) = (dx dx + dy dy) + dz dz in fp32, dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i; no contraction into fused multiply-adds.
 * RESULT.  b0 <= b1 <= b2 the three smallest values of the multiset { d2(i, j) : j != i }:  mean_d2[i] = ((b0 + b1) + b2) / 3.0f.
 *   Exact duplicates of a point therefore contribute zeros.
 * BIT DETERMINISM.  Every d2(i, j) is one fixed fp32 number and the three smallest values of a multiset do not depend on the order it
 *   is searched in, so the result is determined to the bit whatever the search structure: it is what a brute force over all pairs
 *   in fp32 gives, and that is the acceptance criterion.
 * SEARCH (informative; csrc/knn.hip, rules in csrc/knn_rules.h).  The points are sorted by a 30-bit Morton code inside their bounding
 *   box -- per axis cell = hi > lo ? clamp((int)((c - lo) / (hi - lo) * 1023.0f), 0, 1023) : 0 -- and cut into boxes of 256 consecutive
 *   sorted points with their AABBs.  The distance from a query to a box, per axis q < lo ? lo - q : (q > hi ? q - hi : 0), summed in
 *   d2's order, is a lower bound of d2 to every point of the box in fp32 itself (every operation in it is monotone), so a box with
 *   box_d2 >= b2 is skipped without changing the result: a candidate that can only tie the third-best value changes none of the
 *   three.  A cloud of identical points is therefore searched in linear time.
 * DEVIATIONS from the reference, stated: its CUDA build may contract the sum into fused multiply-adds (last-ulp differences), and it
 *   divides by a zero extent when an axis of the cloud is flat; this call does neither.  With fewer than four points the reference
 *   returns inf; this call refuses them.
 * LIMITS.  n == 0 returns 0.  1 <= n <= 3 (fewer than three neighbours), n >= 2^31, a NULL or misaligned pointer (xyz, mean_d2: 4 bytes;
 *   ws: 256), mean_d2 overlapping xyz: SIXDGS_E_BADARG.  ws_bytes < sixdgs_knn_workspace_bytes(n): SIXDGS_E_WORKSPACE.  All answered
 *   without touching a GPU, as is sixdgs_knn_workspace_bytes (0 for n < 4 and n >= 2^31): the bounding-box partials, two (code, index)
 *   buffers of n uint32 pairs, the sort's temporary storage reserved by bound, three planes of the sorted points padded to whole boxes
 *   and the box table.
 * PRECONDITION.  Coordinates are finite with |c| < 2^62, so that d2 is finite.  Nothing derived from a coordinate is ever used as an
 *   index (Morton codes are sort keys only, cells are clamped) and every loop is bounded by n or the box count: a violated
 *   precondition gives meaningless numbers, not a fault or a hang.
 * EXECUTION.  Stream-ordered, no host read-back (the bounding box stays on the device), one owner per output, no atomics: the same
 *   bytes on every call. */
size_t sixdgs_knn_workspace_bytes(int64_t n);
int sixdgs_knn_mean_dist2(int64_t n, const float* xyz /*[n][3]*/, float* mean_d2 /*[n]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Held-out-view metrics (additive in ABI 10): per view L1, SSIM and the squared error, whole and per channel, between an image a and
 * a target b -- what the reference's evaluation forms from them (metrics.py:69-89 after the 8-bit PNG round trip of render.py:25-40;
 * train.py:233-289's training_report after a clamp to [0, 1]).  PSNR is not formed here: it is 10 log10(1 / mse), the caller's
 * logarithm, so no transcendental enters the definition.  All fp32 arithmetic without contraction into fused multiply-adds.
 *
 * INPUTS are sixdgs_photometric_loss's: image fp32 [views][height][width][image_stride], image_stride 3 or 4 (the fourth channel is
 * never read); target fp32 with target_stride 3 or 4, or uint8 [views][height][width][3] (target_is_u8 == 1, target_stride 3).
 * INPUT RULE, per value x of an fp32 input (the image, and a float target):
 *   quantise == 0 (training_report's clamp):  value = fminf(fmaxf(x, 0), 1); NaN counts as 0;
 *   quantise == 1 (the PNG round trip):       u = (int) truncf(fminf(fmaxf(x * 255.0f + 0.5f, 0), 255)), value = float(u) / 255.0f;
 *     NaN counts as 0.  This is torchvision's save_image -- mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- followed by to_tensor's
 *     division.  It is NOT sixdgs_raster_views' image_u8 rule round(255 clamp(., 0, 1)): the two differ at about one fp32 value in
 *     10^5 and at half of the exact half points (k + 0.5) / 255, so the bytes are formed here and image_u8 is not read.
 * A uint8 target's value is float(u) / 255.0f in both modes; the 8-bit rule maps each of the 256 such values to its own byte.
 * OUTPUTS.  metrics [views][6] = (l1, ssim, mse, mse_r, mse_g, mse_b), WRITTEN, NOT ACCUMULATED.  With a, b the values after the rule:
 *   ssim: steps 3 - 7 of sixdgs_photometric_loss on a, b -- the same window, zero padding, tile tree and order of tiles;
 *   quantise == 0:  l1 by step 7's tree; with d = a - b, s_c = the sum of d d over channel c's pixels in the same tree (per pixel one
 *     term; tile tree; tiles in row-major order), mse_c = s_c / float(height width), mse = ((s_r + s_g) + s_b) / float(3 height width);
 *   quantise == 1:  both sides are bytes ua, ub: S1 = sum |ua - ub| over all channels and S2_c = sum (ua - ub)^2 per channel are exact
 *     integers (32 bits per tile, 64 per view), and one fp64 division per output rounds once:
 *     l1 = float(double(S1) / (255.0 (3 height width))), mse_c = float(double(S2_c) / (65025.0 (height width))),
 *     mse = float(double(S2_r + S2_g + S2_b) / (65025.0 (3 height width))) -- reproducible to the bit on any host.
 *   render_u8 [views][height][width][3] (may be NULL): the image's bytes by the quantise == 1 rule, whatever quantise is -- what a caller
 *     saves as PNG --, written in the same pass.
 * SAME INPUT, SAME BYTES: no floating-point atomics.  VIEWS DO NOT MIX: metrics[v] and render_u8[v] are the same bits whether view v is
 * passed alone or in a batch.  Nothing is read or written outside the arrays as declared.  image, a float target and metrics are 4-byte
 * aligned, ws 256-byte.  Limits are sixdgs_photometric_loss's: 1 <= width, height <= 16384, views <= 65535, views gx gy < 2^31.
 * Argument errors: SIXDGS_E_BADARG; too small a workspace: SIXDGS_E_WORKSPACE; both without touching a GPU.  views == 0 returns 0.
 * sixdgs_image_metrics_workspace_bytes is answered without a GPU and is 0 outside the limits: 20 B per tile and view.  One 256-thread
 * workgroup per 16 x 16 tile and view, then one per view.  prof (may be NULL) receives one slot per stage: moments, sums.
 *
 * sixdgs_evaluate_views renders and measures many views as one call.  Scene arrays, flags, sh_degree, scale_modifier and background
 * (device [3]) as sixdgs_raster_views takes them; cams [views][16]; the target in the three forms above, views images of width x height.
 * It zeroes status[0] and instances_needed[0], then for each chunk of up to `chunk` (>= 1) consecutive views enqueues on `stream`,
 * through the entry points as they are: sixdgs_raster_views of the chunk's rows (float image only; the count stays on the device),
 * sixdgs_image_metrics into the chunk's rows of metrics (and of render_u8, when given), and a record: instances_needed[0] =
 * max(instances_needed[0], count); if count > max_instances, bit 1 of status[0] is set and the chunk's metrics rows are NaN (its
 * render_u8 rows are unspecified); other chunks are unaffected.  No host synchronisation, no device-to-host copy, no allocation; the
 * library stays stateless; when it returns, the work is enqueued.  metrics[v] is the same bits for every chunk and whether view v is
 * evaluated alone or with others, given a capacity that fits.  Limits and errors are the parts'; views == 0 returns 0.
 * sixdgs_evaluate_views_workspace_bytes is answered without a GPU and is 0 outside the limits: the two parts' workspaces at `chunk`
 * views, one float image of chunk x height x width x 4 and the count, each piece rounded up to 256 B. */
size_t sixdgs_image_metrics_workspace_bytes(int views, int width, int height);
int sixdgs_image_metrics(const float* image /*[views][height][width][image_stride]*/, int image_stride /*3 or 4*/, const void* target,
                         int target_is_u8, int target_stride /*3 or 4; 3 with uint8*/, int views, int width, int height, int quantise,
                         float* metrics /*[views][6]*/, uint8_t* render_u8 /*[views][height][width][3] or NULL*/, void* ws, size_t ws_bytes,
                         sixdgs_stream_t stream, sixdgs_profile* prof);
size_t sixdgs_evaluate_views_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances);
int sixdgs_evaluate_views(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                          const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams /*[views][16]*/,
                          int views, int width, int height, float scale_modifier, const float* background /*[3] device*/, const void* target,
                          int target_is_u8, int target_stride, int quantise, int chunk, int64_t max_instances, float* metrics /*[views][6]*/,
                          uint8_t* render_u8 /*or NULL*/, int32_t* status /*[1]*/, int64_t* instances_needed /*[1]*/, void* ws,
                          size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scorer, scene side (once per scene): ray MLP + k_proj -> key cache
 * replaces RayPreprocessor.forward (ray_preprocessor.py:36-46) + k_proj (our_multihead_attention.py:74)
 * ------------------------------------------------------------------------------------------- */
typedef struct sixdgs_scorer_weights {
  /* padded copies prepared once by sixdgs_pack_weights (zero padding keeps the arithmetic exact) */
  const float* w1; /* [512][144]  mlp.0  (cols 141..143 zero) */
  const float* b1; /* [512] */
  const float* w2; /* [512][512]  mlp.2 */
  const float* b2;
  const float* w3; /* [512][656]  mlp2.0 (cols 653..655 zero) */
  const float* b3;
  const float* w4; /* [384][512]  mlp2.2 */
  const float* b4;
  const float* wk; /* [384][384]  attention.k_proj */
  const float* bk;
  const float* wq; /* [384][400]  attention.q_proj (cols 398,399 zero) */
  const float* bq;
  /* max |w| of every row of w1 .. wk: the static operand scales of the scaled-fp16 x 3 dense layers (SIXDGS_MMA_DEFAULT / F16X3) */
  const float* m1; /* [512] */
  const float* m2; /* [512] */
  const float* m3; /* [512] */
  const float* m4; /* [384] */
  const float* mk; /* [384] */
  /* k_proj folded into layer 4 (no non-linearity between them: ray_preprocessor.py:27-31,46, our_multihead_attention.py:74):
   * K = (Wk W4) h3 + (Wk b4 + bk), composed in fp64 by sixdgs_pack_weights and rounded to fp32 once */
  const float* w4k; /* [384][512] */
  const float* b4k; /* [384] */
  const float* m4k; /* [384] max |w4k| per row */
  const void* planes; /* w1 .. wk, w4k pre-split into scaled fp16 planes [row][k-slabs][2][32] (w3 as [h | x padded to 160]): the operands of the
                         plane-to-plane ray MLP chain that sixdgs_ray_keys_ex runs when only keys / key planes are asked for */
} sixdgs_scorer_weights;

size_t sixdgs_packed_weights_floats(void);
/* Packs the reference state_dict tensors (SURVEY.md §8(b) shapes) into one caller buffer and fills
 * `out` with pointers into it. */
int sixdgs_pack_weights(const float* mlp0_w, const float* mlp0_b, const float* mlp2_w, const float* mlp2_b,
                        const float* mlp2_0_w, const float* mlp2_0_b, const float* mlp2_2_w, const float* mlp2_2_b,
                        const float* kproj_w, const float* kproj_b, const float* qproj_w, const float* qproj_b,
                        float* packed, sixdgs_scorer_weights* out, sixdgs_stream_t stream);

/* a12: x[R,144] = [pts, dir, rgb, PE(pts,8), PE(dir,8), PE(rgb,6), 0,0,0] */
int sixdgs_ray_encode(const float* ori, const float* dir, const float* rgb, int64_t r, float* x, sixdgs_stream_t stream);

/* a13 + k_proj.  feat (may be NULL) receives the [R,384] ray features, key the [R,384] keys.
 * Rays are processed in chunks sized by the workspace (any ws >= the minimum works). */
size_t sixdgs_ray_keys_workspace_bytes(int64_t r, int64_t max_chunk);
int sixdgs_ray_keys(const float* ori, const float* dir, const float* rgb, int64_t r, const sixdgs_scorer_weights* w,
                    float* feat, float* key, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
/* same, timing the whole MLP chain of each chunk (2 025 472 algorithmic FLOP per ray) into `prof` */
/* key_planes (optional; mma_mode F16X3 / F16X3_L32 / DEFAULT only, SIXDGS_E_UNSUPPORTED otherwise): the keys as scaled fp16 planes
 * (sixdgs_key_planes_f16_bytes(r) bytes, 1536 B per ray) -- the operand of the DMA-fed scorer kernels and of the select path -- and
 * key_inv_scale[ceil(r/128)] (device, required) receives the per-tile reciprocal scales.  With key == NULL only the planes are kept.
 * (Rounds 1-5 also had a three-plane bf16 format for a bf16 x 6 plane scorer; kernel and format were removed in round 6, ABI 6.) */
/* d_key_norm_max (device scalar, may be NULL; scaled fp16 planes only): *d_key_norm_max = max(*d_key_norm_max, max over these rays of
 * |key row|), rounded up -- the bound sixdgs_score_select / sixdgs_select_candidates take; zero it before the first chunk of a scene.
 * Free when k_proj writes the planes itself (its epilogue has the rows), one pass over the planes otherwise. */
int sixdgs_ray_keys_ex(const float* ori, const float* dir, const float* rgb, int64_t r, const sixdgs_scorer_weights* w,
                       float* feat, float* key, void* key_planes, float* key_inv_scale, float* d_key_norm_max, void* ws,
                       size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof, int mma_mode);
/* fp32 rows -> scaled fp16 planes [rows][12][2][32] (1536 B per row) for SIXDGS_MMA_F16X3: every 128-row tile is scaled
 * by the power of two that puts its largest magnitude in [2^13, 2^14); d_inv_scale[ceil(rows/128)] (device) receives the
 * reciprocal scales.  Splitting a row range in chunks is valid when every chunk starts at a multiple of 128 rows. */
size_t sixdgs_key_planes_f16_bytes(int64_t r);
int sixdgs_split_planes_f16(const float* src, int64_t rows, int64_t ld, void* planes, float* d_inv_scale, sixdgs_stream_t stream);

/* generic fp32 MFMA GEMM used by the above: y[M,N] = act(x[M,K] . w[N,K]^T + b), K % 16 == 0,
 * N % 128 == 0, ldx/ldw/ldy in floats and multiples of 4. */
int sixdgs_linear(const float* x, int64_t m, int k, int64_t ldx, const float* w, int64_t ldw, const float* b, int n,
                  int relu, float* y, int64_t ldy, sixdgs_stream_t stream);
int sixdgs_linear_ex(const float* x, int64_t m, int k, int64_t ldx, const float* w, int64_t ldw, const float* b, int n,
                     int relu, float* y, int64_t ldy, sixdgs_stream_t stream, int mma_mode);
/* The same product with K cut into `slices` parts computed by separate workgroups and added in ascending order
 * (deterministic): for few output tiles and a long K (the camera-up CNN as im2col GEMMs: M <= a few hundred, K = 9600). */
size_t sixdgs_linear_splitk_workspace_bytes(int64_t m, int n, int slices);
int sixdgs_linear_splitk(const float* x, int64_t m, int k, int64_t ldx, const float* w, int64_t ldw, const float* b, int n,
                         int relu, float* y, int64_t ldy, int slices, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                         int mma_mode);

/* The dense products of the backbone stage (pose_estimation/backbone.py:82-114 runs DINOv2 ViT-S/14 on every query image) with the
 * elementwise work around them folded in: y = epilogue( prologue(x) . w^T + bias ), fp32 results (two scaled fp16 planes per operand, three cross terms,
 * fp32 accumulation), tiles of 64 token rows x 256 features -- sized for token matrices of 257 .. 4112 rows.  The weights are constants and are split
 * ONCE: sixdgs_tok_pack turns w [n][ldw] (n a multiple of 128, k a multiple of 384) into sixdgs_tok_pack_bytes(n, k) bytes of planes in the matrix
 * pipe's operand order + n reciprocal row scales; sixdgs_tok_linear takes those.
 *   a_mode   SIXDGS_TOK_A_PLAIN  x [m][ldx];
 *            SIXDGS_TOK_A_LAYERNORM  LayerNorm(x; ln_weight, ln_bias, ln_eps) over the k = 384 columns in front of the product (torch.nn.LayerNorm,
 *                                dinov2 block.norm1 / norm2);
 *   epilogue SIXDGS_TOK_EPI_BIAS  y [m][ldy] = acc + bias;   SIXDGS_TOK_EPI_GELU  gelu(acc + bias), erf form (mlp.fc1 + act; erf to 4.1e-7:
 *                                Abramowitz & Stegun 7.1.26's 1.5e-7 plus its fp32 evaluation with the hardware's reciprocal and exp2; measured 3.3e-7);
 *            SIXDGS_TOK_EPI_RESID  residual [m][ldr] + gamma[n] * (acc + bias) (x + ls(branch(x)): attn.proj / mlp.fc2, LayerScale gamma or NULL = 1;
 *                                y may be the residual buffer itself).
 * Pinned against fp64, element by element (tests/vit_stage_reference.py; u = 2^-23; measured figures in profiles/vit_stage_edges.md):
 *   v = prologue(x) . w^T + bias:  |dv_ij| <= 4e-7 (sum_k |xh_ik| |w_jk| + |bias_j|) + u |v_ij| + 2^-125 (sum_k |w_jk| + 1), xh = x or LayerNorm(x);
 *   LayerNorm prologue:            + 0.5 u (1 + max_k |x_ik| / sqrt(var_i + eps)) sum_k |ln_weight_k| |w_jk|;
 *   GELU:                          |dy| <= 1.13 |dv| + 0.5 |v| 4.1e-7 + u |y|;  gelu(-40) = -0, never NaN;
 *   residual:                      |dy| <= |gamma_j| |dv| + u (|residual_ij| + |gamma_j v_ij|).
 *   (the 2^-125 term: a row's power-of-two scale is clamped to 2^+-100, so rows whose largest magnitude lies below 2^-113 keep an absolute grid.)
 * Rows never mix: row i of y depends on row i of x (and of residual), the weights and a fixed order of operations alone -- the same bits whatever m,
 * ldx, ldy, ldr, the row's place in its 64-row tile, the number of feature tiles a workgroup walks, in place or not; a NaN / Inf row of x makes its own
 * output row non-finite and no other.  Rows of x, residual and y beyond m are neither read nor written, nor are columns beyond k / n.  An all-zero row of
 * x gives exactly bias (plain prologue, bias epilogue) or the product of ln_bias (LayerNorm); an all-zero row of w gives exactly bias_j before the epilogue. */
#define SIXDGS_TOK_A_PLAIN 0
#define SIXDGS_TOK_A_LAYERNORM 1
#define SIXDGS_TOK_EPI_BIAS 0
#define SIXDGS_TOK_EPI_GELU 1
#define SIXDGS_TOK_EPI_RESID 2
size_t sixdgs_tok_pack_bytes(int n, int k);
int sixdgs_tok_pack(const float* w /*[n][ldw]*/, int n, int k, int64_t ldw, void* planes, float* inv_scale /*[n]*/, sixdgs_stream_t stream);
int sixdgs_tok_linear(const float* x, int64_t m, int k, int64_t ldx, int a_mode, const float* ln_weight, const float* ln_bias, float ln_eps,
                      const void* w_planes, const float* w_inv_scale, const float* bias /*[n] or NULL*/, int n, int epilogue, const float* residual,
                      int64_t ldr, const float* gamma, float* y, int64_t ldy, sixdgs_stream_t stream);

/* The attention of a ViT block (dinov2 Attention.forward: softmax(q k^T / sqrt(64)) v per image and head) on the QKV product's output as it lies:
 * qkv [images * tokens][ldq] = q | k | v, each heads * 64 wide, head h at columns h * 64; y [images * tokens][ldy], head h at columns h * 64 (what
 * attn.proj reads).  Head dimension 64, tokens <= 288 (SIXDGS_E_UNSUPPORTED beyond: the caller keeps its own attention); fp32-class results.
 * Pinned against fp64 per (image, head, query) (tests/vit_stage_reference.py): |dy_qd| <= (8e-7 Lambda_q + 4e-7) s_q, Lambda_q = max_key sum_d |q_d| |k_d| / 8,
 * s_q = sum_key p_key max_d |v_key,d|.  Images and heads never mix: the output of (image, head) depends on that image's rows and that head's 3 x 64 columns
 * alone -- the same bits whatever the batch, the strides and the number of query groups the launcher chooses; NaN in one image or one head's columns stays
 * there.  Rows of qkv beyond images * tokens and columns beyond 3 * heads * 64 are not read.  K = 0 for a head (scale 0) gives the mean of the head's V rows
 * over exactly `tokens` keys; V = 0 gives exactly 0. */
int sixdgs_tok_attention(const float* qkv, int64_t ldq, int images, int tokens, int heads, float* y, int64_t ldy, sixdgs_stream_t stream);

/* a22 (camera_direction_network.py:29-36, the valid k x k convolutions of the camera-up CNN) as GEMMs: the im2col matrix of a whole batch in one
 * launch.  a [batch * ho * wo][channels * k * k] (ho = height - k + 1, wo = width - k + 1): row (b, oy, ox); column (c, ky, kx) -- the order of
 * conv.weight.view(out, -1) -- or, taps_major != 0, (ky, kx, c) (for weights whose columns the caller permuted the same way: with channel-contiguous
 * input every (row, tap) is then a copy of `channels` consecutive floats); value x[b * stride_b + c * stride_c + (oy + ky) * stride_y + (ox + kx) * stride_x],
 * strides in elements, free (NCHW, or the [B * ho * wo][C] output of the previous layer's GEMM read in place). */
int sixdgs_im2col(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x, int batch, int channels, int height, int width, int k,
                  int taps_major, float* a, sixdgs_stream_t stream);

/* a16, first step, for a batch (pose_estimation/test.py:69-73: uint8 image / 255.0): images [batch][pixels][3] uint8 -> out [batch][3][pixels] fp32,
 * out = table256[value] (the caller's table carries the reference's true division); pixels a multiple of 4. */
int sixdgs_u8_to_planar(const uint8_t* images, int batch, int64_t pixels, const float* table256, float* out, sixdgs_stream_t stream);

/* a16 + the wrapper's transform pipeline for a batch of RGB images of one size (pose_estimation/test.py:69-73, backbone.py:52-77: uint8 / 255.0 -> Resize(256,
 * bicubic, antialias) -> CenterCrop(224) -> Normalize) in one pass: images [batch][height][width][3] uint8 -> out [batch][3][out_size][out_size] fp32 =
 * (crop(resize_aa(table256[value])) - mean3[c]) / std3[c].  The caller states the geometry the reference's transforms would use: the resized grid
 * (resized_h, resized_w) and the crop's corner in it.  The arithmetic is the antialiased bicubic of the op it replaces (spans, a = -0.5 filter, tap-order sums, rows
 * reduced along x first), with the x-reductions shared between the output rows of a band; mean3 / std3 are HOST arrays (read at the call).  SIXDGS_E_UNSUPPORTED for
 * scales beyond 15 or windows that do not fit the kernel's LDS: the caller keeps PyTorch's kernels for those. */
int sixdgs_image_prep(const uint8_t* images, int batch, int height, int width, const float* table256, int resized_h, int resized_w, int crop_top, int crop_left,
                      int out_size, const float* mean3, const float* std3, float* out, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scorer, image side (per batch of query images)
 * replaces MultiHeadAttention.forward (our_multihead_attention.py:70-79, 4-12),
 * IdentificationModule.run_attention's column sum (identification_module.py:80-82) and
 * torch.topk (identification_module.py:131)
 * ------------------------------------------------------------------------------------------- */
/* q[b] = tokens[b] . Wq^T + bq.  tokens [B, 256, 398] (rows >= n_tok[b] ignored), q [B,256,384]
 * (rows >= n_tok[b] are written as zeros).  d_n_tok: device int32 [B], 0 <= n_tok <= 256. */
int sixdgs_q_proj(const float* tokens, const int32_t* d_n_tok, int batch,
                  const sixdgs_scorer_weights* w, float* q, sixdgs_stream_t stream);

/* scores[b][r] = sum_{t < n_tok[b]} softmax_r(q[b][t] . key[r] / sqrt(384)); idx/val = top-k (sorted
 * descending, ties -> lowest index).  scores may be NULL (then they live only in the workspace).
 * q rows at or beyond n_tok[b] are NOT READ, in any mode and by every entry point of the scorer (sixdgs_score_topk[_ex],
 * sixdgs_score_pass1): they may hold anything -- NaN, Inf, values of any magnitude -- without changing a bit of the scores, the
 * top-k or the row statistics of the rows below n_tok[b] (row_stats rows at or beyond n_tok[b] are unspecified).
 * Never materialises more than `ws` allows: images are processed in groups that fit. */
size_t sixdgs_score_topk_workspace_bytes(int64_t r, int batch, int topk);   /* enough for every mode */
/* exact for a mode: with key planes in F16X3 / DEFAULT the logits take 784 instead of 1024 B per ray and image */
size_t sixdgs_score_topk_workspace_bytes_ex(int64_t r, int batch, int topk, int mma_mode, int with_key_planes);
int sixdgs_score_topk(const float* q /*[B,256,384]*/, const int32_t* d_n_tok, int batch, const float* key /*[R,384]*/,
                      int64_t r, int topk, float* scores /*[B,R] or NULL*/, int64_t* idx /*[B,topk]*/,
                      float* val /*[B,topk]*/, float* row_stats /*[B,256,2] (max, sumexp) or NULL*/, void* ws,
                      size_t ws_bytes, sixdgs_stream_t stream);
/* same, timing each launch of the logits kernel (2*T*384 algorithmic FLOP per ray and image) into `prof` */
/* key_planes != NULL in the F16X3 / F16X3_L32 / DEFAULT modes selects the DMA-fed kernel: scaled fp16 planes + d_key_scale (the d_inv_scale of
 * sixdgs_split_planes_f16 / sixdgs_ray_keys_ex); `key` (fp32) may then be NULL.  SIXDGS_MMA_F32 / _BF16X6 score on `key` (fp32 MFMA chain / bf16 x 6
 * with the split on the fly) and ignore the planes; planes without `key` in those modes: SIXDGS_E_UNSUPPORTED. */
int sixdgs_score_topk_ex(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok /*host copy, for the FLOP count*/,
                         int batch, const float* key, const void* key_planes, const float* d_key_scale, int64_t r, int topk,
                         float* scores, int64_t* idx, float* val, float* row_stats, void* ws, size_t ws_bytes,
                         sixdgs_stream_t stream, sixdgs_profile* prof, int mma_mode);

/* Ray-sharded scoring (SURVEY 8(e) fallback: the key cache of a scene is split across GPUs, or one image must be scored by
 * several).  The softmax runs over ALL rays, so the scorer is cut at the row statistics:
 *   pass 1  logits of this shard's rays for ALL `batch` images stay in the workspace (SIXDGS_E_WORKSPACE if they do not
 *           fit: sixdgs_score_topk_workspace_bytes(r, batch, topk)); row_stats[B,256,2] receives the shard's (max, sumexp);
 *   caller  combines the shards: M = max over shards, S = sum over shards of s * exp(m - M)  (two tiny all-reduces);
 *   pass 2  takes the global statistics, writes this shard's scores and its local top-k (indices local to the shard);
 *           the global top-k is the (value desc, global index asc) merge of the shards' candidates.
 * Same r, batch, topk, workspace and mma_mode in both passes; used_planes = pass 1 ran on key planes. */
int sixdgs_score_pass1(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok, int batch, const float* key,
                       const void* key_planes, const float* d_key_scale, int64_t r, int topk, float* row_stats, void* ws,
                       size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof, int mma_mode);
int sixdgs_score_pass2(const float* row_stats, const int32_t* d_n_tok, int batch, int used_planes, int64_t r, int topk,
                       float* scores, int64_t* idx, float* val, void* ws, size_t ws_bytes, sixdgs_stream_t stream, int mma_mode);
/* Backward of scores[b][r] = sum_t softmax_r(q[b][t] . key[r] / sqrt(384)) (training).  g [B,R] = dL/dscores; row_stats [B,256,2] =
 * the forward's (max, sumexp), as sixdgs_score_pass1 returns them.  With A = softmax, c[b][t] = sum_r A g and dS = A (g - c):
 *   dq [B,256,384] = sum_r dS key[r] / sqrt(384)          rows t >= d_n_tok[b] are written as zeros (and q's rows there are not read)
 *   dk [R,384]     = sum_b sum_t dS q[b][t] / sqrt(384)
 * The logits are recomputed from q and key (fp32 MFMA) with the forward's max as the exponent offset; the softmax sum is recomputed
 * with c, on the same logits.  Nothing of size B x T x R is stored.  No floating-point atomics: the same inputs give the same bits.
 * d_n_tok[b] = 0 is legal and contributes nothing.  ws: sixdgs_score_backward_workspace_bytes(batch) bytes (c and the sums, 2 x B x 256
 * floats).  q, key, dq and dk 16-byte aligned, all arrays dense. */
size_t sixdgs_score_backward_workspace_bytes(int batch);
int sixdgs_score_backward(const float* q, const int32_t* d_n_tok, int batch, const float* key /*[R,384]*/, int64_t r,
                          const float* row_stats, const float* g, float* dq, float* dk, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
/* sixdgs_score_backward with the rays of each 128-token tile split into ray_groups = G contiguous ranges of whole 128-ray tiles, so that
 * 2 x B x G workgroups share the work of k_bwd_q's 2 x B (a small window -- a rank's share of a data-parallel iteration -- fills the GPU).
 * Each group writes its partial softmax sums and c terms, then its partial dq, to the workspace; both are summed over g = 0 .. G-1 in that
 * order (no atomics: the same inputs and G give the same bits; different G differ by rounding).  dk as in sixdgs_score_backward.
 *   ray_groups = 1  k_bwd_q + k_bwd_k: the bits of sixdgs_score_backward (as does any G that resolves to 1: R <= 128 rays, B = 0)
 *   ray_groups = 0  auto: G = ceil(CUs / (2 B)), so that the partial kernels cover every compute unit once
 *   ray_groups < 0  SIXDGS_E_BADARG
 * G is clamped to the number of 128-ray tiles and to 1024.  ws: sixdgs_score_backward_split_workspace_bytes(batch, r, ray_groups) bytes,
 * 16-byte aligned: c and the sums (2 x B x 256 floats), the partial sums [G][B][256][2] and the partial dq [G][B][256][384] floats --
 * G x B x 393 KB, about 50 MB with auto G on 256 CUs (2 x B x G = 256 workgroups x 128 rows x 384 floats) at any B. */
size_t sixdgs_score_backward_split_workspace_bytes(int batch, int64_t r, int ray_groups);
int sixdgs_score_backward_split(const float* q, const int32_t* d_n_tok, int batch, const float* key /*[R,384]*/, int64_t r,
                                const float* row_stats, const float* g, float* dq, float* dk, int ray_groups, void* ws, size_t ws_bytes,
                                sixdgs_stream_t stream);
/* Top-k WITHOUT materialising the logits -- the inference path, where only idx/val are wanted (the reference driver reads nothing
 * else: test.py:105-107).  Needs the scaled fp16 key planes of ALL r rays (sixdgs_ray_keys_ex, SIXDGS_MMA_F16X3) and those of a
 * ray SAMPLE (any r_sample <= r rays of the same scene, e.g. one ray in 16, through the same entry point).  score[r] =
 * sum_t e[t][r] / Z_t with e = exp(logit - ref_t), Z_t = sum_r e[t][r]:
 *   pre-pass    over the sample: ref_t = sample maximum, Z~_t = sample sum (so that f Z~_t ~ Z_t, f = r / r_sample).  Since round 6 with ONE of the
 *               three MFMA terms (h x h: logits to ~2^-11 |q||k| / sqrt(384); SIXDGS_PREPASS_TERMS=3 restores all three): these two only set the sweep's
 *               exponent offsets and scale -- g_t below is exact relative to WHATEVER Z~_t the sweep was given;
 *   main sweep  over all rays, one matrix-core pass, nothing of size T x R leaves the chip: U[r] = sum_t e[t][r] / (f Z~_t)
 *               (4 x 4 B per ray and image instead of 784 B of logits) and the EXACT g_t = Z_t / (f Z~_t);
 *   bounds      score[r] = sum_t e'[t][r] / g_t lies in [U[r] / g_max, U[r] / g_min], so every ray of the true top-k has
 *               U[r] >= U_(k) g_min / g_max (1 - eps) / (1 + eps) (U_(k) = k-th largest U).  eps bounds the relative difference between
 *               the sweep's U and the exact re-score: eps = 1.4e-4 x + 1.3e-5 with x = max_t |q_t| max_r |k_r| / sqrt(384) >= every
 *               sum_i |q_i k_i| / sqrt(384) (fp32 accumulation of 1152 products in the MFMAs + the epilogue's roundings; derivation at
 *               k_sel_bounds).  d_key_norm_max (device scalar): max_r |k_r| of the scene, from sixdgs_key_planes_norm_max;
 *   re-score    those candidates exactly (fp32, from their key planes and the exact g_t); their top-k (value descending, ties ->
 *               lowest index) is the result.  The sample decides only how many candidates there are, never the answer.
 * d_status[b] (device) = number of candidates examined, or -1 when this image must be scored by sixdgs_score_topk_ex instead
 * (more than max_candidates candidates, or an exponent overflow because a logit exceeds the sample maximum by > 88).
 * max_candidates: multiple of 8, >= topk.  Workspace ~ 20 B per ray and image. */
size_t sixdgs_score_select_workspace_bytes(int64_t r, int batch, int topk, int max_candidates);
/* *d_norm_max = max(*d_norm_max, max over the rows of |x_row|) for the values the scaled fp16 planes hold (rounded up: it is used as a
 * bound).  Zero *d_norm_max before the first call; scenes that go through in chunks accumulate chunk by chunk. */
int sixdgs_key_planes_norm_max(const void* planes, const float* d_scale, int64_t rows, float* d_norm_max, sixdgs_stream_t stream);
/* The four stages of the select path as entry points of their own, for scenes whose key planes do not fit the GPU: `begin` once
 * (sample pre-pass), `sweep` per ray chunk (chunks start at multiples of 256 rays; each writes its columns of U and adds its
 * share of the exact per-token sums into gsum), `candidates` once over the whole U, then `rescore` on the key planes of the
 * candidates alone.  All buffers are the caller's: ctok, gsum [B,256] floats; U [B][u_stride] floats (u_stride >= r rounded up
 * to 256); cand [B][max_candidates] int64 (ascending ray indices); d_count [B] int32 (candidates, may exceed max_candidates;
 * -1 bounds unusable; -2 image without tokens).  sixdgs_select_workspace_bytes(r, ...) with the largest r of any call.
 * rescore: `planes` are either the scene's key planes (compact == 0: rows addressed by ray index, scales per 128 rays) or the
 * planes of exactly the candidates in candidate order (compact != 0: row b * max_candidates + c, scales per 128 ROWS), e.g.
 * from sixdgs_ray_keys_ex on the gathered rays. */
size_t sixdgs_select_workspace_bytes(int64_t r, int batch, int topk, int max_candidates);              /* begin, sweep: r = rays of the call */
size_t sixdgs_select_candidates_workspace_bytes(int64_t r, int batch, int topk, int max_candidates);   /* candidates (r = all rays), rescore */
/* h_n_tok (begin, sample_stats, sweep, sixdgs_score_select; may be NULL): a HOST copy of d_n_tok.  With it the images of a launch are PACKED by their
 * token counts into the 256-token tiles of the matrix-core sweep (two views of <= 128 tokens, four of <= 64, 192 + 64 ... share a tile; ABI 5), so a
 * masked view costs what its surviving tokens cost (the reference scores only those: backbone.py:86-114, identification_module.py:80-82).  It MUST equal
 * d_n_tok; an image the host copy gives too few tokens is reported undecidable (status -1), never scored without some of its tokens.  Results do not
 * depend on it: an image's U, sums and statistics are the same bits packed or alone.  NULL: one image per tile (and 256 tokens each in the FLOP count). */
/* How sixdgs_select_sweep / _sample_stats / sixdgs_score_select cut `batch` images with these token counts (NULL: unknown) into launches: returns the
 * number of launches (>= 0; < 0 an error) and fills, for the first max_launches of them, the 256-token tiles ("slots") and the images of each.  Host
 * arithmetic only (csrc/sweep_plan.h); for reporting and tests. */
int sixdgs_select_sweep_plan(const int32_t* h_n_tok, int batch, int32_t* slots_per_launch, int32_t* images_per_launch, int max_launches);
int sixdgs_select_begin(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok, int batch, const void* sample_planes, const float* d_sample_scale,
                        int64_t r_sample, int64_t r_total, float* ctok, float* gsum, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
/* Ray-sharded select (the scene's key planes split over ranks, SURVEY 8(e) fallback): `begin` in two halves, so that the shards can
 * merge their sample statistics in between -- sample_stats writes this shard's (max, sumexp) [B,256,2] of ITS sample; the caller
 * merges (M = max, S = sum s e^(m - M): two all-reduces of 1 KB per image) and hands the global statistics to prepare together with
 * the TOTAL sample and ray counts.  Then per shard: sweep -> all-reduce(SUM) of gsum, all-reduce(MAX) of the key norm ->
 * sixdgs_select_topk_u (the shard's k largest U, descending, NaN-padded) -> all-gather, k-th largest of the union = U_(k) of the
 * scene -> candidates with d_uk [B] -> rescore with allow_fewer (a shard may hold fewer than k candidates: idx / val are then padded
 * with -1 / NaN and status = candidates examined) -> all-gather + (value desc, global index asc) merge. */
int sixdgs_select_sample_stats(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok, int batch, const void* sample_planes, const float* d_sample_scale,
                               int64_t r_sample, float* row_stats /*[B,256,2]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
int sixdgs_select_prepare(const float* row_stats, const int32_t* d_n_tok, int batch, int64_t r_sample, int64_t r_total, float* ctok, float* gsum,
                          sixdgs_stream_t stream);
int sixdgs_select_topk_u(const float* u, int64_t u_stride, int64_t r, const float* u_tile_max /*or NULL*/, int batch, int topk, float* val /*[B,topk]*/,
                         void* ws, size_t ws_bytes, sixdgs_stream_t stream);        /* ws: sixdgs_select_candidates_workspace_bytes */
/* u_tile_max (optional, [B][u_stride / 256] floats, u_stride a multiple of 256; a chunk passes u + ray_offset and u_tile_max + ray_offset / 256):
 * the largest U of every 256-ray tile.  The k-th largest tile maximum is a lower bound of the k-th largest U -- k tiles hold a ray that large --
 * and with the top rays scattered over r / 256 tiles practically equal to it; `candidates` (and `topk_u`) take it from these r / 256 values
 * instead of a radix select over all r values of U (six passes less over U per batch).  A lower threshold admits a few more candidates, never fewer. */
int sixdgs_select_sweep(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok, int batch, const void* key_planes,
                        const float* d_key_scale, int64_t r, const float* ctok, float* gsum, float* u, int64_t u_stride, float* u_tile_max,
                        void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof);
int sixdgs_select_candidates(const float* u, int64_t u_stride, int64_t r, const float* u_tile_max /*or NULL*/, const float* q, const int32_t* d_n_tok, int batch, const float* gsum,
                             const float* d_key_norm_max, const float* d_uk /*[B] k-th largest U of the whole scene, or NULL = of these rays*/,
                             int topk, int max_candidates, int64_t* cand, int32_t* d_count, void* ws, size_t ws_bytes, sixdgs_stream_t stream);
int sixdgs_select_rescore(const float* q, const int32_t* d_n_tok, int batch, const void* planes, const float* d_scale, int compact,
                          const float* ctok, const float* gsum, const int64_t* cand, const int32_t* d_count, int64_t r, int topk,
                          int max_candidates, int allow_fewer, int64_t* idx, float* val, int32_t* d_status, void* ws, size_t ws_bytes,
                          sixdgs_stream_t stream);
int sixdgs_score_select(const float* q, const int32_t* d_n_tok, const int32_t* h_n_tok /*host copy for the FLOP count, may be NULL*/,
                        int batch, const void* key_planes, const float* d_key_scale, const float* d_key_norm_max, int64_t r,
                        const void* sample_planes, const float* d_sample_scale, int64_t r_sample, int topk, int max_candidates, int64_t* idx /*[B,topk]*/,
                        float* val /*[B,topk]*/, int32_t* d_status /*[B]*/, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                        sixdgs_profile* prof);
/* top-k alone over precomputed scores [B,R] */
size_t sixdgs_topk_workspace_bytes(int64_t r, int batch, int topk);
int sixdgs_topk(const float* scores, int64_t r, int batch, int topk, int64_t* idx, float* val, void* ws,
                size_t ws_bytes, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Pose assembly (per image) -- replaces pose_estimation/test.py:157-198,216-218 with
 * line_intersection.py:5-34,75-154 and error_computation.py:3-8
 * ------------------------------------------------------------------------------------------- */
/* SURVEY 8(f)#1, forward part: the target scores of DistanceBasedScoreLoss (distance_based_loss.py:5-71,179-222) for the
 * ground-truth camera d_pose (device, row-major c2w 4x4): 1 - tanh(distance of the camera centre to each ray), zero for ray
 * origins behind the camera plane, rescaled so that the targets sum to n_tokens.  d_sum (device scalar, may be NULL)
 * receives the un-scaled sum.  The loss value mean((pred - target)^2) and its gradient stay with the caller (PyTorch). */
size_t sixdgs_distance_target_workspace_bytes(int64_t r);
int sixdgs_distance_target(const float* rays_ori, const float* rays_dir, int64_t r, const float* d_pose, int n_tokens,
                           float* target /*[r]*/, float* d_sum, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

/* For each image b: duplicate-origin filter, unweighted LS centre (NaN when det < 1e-7),
 * exclude_negatives reweighting, watch direction, make_rotation_mat(-watch, up[b]), singular -> I,
 * c2w = [inv(R) | centre], NaN -> I4.
 * A POSITION is an entry 0..k-1 of idx[b,:]; it is VALID when 0 <= idx < r (other entries are padding, at any position: they
 * neither filter nor solve, and val is not read there).  The valid positions are taken in index order: a padded list gives the
 * bits of the call on the list without its padding.  No valid position: identity, status bits 1 and 2, n_kept 0.  1 <= k <= 256.
 * outputs: c2w [B,4,4]; status [B] bit0 = singular rotation, bit1 = NaN pose (identity returned),
 * bit2 = NaN centre; w_final [B,k] (0 for filtered rays and for padding), n_kept [B]; errors [B,2] =
 * (translation error, angular error in degrees) against gt_c2w when gt_c2w != NULL. */
int sixdgs_solve_pose(const float* rays_ori, const float* rays_dir, int64_t r, const int64_t* idx /*[B,k]*/,
                      const float* val /*[B,k]*/, int k, const float* up /*[B,3]*/, const float* gt_c2w /*[B,4,4]*/,
                      int batch, float* c2w, int32_t* status, float* w_final, int32_t* n_kept, float* centre /*[B,3]*/,
                      float* errors, sixdgs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Consensus pose solver (added under ABI 10, additive: nothing above changes signature or meaning).  A hypothesise-and-verify
 * estimator of the camera centre over the same top-k, for top-k lists in which many rays do not see the camera; the pose is
 * then assembled as by sixdgs_solve_pose.  Deterministic, no random numbers.  All arithmetic in fp32.
 *
 * Per image b.  A POSITION is an entry 0..k-1 of idx[b,:]; it is VALID when 0 <= idx < r (other entries are padding: they
 * neither vote nor form hypotheses); n = number of valid positions.  o_i, d_i: origin and (unit) direction of the ray at
 * position i.  There is no duplicate-origin filter.  Prior p_i: prior = 0: 1/n; prior = 1: v_i / sum v with v_i = val[b,i]
 * where that is > 0, else 0.  tau > 0: inlier scale in scene units.
 *   r_i(c)     distance of c to the line (o_i, d_i): |v - (v.d_i) d_i| with v = c - o_i;    front_i(c) = [(c - o_i).d_i > 0].
 *  1. Hypotheses: pairs of positions (i, j).  k <= 256: every pair i < j.  k > 256: (i, (i + m) mod k), m = 1..floor(32768 / k)
 *     (the top-k is sorted by score: each ray meets its neighbours in rank).  With w0 = o_i - o_j, b = d_i.d_j, d = d_i.w0,
 *     e = d_j.w0, den = 1 - b^2, s = (b e - d) / den, t = (e - b d) / den the candidate is the midpoint of the closest approach,
 *     c = ((o_i + s d_i) + (o_j + t d_j)) / 2.  A pair is INVALID when a position of it is padding, den <= 1e-6, s <= 0 or t <= 0
 *     (the camera is in front of both rays).
 *  2. Support S(c) = sum_i p_i front_i(c) / (1 + (r_i(c) / tau)^2), in [0, 1], summed in position order.  The winner is the valid
 *     hypothesis of largest S; equal S: the smallest (i, j) in lexicographic order, (i, j) as listed in 1.  (The sweep evaluates S
 *     with the prior left un-normalised and a hardware reciprocal -- neither changes the order beyond fp32 rounding; hypotheses
 *     whose supports differ by less than that are the same basin, and the refinement below takes them to the same centre.)
 *  3. Refinement from the winner's c, 8 iterations, tau fixed: w_i = p_i front_i(c) / (1 + (r_i(c) / tau)^2)^2,
 *     c <- solve(sum w_i (I - d_i d_i^T), sum w_i (I - d_i d_i^T) o_i) (LU with partial pivoting).  A determinant that is not
 *     positive or < 1e-7 (sum w_i)^3, or a non-finite solution, ends the refinement at the last good c.  SUMS over the rays
 *     (here and below) run on a fixed tree: positions in groups of 64 consecutive ones; inside a group the butterfly
 *     x_l += x_(l xor s), s = 32, 16, .. 1; the group sums added in group order.
 *  4. Tail as in sixdgs_solve_pose: final w_i at the final c, written to w_final renormalised to sum 1 (0 for padding); watch =
 *     normalised sum w_i d_i; make_rotation_mat(-watch, up[b]); singular -> I; c2w = [inv(R) | c]; NaN -> I4; errors against
 *     gt_c2w when given.
 *  5. No valid hypothesis (or n < 2): status bit 3; c = the plain unweighted least-squares centre over the valid rays (NaN when
 *     its determinant < 1e-7, bit 2), w_i = p_i front_i(c), then the tail of 4; winner = (-1, -1).
 * outputs: those of sixdgs_solve_pose (status bits 0..2 as there, bit 3 = no hypothesis; n_kept = n), and -- each may be NULL --
 *   support [B]     S at the final centre (normalised prior): a confidence in [0, 1];
 *   n_inliers [B]   rays with front_i and r_i <= 2 tau at the final centre;
 *   rms [B]         sqrt(sum w_i r_i^2 / sum w_i) with the final w_i;
 *   winner [B,2]    the winning pair's positions.
 * Workspace: the best (S, pair) of every block of 256 hypotheses, per image.  SIXDGS_E_BADARG for k < 2, k > 1024, tau <= 0 (or
 * tau^2 not a finite non-zero fp32 number), prior outside {0, 1}, batch > 65535 or ws_bytes below the query -- answered without
 * touching the GPU.  Two kernels on `stream`, no sync, capturable. */
size_t sixdgs_solve_pose_consensus_workspace_bytes(int batch, int k);
int sixdgs_solve_pose_consensus(const float* rays_ori, const float* rays_dir, int64_t r, const int64_t* idx /*[B,k]*/,
                                const float* val /*[B,k]*/, int k, const float* up /*[B,3]*/, const float* gt_c2w /*[B,4,4] or NULL*/,
                                int batch, float tau, int prior, float* c2w, int32_t* status, float* w_final, int32_t* n_kept,
                                float* centre /*[B,3]*/, float* errors, float* support, int32_t* n_inliers, float* rms,
                                int32_t* winner, void* ws, size_t ws_bytes, sixdgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIXDGS_H */
