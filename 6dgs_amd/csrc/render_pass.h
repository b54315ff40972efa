// render_pass.h -- the host side of one render-and-compare pass, shared by raster.hip, refine.hip, fit.hip and metrics.hip: the scene and the
// target as the entry points receive them, with their checks; the workspace every fused loop starts with; and the three calls of a
// pass -- rasteriser, photometric loss, rasteriser's backward -- through their own entry points.  Internal: not part of the C ABI.
#pragma once
#include <math.h>

#include "common.h"

namespace rp {

constexpr int kMaxViews = 65535;

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool hyper_ok(float beta1, float beta2, float eps) {
  return beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && eps < INFINITY;
}
inline bool loop_ok(float lambda, int steps) { return lambda >= 0.f && lambda <= 1.f && steps >= 1 && steps < INT32_MAX - 1; }

struct Scene {
  const float *xyz, *scale, *rot, *opacity, *f_dc, *f_rest, *background;
  int scale_is_log, opacity_is_logit, n_coef;
  int64_t n;
  float scale_modifier;
};
struct Target {
  const void* data;      // fp32 [views,height,width,stride] or, with is_u8, bytes [views,height,width,3]
  int is_u8, stride;
};

struct Image {
  const float* data;     // fp32 [views,height,width,stride]: a render (stride 4, the fourth channel never read) or three plain channels
  int stride;
};

// the numbers, for a render at sh_degree: asked before an entry point's `no views, nothing to do` ...
inline bool scene_ok(const Scene& S, int sh_degree) {
  return S.scale_modifier > 0.f && S.scale_modifier < INFINITY && sh_degree >= 0 && sh_degree <= 3 &&
         S.n_coef >= (sh_degree + 1) * (sh_degree + 1) && S.n_coef <= 16;
}
inline bool target_ok(const Target& T) { return T.is_u8 == 1 ? T.stride == 3 : (T.is_u8 == 0 && (T.stride == 3 || T.stride == 4)); }
// ... and the pointers: asked behind it
inline bool scene_present(const Scene& S) {
  return S.background && (S.n == 0 || (S.xyz && S.scale && S.rot && S.opacity && S.f_dc && (S.n_coef == 1 || S.f_rest)));
}
inline bool target_present(const Target& T) { return T.data && (T.is_u8 || aligned4(T.data)); }
// the measured image and the input rule of the held-out-view metrics, in the same two halves
inline bool image_ok(const Image& I) { return I.stride == 3 || I.stride == 4; }
inline bool quantise_ok(int quantise) { return quantise == 0 || quantise == 1; }
inline bool image_present(const Image& I) { return I.data && aligned4(I.data); }

// What every loop's workspace starts with: the three entry points' own workspaces, the image, its gradient, the camera rows of the
// views drawn, their losses and the instance count.  A loop's Layout derives from it and goes on with take().
struct PassLayout : SdgBump {
  size_t fwd, bwd, photo, image, grad, rows, loss, count;
  size_t fwd_bytes, bwd_bytes, photo_bytes;
};

// L comes in zeroed; false (and total still 0) = outside the limits (the rasteriser's: its workspace is never 0 inside them)
inline bool pass_layout(PassLayout& L, int64_t n, int views, int width, int height, int64_t max_instances) {
  L.fwd_bytes = sixdgs_raster_views_workspace_bytes(n, views, width, height, max_instances);
  L.bwd_bytes = sixdgs_raster_views_backward_workspace_bytes(n, views, width, height, max_instances);
  L.photo_bytes = sixdgs_photometric_loss_workspace_bytes(views, width, height, 1);
  if (L.fwd_bytes == 0 || L.bwd_bytes == 0 || (views > 0 && L.photo_bytes == 0)) return false;
  const size_t image_bytes = (size_t)views * (size_t)height * (size_t)width * 4 * sizeof(float);
  L.fwd = L.take(L.fwd_bytes);
  L.bwd = L.take(L.bwd_bytes);
  L.photo = L.take(L.photo_bytes);
  L.image = L.take(image_bytes);
  L.grad = L.take(image_bytes);
  L.rows = L.take((size_t)views * 16 * sizeof(float));
  L.loss = L.take((size_t)views * sizeof(float));
  L.count = L.take(sizeof(int64_t));
  return true;
}

// One pass over `views` camera rows in the workspace w laid out by L: the image, its loss per view against T and -- with grad, which
// is NULL or w + L.grad -- the loss's gradient, then the rasteriser's backward into the seven d_ outputs; all NULL: no backward.
// radii (may be NULL): the forward's radii [views][n], for the densification statistics.
inline int render_pass(const Scene& S, int sh_degree, const float* rows, int views, int width, int height, const Target& T, float lambda,
                       int64_t max_instances, const PassLayout& L, char* w, float* grad, float* d_xyz, float* d_scale, float* d_rot,
                       float* d_opacity, float* d_f_dc, float* d_f_rest, float* d_rows, sixdgs_stream_t stream,
                       int32_t* radii = nullptr) {
  float* image = (float*)(w + L.image);
  int st = sixdgs_raster_views(S.xyz, S.scale, S.scale_is_log, S.rot, S.opacity, S.opacity_is_logit, S.f_dc, S.f_rest, sh_degree, S.n_coef, S.n,
                               rows, views, width, height, S.scale_modifier, S.background, image, nullptr, 3, radii, max_instances,
                               (int64_t*)(w + L.count), w + L.fwd, L.fwd_bytes, stream, nullptr);
  if (st != 0) return st;
  st = sixdgs_photometric_loss(image, 4, T.data, T.is_u8, T.stride, views, width, height, lambda, nullptr, (float*)(w + L.loss), nullptr, grad,
                               w + L.photo, L.photo_bytes, stream, nullptr);
  if (st != 0 || !(d_xyz || d_scale || d_rot || d_opacity || d_f_dc || d_f_rest || d_rows)) return st;
  return sixdgs_raster_views_backward(S.xyz, S.scale, S.scale_is_log, S.rot, S.opacity, S.opacity_is_logit, S.f_dc, S.f_rest, sh_degree, S.n_coef,
                                      S.n, rows, views, width, height, S.scale_modifier, S.background, grad, max_instances, w + L.fwd,
                                      L.fwd_bytes, d_xyz, d_scale, d_rot, d_opacity, d_f_dc, d_f_rest, d_rows, w + L.bwd, L.bwd_bytes, stream,
                                      nullptr);
}

}  // namespace rp
