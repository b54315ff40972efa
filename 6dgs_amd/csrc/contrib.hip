// contrib.hip -- every Gaussian's contribution to many views as one call (include/sixdgs.h, sixdgs_scene_contrib): chunks of views, each
// projected, sorted and ranged by sixdgs_raster_views without an image -- its blend does not run -- and walked by sixdgs_raster_contrib
// into the caller's accumulators, through the entry points as they are.  No host synchronisation, no read-back, no allocation.
#include "render_pass.h"

namespace {

using namespace rp;

// Behind a chunk: the largest count, and bit 1 when the rasteriser's capacity did not hold it (the contribution kernels read the same
// count and have left the accumulators as they were)
__global__ __launch_bounds__(64) void k_contrib_record(const int64_t* __restrict__ count, int64_t max_instances, int32_t* __restrict__ status,
                                                       int64_t* __restrict__ instances_needed) {
  if (threadIdx.x != 0) return;
  const int64_t cnt = *count;
  if (cnt > *instances_needed) *instances_needed = cnt;
  if (cnt > max_instances) *status |= 2;
}

struct ContribLayout : SdgBump {
  size_t fwd, walk, count;
  size_t fwd_bytes, walk_bytes;
};

// 0 total = outside the limits
ContribLayout contrib_layout(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  ContribLayout L = {};
  if (chunk < 1) return L;
  L.fwd_bytes = sixdgs_raster_views_workspace_bytes(n, chunk, width, height, max_instances);
  L.walk_bytes = sixdgs_raster_contrib_workspace_bytes(n, chunk, width, height, max_instances);
  if (L.fwd_bytes == 0 || L.walk_bytes == 0) return L;
  L.fwd = L.take(L.fwd_bytes);
  L.walk = L.take(L.walk_bytes);
  L.count = L.take(sizeof(int64_t));
  return L;
}

}  // namespace

extern "C" {

size_t sixdgs_scene_contrib_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  return contrib_layout(n, chunk, width, height, max_instances).total;
}

int sixdgs_scene_contrib(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                         const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams, int views, int width,
                         int height, float scale_modifier, int chunk, int64_t max_instances, float* weight, float* peak, int64_t* pixels,
                         int64_t* stops, int32_t* seen, float* view_weight, int32_t* view_pixels, int32_t* status, int64_t* instances_needed,
                         void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const ContribLayout L = contrib_layout(n, chunk, width, height, max_instances);
  // no image is formed, so no background enters; the rasteriser's check wants the pointer, and the camera rows are one it never writes
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, cams, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  SDG_CHECK_ARG(L.total != 0 && views >= 0 && views <= kMaxViews);
  SDG_CHECK_ARG(scene_ok(S, sh_degree));
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && scene_present(S));
  SDG_CHECK_ARG(status && instances_needed);
  SDG_CHECK_ARG(aligned4(cams) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  SDG_CHECK_ARG(aligned4(weight) && aligned4(peak) && ((uintptr_t)pixels & 7) == 0 && ((uintptr_t)stops & 7) == 0 && aligned4(seen) &&
                aligned4(view_weight) && aligned4(view_pixels));
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  int64_t* count = (int64_t*)(w + L.count);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(instances_needed, 0, sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  if (n == 0) return 0;
  for (int v0 = 0; v0 < views; v0 += chunk) {
    const int nv = views - v0 < chunk ? views - v0 : chunk;
    int st = sixdgs_raster_views(S.xyz, S.scale, S.scale_is_log, S.rot, S.opacity, S.opacity_is_logit, S.f_dc, S.f_rest, sh_degree, S.n_coef, S.n,
                                 cams + 16 * (size_t)v0, nv, width, height, S.scale_modifier, S.background, nullptr, nullptr, 3, nullptr,
                                 max_instances, count, w + L.fwd, L.fwd_bytes, stream, nullptr);
    if (st != 0) return st;
    st = sixdgs_raster_contrib(n, nv, width, height, max_instances, w + L.fwd, L.fwd_bytes, weight, peak, pixels, stops, seen,
                               view_weight ? view_weight + (size_t)v0 * (size_t)n : nullptr,
                               view_pixels ? view_pixels + (size_t)v0 * (size_t)n : nullptr, w + L.walk, L.walk_bytes, stream, nullptr);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_contrib_record, dim3(1), dim3(64), 0, s, (const int64_t*)count, max_instances, status, instances_needed);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
