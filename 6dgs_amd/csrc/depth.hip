// depth.hip -- depth maps of many views as one call (include/sixdgs.h, sixdgs_scene_depth): chunks of views, each rasterised by
// sixdgs_raster_views -- into the chunk's rows of the caller's uint8 image, or with no image: then its blend does not run -- and walked by
// sixdgs_raster_depth into the chunk's rows of the maps, through the entry points as they are.  No host synchronisation, no read-back, no
// allocation.
#include "render_pass.h"

namespace {

using namespace rp;

// Behind a chunk: the largest count, and bit 1 when the rasteriser's capacity did not hold it (the blend and the depth kernel read the
// same count and have left the chunk's rows as they were)
__global__ __launch_bounds__(64) void k_depth_record(const int64_t* __restrict__ count, int64_t max_instances, int32_t* __restrict__ status,
                                                     int64_t* __restrict__ instances_needed) {
  if (threadIdx.x != 0) return;
  const int64_t cnt = *count;
  if (cnt > *instances_needed) *instances_needed = cnt;
  if (cnt > max_instances) *status |= 2;
}

struct DepthLayout : SdgBump {
  size_t fwd, walk, count;
  size_t fwd_bytes, walk_bytes;
};

// 0 total = outside the limits
DepthLayout depth_layout(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  DepthLayout L = {};
  if (chunk < 1) return L;
  L.fwd_bytes = sixdgs_raster_views_workspace_bytes(n, chunk, width, height, max_instances);
  L.walk_bytes = sixdgs_raster_depth_workspace_bytes(n, chunk, width, height, max_instances);
  if (L.fwd_bytes == 0 || L.walk_bytes == 0) return L;
  L.fwd = L.take(L.fwd_bytes);
  L.walk = L.take(L.walk_bytes);
  L.count = L.take(sizeof(int64_t));
  return L;
}

}  // namespace

extern "C" {

size_t sixdgs_scene_depth_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  return depth_layout(n, chunk, width, height, max_instances).total;
}

int sixdgs_scene_depth(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                       const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams, int views, int width,
                       int height, float scale_modifier, const float* background, int chunk, int64_t max_instances, float* expected,
                       float* median, int32_t* median_index, float* alpha, float* points, int points_kind, uint8_t* image_u8, int channels,
                       int32_t* status, int64_t* instances_needed, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const DepthLayout L = depth_layout(n, chunk, width, height, max_instances);
  // without an image no background enters; the rasteriser's check wants the pointer, and the camera rows are one it never writes
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, image_u8 ? background : cams, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  SDG_CHECK_ARG(L.total != 0 && views >= 0 && views <= kMaxViews);
  SDG_CHECK_ARG((channels == 3 || channels == 4) && (points_kind == 0 || points_kind == 1));
  SDG_CHECK_ARG(scene_ok(S, sh_degree));
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && scene_present(S));
  SDG_CHECK_ARG(status && instances_needed);
  SDG_CHECK_ARG(aligned4(cams) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  SDG_CHECK_ARG(aligned4(expected) && aligned4(median) && aligned4(median_index) && aligned4(alpha) && aligned4(points) &&
                (channels == 3 || aligned4(image_u8)));
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  int64_t* count = (int64_t*)(w + L.count);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(instances_needed, 0, sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  const size_t px = (size_t)height * (size_t)width;
  for (int v0 = 0; v0 < views; v0 += chunk) {
    const int nv = views - v0 < chunk ? views - v0 : chunk;
    const size_t p0 = (size_t)v0 * px;
    int st = sixdgs_raster_views(S.xyz, S.scale, S.scale_is_log, S.rot, S.opacity, S.opacity_is_logit, S.f_dc, S.f_rest, sh_degree, S.n_coef, S.n,
                                 cams + 16 * (size_t)v0, nv, width, height, S.scale_modifier, S.background, nullptr,
                                 image_u8 ? image_u8 + p0 * (size_t)channels : nullptr, channels, nullptr, max_instances, count, w + L.fwd,
                                 L.fwd_bytes, stream, nullptr);
    if (st != 0) return st;
    st = sixdgs_raster_depth(n, nv, width, height, max_instances, w + L.fwd, L.fwd_bytes, cams + 16 * (size_t)v0, expected ? expected + p0 : nullptr,
                             median ? median + p0 : nullptr, median_index ? median_index + p0 : nullptr, alpha ? alpha + p0 : nullptr,
                             points ? points + 3 * p0 : nullptr, points_kind, w + L.walk, L.walk_bytes, stream, nullptr);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_depth_record, dim3(1), dim3(64), 0, s, (const int64_t*)count, max_instances, status, instances_needed);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
