// raster.hip -- views of a 3DGS scene by the alpha-blended tile rasteriser (include/sixdgs.h, sixdgs_raster_views).  The image
// is defined operation by operation in the header; tests/raster_reference.py restates that definition in numpy.
//
//   project  k_raster_project  one lane per (view, Gaussian): steps 1-9 of the header (cull, 2D covariance, conic, radius, centre,
//            tile rectangle, SH colour, opacity) packed into per-(view, Gaussian) records, and the number of tiles it touches
//   scan     rocPRIM exclusive scan of the tile counts (one element more than there are records: the last offset is the total)
//   emit     k_raster_emit     one lane per (view, Gaussian): its (tile << 32 | depth bits, index) pairs at its scanned offset, in
//            rectangle order.  Offsets ascend with the index, so pairs of one tile and depth appear in index order: no atomics
//   sort     rocPRIM radix sort (stable) on the used key bits only; the slots behind the total carry a key past the last tile
//   ranges   k_raster_ranges   [start, end) of every tile in the sorted keys
//   blend    k_raster_blend    one workgroup of 256 lanes per tile, one pixel per lane; rounds of 256 instances staged in LDS
//
// When the scene needs more than max_instances pairs, emit / ranges / blend read the total on the device and return; nothing is
// written past a buffer, `instances` still receives the needed number.  No kernel here uses scratch or a global atomic, and every
// pixel blends its Gaussians in one fixed order: the same input gives the same bytes.
#include <cstring>

#include "common.h"
#include "device_math.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

using namespace sdg;

typedef unsigned long long u64;

constexpr int kTile = 16;                       // part of the image's definition
constexpr int kMaxSide = 16384;
constexpr float kNearZ = 0.2f;
constexpr float kMaxRadius = 1073741824.f;      // radii saturate here (2^30): they are stored as int32
// rocPRIM's temporary storage is reserved by bound, because its own size query needs a device and *_workspace_bytes must not:
// the scan keeps a look-back state per block of >= 256 items, the sort (double-buffered: no copy of the pairs) histograms and a
// look-back state per block and digit.  Both bounds are far above what rocPRIM 3.x / 4.x ask for; the call checks them.
constexpr size_t kTmpFixed = (size_t)1 << 20;
inline size_t scan_tmp_bound(size_t items) { return sdg_align(kTmpFixed + 2 * items); }
inline size_t sort_tmp_bound(size_t items) { return sdg_align(kTmpFixed + 16 * items); }

struct Records {            // per (view, Gaussian), index view * n + i
  float4* co;               // conic.x, conic.y, conic.z, opacity
  float2* uv;               // centre
  float* rgb;               // [.][3]
  uint32_t* depth;          // bits of p.z
  ushort4* rect;            // x0, y0, x1, y1 in tiles
  int64_t* cnt;             // tiles touched; one element more, which is 0
  int64_t* offs;            // exclusive scan of cnt; offs[views * n] = the total
};

struct ProjectArgs {
  const float *xyz, *scale, *rot, *opacity, *f_dc, *f_rest, *cams;
  Records r;
  int32_t* radii;
  int64_t n;
  int scale_is_log, opacity_is_logit, sh_degree, n_coef, width, height, gx, gy;
  float scale_modifier;
};

// int(q) clamped to [0, g]: q is clamped as a float first (it may be huge or not finite), which does not change the result
__device__ __forceinline__ int tile_bound(float q, int g) {
  const int t = (int)fminf(fmaxf(q, -1.f), (float)(g + 1));
  return min(max(t, 0), g);
}

__global__ __launch_bounds__(256) void k_raster_project(ProjectArgs A) {
  const int view = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const int64_t vi = (int64_t)view * A.n + i;
  if (vi == 0) A.r.cnt[(int64_t)gridDim.y * A.n] = 0;
  const float* __restrict__ cam = A.cams + 16 * (size_t)view;

  int radius_i = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  const float X = A.xyz[3 * i], Y = A.xyz[3 * i + 1], Z = A.xyz[3 * i + 2];
  const float pz = ((cam[8] * X + cam[9] * Y) + cam[10] * Z) + cam[11];
  if (pz > kNearZ) {                      // (false for NaN too)
    const float px = ((cam[0] * X + cam[1] * Y) + cam[2] * Z) + cam[3];
    const float py = ((cam[4] * X + cam[5] * Y) + cam[6] * Z) + cam[7];
    const float fx = cam[12], fy = cam[13];
    // 3D covariance: M = R S, Sigma = M M^T
    float R[9];
    quat_to_rotmat(A.rot + 4 * i, R);
    float s[3] = {A.scale[3 * i], A.scale[3 * i + 1], A.scale[3 * i + 2]};
    float M[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sc = A.scale_modifier * (A.scale_is_log ? expf(s[c]) : s[c]);
#pragma unroll
      for (int r = 0; r < 3; ++r) M[3 * r + c] = R[3 * r + c] * sc;
    }
    float S[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[3 * r + c] = (M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1]) + M[3 * r + 2] * M[3 * c + 2];
    // 2D covariance: T = J W, cov = T Sigma T^T
    const float limx = 1.3f * ((float)A.width / (2.f * fx)), limy = 1.3f * ((float)A.height / (2.f * fy));
    const float tx = fminf(limx, fmaxf(-limx, px / pz)) * pz, ty = fminf(limy, fmaxf(-limy, py / pz)) * pz;
    const float j00 = fx / pz, j02 = -(fx * tx) / (pz * pz), j11 = fy / pz, j12 = -(fy * ty) / (pz * pz);
    float T0[3], T1[3], v0[3], v1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      T0[k] = j00 * cam[k] + j02 * cam[8 + k];
      T1[k] = j11 * cam[4 + k] + j12 * cam[8 + k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      v0[r] = (S[3 * r] * T0[0] + S[3 * r + 1] * T0[1]) + S[3 * r + 2] * T0[2];
      v1[r] = (S[3 * r] * T1[0] + S[3 * r + 1] * T1[1]) + S[3 * r + 2] * T1[2];
    }
    const float a = ((T0[0] * v0[0] + T0[1] * v0[1]) + T0[2] * v0[2]) + 0.3f;
    const float b = (T1[0] * v0[0] + T1[1] * v0[1]) + T1[2] * v0[2];
    const float c = ((T1[0] * v1[0] + T1[1] * v1[1]) + T1[2] * v1[2]) + 0.3f;
    const float det = a * c - b * b;
    if (det != 0.f) {
      const float mid = 0.5f * (a + c);
      const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
      const float radius = fminf(fmaxf(ceilf(3.f * sqrtf(lam)), 0.f), kMaxRadius);      // (0 for NaN)
      const float u = fx * px / pz + cam[14], v = fy * py / pz + cam[15];
      const float um = u - 0.5f, vm = v - 0.5f;
      x0 = tile_bound((um - radius) / 16.f, A.gx);
      x1 = tile_bound(((um + radius) + 15.f) / 16.f, A.gx);
      y0 = tile_bound((vm - radius) / 16.f, A.gy);
      y1 = tile_bound(((vm + radius) + 15.f) / 16.f, A.gy);
      if (x1 > x0 && y1 > y0) {
        radius_i = (int)radius;
        // colour: the camera centre is -W^T t; view direction = normalize(xyz - centre)
        const float t0 = cam[3], t1 = cam[7], t2 = cam[11];
        const float ccx = -((cam[0] * t0 + cam[4] * t1) + cam[8] * t2);
        const float ccy = -((cam[1] * t0 + cam[5] * t1) + cam[9] * t2);
        const float ccz = -((cam[2] * t0 + cam[6] * t1) + cam[10] * t2);
        const V3 d = normalize_eps(v3(X - ccx, Y - ccy, Z - ccz));
        float sh[48];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sh[ch] = A.f_dc[3 * i + ch];
#pragma unroll
        for (int k = 1; k < 16; ++k)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) sh[3 * k + ch] = k < A.n_coef ? A.f_rest[(i * (A.n_coef - 1) + (k - 1)) * 3 + ch] : 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) A.r.rgb[3 * vi + ch] = sh_channel(sh + ch, 3, A.sh_degree, d.x, d.y, d.z);
        const float op = A.opacity[i];
        A.r.co[vi] = make_float4(c / det, -b / det, a / det, A.opacity_is_logit ? 1.f / (1.f + expf(-op)) : op);
        A.r.uv[vi] = make_float2(u, v);
        A.r.depth[vi] = __float_as_uint(pz);
      } else {
        x0 = y0 = x1 = y1 = 0;
      }
    }
  }
  A.r.rect[vi] = make_ushort4((unsigned short)x0, (unsigned short)y0, (unsigned short)x1, (unsigned short)y1);
  A.r.cnt[vi] = (int64_t)(x1 - x0) * (y1 - y0);
  if (A.radii) A.radii[vi] = radius_i;
}

// one lane per (view, Gaussian): its pairs, rectangle row by rectangle row
__global__ __launch_bounds__(256) void k_raster_emit(Records r, int64_t n, int gx, int gy, int64_t max_instances, u64* __restrict__ keys,
                                                     uint32_t* __restrict__ vals) {
  const int view = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r.offs[(int64_t)gridDim.y * n] > max_instances || i >= n) return;
  const int64_t vi = (int64_t)view * n + i;
  const ushort4 rc = r.rect[vi];
  if (rc.x == rc.z || rc.y == rc.w) return;
  int64_t o = r.offs[vi];
  const u64 lo = r.depth[vi];
  const u64 tile0 = (u64)view * gx * gy;
  for (int y = rc.y; y < rc.w; ++y)
    for (int x = rc.x; x < rc.z; ++x, ++o) {
      keys[o] = ((tile0 + (u64)y * gx + x) << 32) | lo;
      vals[o] = (uint32_t)i;
    }
}

// the slots the scene did not fill get a key past the last tile (all of them when the scene does not fit); the needed number
__global__ __launch_bounds__(256) void k_raster_pad(const int64_t* __restrict__ total, int64_t max_instances, u64 pad_key,
                                                    u64* __restrict__ keys, uint32_t* __restrict__ vals, int64_t* __restrict__ instances) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = *total;
  if (k == 0 && instances) *instances = t;
  if (k < max_instances && (k >= t || t > max_instances)) {
    keys[k] = pad_key;
    vals[k] = 0;
  }
}

// ranges [tiles + 1] (zeroed before): where each tile's run of sorted keys starts and ends; the padding is the run of tile `tiles`
__global__ __launch_bounds__(256) void k_raster_ranges(const int64_t* __restrict__ total, int64_t max_instances, const u64* __restrict__ keys,
                                                       int2* __restrict__ ranges) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (*total > max_instances || k >= max_instances) return;
  const uint32_t t = (uint32_t)(keys[k] >> 32);
  if (k == 0) {
    ranges[t].x = 0;
  } else {
    const uint32_t p = (uint32_t)(keys[k - 1] >> 32);
    if (p != t) {
      ranges[p].y = (int)k;
      ranges[t].x = (int)k;
    }
  }
  if (k == max_instances - 1) ranges[t].y = (int)max_instances;
}

struct BlendArgs {
  Records r;
  const int64_t* total;
  const int2* ranges;
  const uint32_t* vals;
  const float* background;
  float* image_f32;
  uint8_t* image_u8;
  int64_t n, max_instances;
  int width, height, gx, gy, channels;
};

__device__ __forceinline__ uint8_t to_u8(float x) { return (uint8_t)rintf(255.f * fminf(fmaxf(x, 0.f), 1.f)); }

__global__ __launch_bounds__(256) void k_raster_blend(BlendArgs B) {
  __shared__ float4 s_co[256];
  __shared__ float2 s_uv[256];
  __shared__ float s_rgb[3 * 256];
  if (*B.total > B.max_instances) return;
  const int tid = threadIdx.x, view = blockIdx.z;
  const int2 rg = B.ranges[((int64_t)view * B.gy + blockIdx.y) * B.gx + blockIdx.x];
  const int x = blockIdx.x * kTile + (tid & 15), y = blockIdx.y * kTile + (tid >> 4);
  const bool inside = x < B.width && y < B.height;
  const float xf = (float)x, yf = (float)y;
  const int64_t rec0 = (int64_t)view * B.n;
  bool done = !inside;
  float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
  for (int base = rg.x; base < rg.y; base += 256) {
    if (__syncthreads_and(done)) break;          // (also: everybody has left the previous round's LDS)
    const int m = min(256, rg.y - base);
    if (tid < m) {
      const int64_t rec = rec0 + B.vals[base + tid];
      s_co[tid] = B.r.co[rec];
      s_uv[tid] = B.r.uv[rec];
      s_rgb[3 * tid] = B.r.rgb[3 * rec];
      s_rgb[3 * tid + 1] = B.r.rgb[3 * rec + 1];
      s_rgb[3 * tid + 2] = B.r.rgb[3 * rec + 2];
    }
    __syncthreads();
    for (int j = 0; !done && j < m; ++j) {
      const float2 uv = s_uv[j];
      const float4 co = s_co[j];
      const float dx = (uv.x - xf) - 0.5f, dy = (uv.y - yf) - 0.5f;
      const float power = -0.5f * ((co.x * dx) * dx + (co.z * dy) * dy) - (co.y * dx) * dy;
      if (power > 0.f) continue;
      const float alpha = fminf(0.99f, co.w * expf(power));
      if (alpha < 1.f / 255.f) continue;
      const float Tn = T * (1.f - alpha);
      if (Tn < 1e-4f) {
        done = true;
        break;
      }
      C0 += (s_rgb[3 * j] * alpha) * T;
      C1 += (s_rgb[3 * j + 1] * alpha) * T;
      C2 += (s_rgb[3 * j + 2] * alpha) * T;
      T = Tn;
    }
  }
  if (!inside) return;
  const float o0 = C0 + T * B.background[0], o1 = C1 + T * B.background[1], o2 = C2 + T * B.background[2], oa = 1.f - T;
  const int64_t p = ((int64_t)view * B.height + y) * B.width + x;
  if (B.image_f32) reinterpret_cast<float4*>(B.image_f32)[p] = make_float4(o0, o1, o2, oa);
  if (B.image_u8) {
    if (B.channels == 4) {
      reinterpret_cast<uchar4*>(B.image_u8)[p] = make_uchar4(to_u8(o0), to_u8(o1), to_u8(o2), to_u8(oa));
    } else {
      uint8_t* o = B.image_u8 + 3 * p;
      o[0] = to_u8(o0); o[1] = to_u8(o1); o[2] = to_u8(o2);
    }
  }
}

struct Layout {
  size_t co, uv, rgb, depth, rect, cnt, offs, ranges, keys0, keys1, vals0, vals1, scan_tmp, sort_tmp, total;
  size_t scan_tmp_bytes, sort_tmp_bytes;
};

bool sizes_ok(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (n < 0 || n >= ((int64_t)1 << 31) || views < 0 || views > 65535) return false;
  if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return false;
  if (max_instances < 1 || max_instances >= ((int64_t)1 << 31)) return false;
  const int64_t tiles = (int64_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile);
  return tiles < ((int64_t)1 << 31);
}

Layout layout(int64_t n, int views, int width, int height, int64_t max_instances) {
  const size_t vn = (size_t)views * (size_t)n, m = (size_t)max_instances;
  const size_t tiles = (size_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile);
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += sdg_align(bytes); return at; };
  L.co = take(vn * sizeof(float4));
  L.uv = take(vn * sizeof(float2));
  L.rgb = take(vn * 3 * sizeof(float));
  L.depth = take(vn * sizeof(uint32_t));
  L.rect = take(vn * sizeof(ushort4));
  L.cnt = take((vn + 1) * sizeof(int64_t));
  L.offs = take((vn + 1) * sizeof(int64_t));
  L.ranges = take((tiles + 1) * sizeof(int2));
  L.keys0 = take(m * sizeof(u64));
  L.keys1 = take(m * sizeof(u64));
  L.vals0 = take(m * sizeof(uint32_t));
  L.vals1 = take(m * sizeof(uint32_t));
  L.scan_tmp_bytes = scan_tmp_bound(vn + 1);
  L.sort_tmp_bytes = sort_tmp_bound(m);
  L.scan_tmp = take(L.scan_tmp_bytes);
  L.sort_tmp = take(L.sort_tmp_bytes);
  L.total = o;
  return L;
}

}  // namespace

extern "C" {

size_t sixdgs_raster_views_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (!sizes_ok(n, views, width, height, max_instances)) return 0;
  return layout(n, views, width, height, max_instances).total;
}

int sixdgs_raster_views(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity,
                        int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n,
                        const float* cams, int views, int width, int height, float scale_modifier, const float* background,
                        float* image_f32, uint8_t* image_u8, int channels, int32_t* radii, int64_t max_instances, int64_t* instances,
                        void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof) {
  SDG_CHECK_ARG(sizes_ok(n, views, width, height, max_instances));
  SDG_CHECK_ARG(channels == 3 || channels == 4);
  SDG_CHECK_ARG(scale_modifier > 0.f && scale_modifier < INFINITY);
  SDG_CHECK_ARG(sh_degree >= 0 && sh_degree <= 3 && n_coef >= (sh_degree + 1) * (sh_degree + 1) && n_coef <= 16);
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && background);
  SDG_CHECK_ARG(n == 0 || (xyz && scale && rot && opacity && f_dc && (n_coef == 1 || f_rest)));
  const Layout L = layout(n, views, width, height, max_instances);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const int64_t vn = (int64_t)views * n, tiles = (int64_t)views * gx * gy;
  Records r = {(float4*)(w + L.co), (float2*)(w + L.uv), (float*)(w + L.rgb), (uint32_t*)(w + L.depth), (ushort4*)(w + L.rect),
               (int64_t*)(w + L.cnt), (int64_t*)(w + L.offs)};
  int2* ranges = (int2*)(w + L.ranges);
  const uint32_t* vals = (uint32_t*)(w + L.vals0);
  hipError_t e = hipMemsetAsync(ranges, 0, (size_t)(tiles + 1) * sizeof(int2), s);
  if (e != hipSuccess) return (int)e;
  if (n == 0) {           // the background everywhere; r.offs[0] is the total the blend kernel reads
    e = hipMemsetAsync(r.offs, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    if (instances) {
      e = hipMemsetAsync(instances, 0, sizeof(int64_t), s);
      if (e != hipSuccess) return (int)e;
    }
  } else {
    const dim3 per_gaussian((unsigned)sdg_cdiv(n, 256), (unsigned)views);
    const unsigned per_instance = (unsigned)sdg_cdiv(max_instances, 256);
    {
      SdgProfileScope t(prof, s, 0, 0);
      ProjectArgs A = {xyz, scale, rot, opacity, f_dc, f_rest, cams, r, radii, n, scale_is_log, opacity_is_logit, sh_degree, n_coef,
                       width, height, gx, gy, scale_modifier};
      hipLaunchKernelGGL(k_raster_project, per_gaussian, dim3(256), 0, s, A);
      SDG_LAUNCH_OK();
    }
    {
      SdgProfileScope t(prof, s, 0, 0);
      size_t need = 0;
      e = rocprim::exclusive_scan((void*)nullptr, need, r.cnt, r.offs, (int64_t)0, (size_t)(vn + 1), rocprim::plus<int64_t>(), s);
      if (e != hipSuccess) return (int)e;
      if (need > L.scan_tmp_bytes) return SIXDGS_E_WORKSPACE;
      need = L.scan_tmp_bytes;
      e = rocprim::exclusive_scan((void*)(w + L.scan_tmp), need, r.cnt, r.offs, (int64_t)0, (size_t)(vn + 1), rocprim::plus<int64_t>(), s);
      if (e != hipSuccess) return (int)e;
    }
    rocprim::double_buffer<u64> keys((u64*)(w + L.keys0), (u64*)(w + L.keys1));
    rocprim::double_buffer<uint32_t> idx((uint32_t*)(w + L.vals0), (uint32_t*)(w + L.vals1));
    {
      SdgProfileScope t(prof, s, 0, 0);
      hipLaunchKernelGGL(k_raster_emit, per_gaussian, dim3(256), 0, s, r, n, gx, gy, max_instances, keys.current(), idx.current());
      SDG_LAUNCH_OK();
      hipLaunchKernelGGL(k_raster_pad, dim3(per_instance), dim3(256), 0, s, r.offs + vn, max_instances, (u64)tiles << 32, keys.current(),
                         idx.current(), instances);
      SDG_LAUNCH_OK();
    }
    {
      SdgProfileScope t(prof, s, 0, 0);
      int tile_bits = 0;
      while (tile_bits < 32 && ((int64_t)1 << tile_bits) <= tiles) ++tile_bits;      // the padding's tile id is `tiles` itself
      size_t need = 0;
      e = rocprim::radix_sort_pairs((void*)nullptr, need, keys, idx, (size_t)max_instances, 0u, (unsigned)(32 + tile_bits), s);
      if (e != hipSuccess) return (int)e;
      if (need > L.sort_tmp_bytes) return SIXDGS_E_WORKSPACE;
      need = L.sort_tmp_bytes;
      e = rocprim::radix_sort_pairs((void*)(w + L.sort_tmp), need, keys, idx, (size_t)max_instances, 0u, (unsigned)(32 + tile_bits), s);
      if (e != hipSuccess) return (int)e;
    }
    {
      SdgProfileScope t(prof, s, 0, 0);
      hipLaunchKernelGGL(k_raster_ranges, dim3(per_instance), dim3(256), 0, s, r.offs + vn, max_instances, keys.current(), ranges);
      SDG_LAUNCH_OK();
    }
    vals = idx.current();
  }
  if (image_f32 || image_u8) {
    SdgProfileScope t(prof, s, 0, 0);
    BlendArgs B = {r, r.offs + vn, ranges, vals, background, image_f32, image_u8, n, max_instances, width, height, gx, gy, channels};
    hipLaunchKernelGGL(k_raster_blend, dim3((unsigned)gx, (unsigned)gy, (unsigned)views), dim3(256), 0, s, B);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
