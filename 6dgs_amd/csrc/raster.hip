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
// The backward (sixdgs_raster_views_backward: k_raster_blend_bwd, k_raster_project_bwd, k_raster_cams_bwd) is further down; it reads this
// workspace and sorts nothing again.  So does the contribution pass behind it (sixdgs_raster_contrib: k_raster_contrib_walk,
// k_raster_contrib_gather), which repeats the blend's walk and keeps alpha T per (view, Gaussian) instead of a colour, and the depth pass
// behind that (sixdgs_raster_depth: k_raster_depth), which repeats it with the Gaussians' p.z as the colour and notes where T crosses 0.5.
//
// When the scene needs more than max_instances pairs, emit / ranges / blend read the total on the device and return; nothing is
// written past a buffer, `instances` still receives the needed number.  No kernel here uses scratch or a global atomic, and every
// pixel blends its Gaussians in one fixed order: the same input gives the same bytes.
#include <cstring>

#include "device_math.h"
#include "pose_step.h"
#include "render_pass.h"

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

struct Layout : SdgBump {
  size_t co, uv, rgb, depth, rect, cnt, offs, ranges, keys0, keys1, vals0, vals1, scan_tmp, sort_tmp;
  size_t scan_tmp_bytes, sort_tmp_bytes;
};

bool sizes_ok(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (n < 0 || n >= ((int64_t)1 << 31) || views < 0 || views > rp::kMaxViews) return false;
  if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return false;
  if (max_instances < 1 || max_instances >= ((int64_t)1 << 31)) return false;
  const int64_t tiles = (int64_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile);
  return tiles < ((int64_t)1 << 31);
}

Layout layout(int64_t n, int views, int width, int height, int64_t max_instances) {
  const size_t vn = (size_t)views * (size_t)n, m = (size_t)max_instances;
  const size_t tiles = (size_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile);
  Layout L = {};
  L.co = L.take(vn * sizeof(float4));
  L.uv = L.take(vn * sizeof(float2));
  L.rgb = L.take(vn * 3 * sizeof(float));
  L.depth = L.take(vn * sizeof(uint32_t));
  L.rect = L.take(vn * sizeof(ushort4));
  L.cnt = L.take((vn + 1) * sizeof(int64_t));
  L.offs = L.take((vn + 1) * sizeof(int64_t));
  L.ranges = L.take((tiles + 1) * sizeof(int2));
  L.keys0 = L.take(m * sizeof(u64));
  L.keys1 = L.take(m * sizeof(u64));
  L.vals0 = L.take(m * sizeof(uint32_t));
  L.vals1 = L.take(m * sizeof(uint32_t));
  L.scan_tmp_bytes = scan_tmp_bound(vn + 1);
  L.sort_tmp_bytes = sort_tmp_bound(m);
  L.scan_tmp = L.take(L.scan_tmp_bytes);
  L.sort_tmp = L.take(L.sort_tmp_bytes);
  return L;
}

// ---- backward (include/sixdgs.h, sixdgs_raster_views_backward) ---------------------------------------------------------------------
//   blend_bwd    k_raster_blend_bwd    one workgroup per tile, one pixel per lane.  Phase A repeats the forward walk (final T, where
//                the pixel stopped); phase B walks the tile's list back to front in rounds of 256 and reduces, per instance, the 9
//                sums over the tile's pixels in a fixed tree (lanes by xor 32 .. 1, then waves 0 .. 3) into the instance's OWN slot
//                offs[vi] + (ty - y0)(x1 - x0) + (tx - x0): every slot is written exactly once, no memset, no atomic
//   project_bwd  k_raster_project_bwd  one lane per Gaussian, views in ascending order: sums its slots in order, chains steps 9 .. 1 to
//                the parameters and adds to register accumulators; the 16 camera terms are block-reduced to [view][block][16]
//   cams         k_raster_cams_bwd     adds the block partials in block order
constexpr int kSlot = 9;        // per instance: d u, d v, d conic.x, d conic.y, d conic.z, d o, d rgb[3]

struct BlendBwdArgs {
  Records r;
  const int64_t* total;
  const int2* ranges;
  const uint32_t *vals0, *vals1;
  const uint32_t* which;        // != 0: vals1 holds the sorted indices (written by the forward after its sort)
  const float* background;
  const float* grad;
  float* slots;
  int64_t n, max_instances;
  int width, height, gx, gy;
};

__global__ __launch_bounds__(256) void k_raster_blend_bwd(BlendBwdArgs B) {
  __shared__ float4 s_co[256];
  __shared__ float2 s_uv[256];
  __shared__ float s_rgb[3 * 256];
  __shared__ float s_part[256 * 4 * kSlot];
  __shared__ uint32_t s_has[256];              // byte w of entry j: wave w has a sum for instance j
  __shared__ int s_hi[4];
  if (*B.total > B.max_instances) return;
  const int tid = threadIdx.x, view = blockIdx.z, wave = tid >> 6, lane = tid & 63;
  const int2 rg = B.ranges[((int64_t)view * B.gy + blockIdx.y) * B.gx + blockIdx.x];
  if (rg.y <= rg.x) return;
  const uint32_t* __restrict__ vals = *B.which ? B.vals1 : B.vals0;
  const int x = blockIdx.x * kTile + (tid & 15), y = blockIdx.y * kTile + (tid >> 4);
  const bool inside = x < B.width && y < B.height;
  const float xf = (float)x, yf = (float)y;
  const int64_t rec0 = (int64_t)view * B.n;
  // phase A: the forward's walk, operation by operation; `end` = the list position at which this pixel stopped
  bool done = !inside;
  float T = 1.f;
  int end = inside ? rg.y : rg.x;
  for (int base = rg.x; base < rg.y; base += 256) {
    if (__syncthreads_and(done)) break;
    const int m = min(256, rg.y - base);
    if (tid < m) {
      const int64_t rec = rec0 + vals[base + tid];
      s_co[tid] = B.r.co[rec];
      s_uv[tid] = B.r.uv[rec];
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
        end = base + j;
        break;
      }
      T = Tn;
    }
  }
  int hi = end;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
  if (lane == 0) s_hi[wave] = hi;
  __syncthreads();
  hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
  // phase B: back to front.  channel 3 is 1 - T: colour 1, background 0
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (inside) g = reinterpret_cast<const float4*>(B.grad)[((int64_t)view * B.height + y) * B.width + x];
  float R0 = T * B.background[0], R1 = T * B.background[1], R2 = T * B.background[2], R3 = 0.f;
  for (int base = rg.x + ((rg.y - rg.x - 1) / 256) * 256; base >= rg.x; base -= 256) {
    const int m = min(256, rg.y - base);
    int64_t slot = -1, rec = 0;
    if (tid < m) {
      rec = rec0 + vals[base + tid];
      const ushort4 rc = B.r.rect[rec];
      slot = B.r.offs[rec] + (int64_t)((int)blockIdx.y - (int)rc.y) * ((int)rc.z - (int)rc.x) + ((int)blockIdx.x - (int)rc.x);
      if (slot < 0 || slot >= B.max_instances) slot = -1;          // (cannot happen with the workspace of a completed forward)
    }
    float* __restrict__ out = B.slots + (size_t)(slot < 0 ? 0 : slot) * kSlot;
    if (base >= hi) {             // no pixel got this far: zeros
      if (slot >= 0)
#pragma unroll
        for (int k = 0; k < kSlot; ++k) out[k] = 0.f;
      continue;
    }
    __syncthreads();              // everybody has left the previous round's LDS
    if (tid < m) {
      s_co[tid] = B.r.co[rec];
      s_uv[tid] = B.r.uv[rec];
      s_rgb[3 * tid] = B.r.rgb[3 * rec];
      s_rgb[3 * tid + 1] = B.r.rgb[3 * rec + 1];
      s_rgb[3 * tid + 2] = B.r.rgb[3 * rec + 2];
    }
    s_has[tid] = 0;
    __syncthreads();
    for (int j = min(m, hi - base) - 1; j >= 0; --j) {
      float d[kSlot];
#pragma unroll
      for (int k = 0; k < kSlot; ++k) d[k] = 0.f;
      bool on = false;
      if (base + j < end) {
        const float2 uv = s_uv[j];
        const float4 co = s_co[j];
        const float dx = (uv.x - xf) - 0.5f, dy = (uv.y - yf) - 0.5f;
        const float power = -0.5f * ((co.x * dx) * dx + (co.z * dy) * dy) - (co.y * dx) * dy;
        if (!(power > 0.f)) {
          const float G = expf(power);
          const float araw = co.w * G;
          const float alpha = fminf(0.99f, araw);
          if (!(alpha < 1.f / 255.f)) {
            on = true;
            const float c0 = s_rgb[3 * j], c1 = s_rgb[3 * j + 1], c2 = s_rgb[3 * j + 2];
            const float om = 1.f - alpha;
            const float Tj = T / om;
            const float dalpha = ((g.x * (c0 * Tj - R0 / om) + g.y * (c1 * Tj - R1 / om)) + g.z * (c2 * Tj - R2 / om)) + g.w * (Tj - R3 / om);
            const float w = alpha * Tj;
            d[6] = g.x * w;
            d[7] = g.y * w;
            d[8] = g.z * w;
            R0 += c0 * w;
            R1 += c1 * w;
            R2 += c2 * w;
            R3 += w;
            T = Tj;
            if (araw < 0.99f) {       // the clamp does not act
              const float dp = dalpha * alpha;
              d[0] = dp * (-(co.x * dx) - co.y * dy);
              d[1] = dp * (-(co.z * dy) - co.y * dx);
              d[2] = (-0.5f * dp) * (dx * dx);
              d[3] = -dp * (dx * dy);
              d[4] = (-0.5f * dp) * (dy * dy);
              d[5] = dalpha * G;
            }
          }
        }
      }
      if (__ballot(on) != 0) {      // (uniform in the wave)
#pragma unroll
        for (int k = 0; k < kSlot; ++k) d[k] = sdg_wave_sum(d[k]);
        if (lane == 0) {
          float* __restrict__ p = s_part + (j * 4 + wave) * kSlot;
#pragma unroll
          for (int k = 0; k < kSlot; ++k) p[k] = d[k];
          reinterpret_cast<uint8_t*>(s_has)[j * 4 + wave] = 1;
        }
      }
    }
    __syncthreads();
    if (slot >= 0) {
      const uint32_t has = s_has[tid];
      float acc[kSlot];
#pragma unroll
      for (int k = 0; k < kSlot; ++k) acc[k] = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if ((has >> (8 * w)) & 0xffu) {
          const float* __restrict__ p = s_part + (tid * 4 + w) * kSlot;
#pragma unroll
          for (int k = 0; k < kSlot; ++k) acc[k] += p[k];
        }
#pragma unroll
      for (int k = 0; k < kSlot; ++k) out[k] = acc[k];
    }
  }
}

// the 16 basis values of sh_channel (its constants and signs) at (x, y, z) and their derivatives by x, y and z
__device__ __forceinline__ void sh_basis_grad(float x, float y, float z, float* b, float* bx, float* by, float* bz) {
  const float C1 = 0.4886025119029199f, C2 = 1.0925484305920792f, C6 = 0.31539156525252005f, C8 = 0.5462742152960396f;
  const float C9 = 0.5900435899266435f, C10 = 2.890611442640554f, C11 = 0.4570457994644658f, C12 = 0.3731763325901154f, C14 = 1.445305721320277f;
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  b[0] = 0.28209479177387814f; bx[0] = 0.f; by[0] = 0.f; bz[0] = 0.f;
  b[1] = -C1 * y; bx[1] = 0.f; by[1] = -C1; bz[1] = 0.f;
  b[2] = C1 * z; bx[2] = 0.f; by[2] = 0.f; bz[2] = C1;
  b[3] = -C1 * x; bx[3] = -C1; by[3] = 0.f; bz[3] = 0.f;
  b[4] = C2 * xy; bx[4] = C2 * y; by[4] = C2 * x; bz[4] = 0.f;
  b[5] = -C2 * yz; bx[5] = 0.f; by[5] = -C2 * z; bz[5] = -C2 * y;
  b[6] = C6 * ((2.f * zz - xx) - yy); bx[6] = -2.f * C6 * x; by[6] = -2.f * C6 * y; bz[6] = 4.f * C6 * z;
  b[7] = -C2 * xz; bx[7] = -C2 * z; by[7] = 0.f; bz[7] = -C2 * x;
  b[8] = C8 * (xx - yy); bx[8] = 2.f * C8 * x; by[8] = -2.f * C8 * y; bz[8] = 0.f;
  b[9] = (-C9 * y) * (3.f * xx - yy); bx[9] = -6.f * C9 * xy; by[9] = -C9 * (3.f * xx - 3.f * yy); bz[9] = 0.f;
  b[10] = (C10 * xy) * z; bx[10] = C10 * yz; by[10] = C10 * xz; bz[10] = C10 * xy;
  b[11] = (-C11 * y) * ((4.f * zz - xx) - yy); bx[11] = 2.f * C11 * xy; by[11] = -C11 * ((4.f * zz - xx) - 3.f * yy); bz[11] = -8.f * C11 * yz;
  b[12] = (C12 * z) * ((2.f * zz - 3.f * xx) - 3.f * yy); bx[12] = -6.f * C12 * xz; by[12] = -6.f * C12 * yz; bz[12] = C12 * ((6.f * zz - 3.f * xx) - 3.f * yy);
  b[13] = (-C11 * x) * ((4.f * zz - xx) - yy); bx[13] = -C11 * ((4.f * zz - 3.f * xx) - yy); by[13] = 2.f * C11 * xy; bz[13] = -8.f * C11 * xz;
  b[14] = (C14 * z) * (xx - yy); bx[14] = 2.f * C14 * xz; by[14] = -2.f * C14 * yz; bz[14] = C14 * (xx - yy);
  b[15] = (-C9 * x) * (xx - 3.f * yy); bx[15] = -C9 * (3.f * xx - 3.f * yy); by[15] = 6.f * C9 * xy; bz[15] = 0.f;
}

struct ProjectBwdArgs {
  const float *xyz, *scale, *rot, *opacity, *f_dc, *f_rest, *cams;
  Records r;
  const float* slots;
  float *d_xyz, *d_scale, *d_rot, *d_opacity, *d_f_dc, *d_f_rest, *cam_part;
  int64_t n, max_instances;
  int views, scale_is_log, opacity_is_logit, sh_degree, n_coef, width, height;
  float scale_modifier;
};

__global__ __launch_bounds__(256) void k_raster_project_bwd(ProjectBwdArgs A) {
  __shared__ float s_cam[4 * 16];
  if (A.r.offs[(int64_t)A.views * A.n] > A.max_instances) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool mine = i < A.n;
  const int nb = (A.sh_degree + 1) * (A.sh_degree + 1);
  float X = 0.f, Y = 0.f, Z = 0.f, q[4] = {1.f, 0.f, 0.f, 0.f}, s[3] = {0.f, 0.f, 0.f}, op = 0.f;
  if (mine) {
    X = A.xyz[3 * i]; Y = A.xyz[3 * i + 1]; Z = A.xyz[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = A.rot[4 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = A.scale[3 * i + k];
    op = A.opacity[i];
  }
  float a_xyz[3] = {0.f, 0.f, 0.f}, a_scale[3] = {0.f, 0.f, 0.f}, a_rot[4] = {0.f, 0.f, 0.f, 0.f}, a_op = 0.f, a_sh[48];
#pragma unroll
  for (int k = 0; k < 48; ++k) a_sh[k] = 0.f;
  for (int view = 0; view < A.views; ++view) {
    const float* __restrict__ cam = A.cams + 16 * (size_t)view;
    const int64_t vi = (int64_t)view * A.n + i;
    const int64_t cnt = mine ? A.r.cnt[vi] : 0;
    float dcam[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) dcam[k] = 0.f;
    if (cnt > 0) {
      // the instance sums of this (view, Gaussian), in slot order
      float in[kSlot];
#pragma unroll
      for (int k = 0; k < kSlot; ++k) in[k] = 0.f;
      const float* __restrict__ sl = A.slots + (size_t)A.r.offs[vi] * kSlot;
      for (int64_t t = 0; t < cnt; ++t)
#pragma unroll
        for (int k = 0; k < kSlot; ++k) in[k] += sl[t * kSlot + k];
      const float du = in[0], dv = in[1], dA = in[2], dB = in[3], dC = in[4];
      // ---- steps 1 - 6 again, as k_raster_project does them
      const float pz = ((cam[8] * X + cam[9] * Y) + cam[10] * Z) + cam[11];
      const float px = ((cam[0] * X + cam[1] * Y) + cam[2] * Z) + cam[3];
      const float py = ((cam[4] * X + cam[5] * Y) + cam[6] * Z) + cam[7];
      const float fx = cam[12], fy = cam[13];
      const float n0 = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      const float d0 = fmaxf(n0, 1e-12f);
      const float q1[4] = {q[0] / d0, q[1] / d0, q[2] / d0, q[3] / d0};
      const float n1 = sqrtf(q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2] + q1[3] * q1[3]);
      const float qr = q1[0] / n1, qx = q1[1] / n1, qy = q1[2] / n1, qz = q1[3] / n1;
      float R[9];
      R[0] = 1.f - 2.f * (qy * qy + qz * qz);
      R[1] = 2.f * (qx * qy - qr * qz);
      R[2] = 2.f * (qx * qz + qr * qy);
      R[3] = 2.f * (qx * qy + qr * qz);
      R[4] = 1.f - 2.f * (qx * qx + qz * qz);
      R[5] = 2.f * (qy * qz - qr * qx);
      R[6] = 2.f * (qx * qz - qr * qy);
      R[7] = 2.f * (qy * qz + qr * qx);
      R[8] = 1.f - 2.f * (qx * qx + qy * qy);
      float sc[3], M[9], S[9];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sc[c] = A.scale_modifier * (A.scale_is_log ? expf(s[c]) : s[c]);
#pragma unroll
        for (int r = 0; r < 3; ++r) M[3 * r + c] = R[3 * r + c] * sc[c];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) S[3 * r + c] = (M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1]) + M[3 * r + 2] * M[3 * c + 2];
      const float limx = 1.3f * ((float)A.width / (2.f * fx)), limy = 1.3f * ((float)A.height / (2.f * fy));
      const float rx = px / pz, ry = py / pz;
      const float clx = fminf(limx, fmaxf(-limx, rx)), cly = fminf(limy, fmaxf(-limy, ry));
      const float tx = clx * pz, ty = cly * pz;
      const float pz2 = pz * pz;
      const float j00 = fx / pz, j02 = -(fx * tx) / pz2, j11 = fy / pz, j12 = -(fy * ty) / pz2;
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
      // ---- step 4: conic = (c, -b, a) / det
      const float inv = 1.f / det;
      const float ddet = -(((dA * c - dB * b) + dC * a) * inv) * inv;
      const float da = dC * inv + ddet * c, dc = dA * inv + ddet * a, db = -(dB * inv) - (2.f * b) * ddet;
      // ---- step 3: a = T0' S T0, b = T1' S T0, c = T1' S T1
      float dT0[3], dT1[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dT0[k] = (2.f * da) * v0[k] + db * v1[k];
        dT1[k] = (2.f * dc) * v1[k] + db * v0[k];
      }
      // ---- step 2: S = M M', dM = (dS + dS') M
      float Gs[9], dM[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          Gs[3 * r + k] = ((2.f * da) * (T0[r] * T0[k]) + db * (T1[r] * T0[k] + T0[r] * T1[k])) + (2.f * dc) * (T1[r] * T1[k]);
      float dsc[3], dR[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) dM[3 * r + k] = (Gs[3 * r] * M[k] + Gs[3 * r + 1] * M[3 + k]) + Gs[3 * r + 2] * M[6 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dsc[k] = (dM[k] * R[k] + dM[3 + k] * R[3 + k]) + dM[6 + k] * R[6 + k];
#pragma unroll
        for (int r = 0; r < 3; ++r) dR[3 * r + k] = dM[3 * r + k] * sc[k];
      }
      float l_scale[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) l_scale[k] = A.scale_is_log ? dsc[k] * sc[k] : dsc[k] * A.scale_modifier;
      // rotation matrix -> unit quaternion -> both normalisations
      float dq2[4];
      dq2[0] = 2.f * (((qz * (dR[3] - dR[1]) + qy * (dR[2] - dR[6])) + qx * (dR[7] - dR[5])));
      dq2[1] = 2.f * ((((qy * (dR[1] + dR[3]) + qz * (dR[2] + dR[6])) + qr * (dR[7] - dR[5])) - 2.f * qx * (dR[4] + dR[8])));
      dq2[2] = 2.f * ((((qx * (dR[1] + dR[3]) + qz * (dR[5] + dR[7])) + qr * (dR[2] - dR[6])) - 2.f * qy * (dR[0] + dR[8])));
      dq2[3] = 2.f * ((((qx * (dR[2] + dR[6]) + qy * (dR[5] + dR[7])) + qr * (dR[3] - dR[1])) - 2.f * qz * (dR[0] + dR[4])));
      const float q2[4] = {qr, qx, qy, qz};
      const float dot2 = ((q2[0] * dq2[0] + q2[1] * dq2[1]) + q2[2] * dq2[2]) + q2[3] * dq2[3];
      float dq1[4], l_rot[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) dq1[k] = (dq2[k] - q2[k] * dot2) / n1;
      const float dot1 = ((q1[0] * dq1[0] + q1[1] * dq1[1]) + q1[2] * dq1[2]) + q1[3] * dq1[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) l_rot[k] = n0 > 1e-12f ? (dq1[k] - q1[k] * dot1) / d0 : dq1[k] / d0;
      // ---- J: T0 = j00 W0 + j02 W2, T1 = j11 W1 + j12 W2
      const float dj00 = (dT0[0] * cam[0] + dT0[1] * cam[1]) + dT0[2] * cam[2];
      const float dj02 = (dT0[0] * cam[8] + dT0[1] * cam[9]) + dT0[2] * cam[10];
      const float dj11 = (dT1[0] * cam[4] + dT1[1] * cam[5]) + dT1[2] * cam[6];
      const float dj12 = (dT1[0] * cam[8] + dT1[1] * cam[9]) + dT1[2] * cam[10];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dcam[k] = dT0[k] * j00;
        dcam[4 + k] = dT1[k] * j11;
        dcam[8 + k] = dT0[k] * j02 + dT1[k] * j12;
      }
      const float dtx = -(dj02 * fx) / pz2, dty = -(dj12 * fy) / pz2;
      float dfx = (dj00 / pz - (dj02 * tx) / pz2) + (du * px) / pz;
      float dfy = (dj11 / pz - (dj12 * ty) / pz2) + (dv * py) / pz;
      float dpx = (du * fx) / pz, dpy = (dv * fy) / pz;
      float dpz = ((-(dj00 * j00) - (dj11 * j11)) - 2.f * (dj02 * j02 + dj12 * j12)) / pz - ((du * fx) * px + (dv * fy) * py) / pz2;
      // tx = clamp(p.x / p.z) p.z: inside the clamp it is p.x, at the clamp +-limx p.z
      if (rx > limx || rx < -limx) {
        const float sg = rx > 0.f ? 1.f : -1.f;
        dpz += dtx * clx;
        dfx -= ((sg * dtx) * pz) * (limx / fx);
      } else {
        dpx += dtx;
      }
      if (ry > limy || ry < -limy) {
        const float sg = ry > 0.f ? 1.f : -1.f;
        dpz += dty * cly;
        dfy -= ((sg * dty) * pz) * (limy / fy);
      } else {
        dpy += dty;
      }
      dcam[12] = dfx;
      dcam[13] = dfy;
      dcam[14] = du;
      dcam[15] = dv;
      // ---- step 8: colour towards the camera centre -W' t
      const float t0 = cam[3], t1 = cam[7], t2 = cam[11];
      const float ccx = -((cam[0] * t0 + cam[4] * t1) + cam[8] * t2);
      const float ccy = -((cam[1] * t0 + cam[5] * t1) + cam[9] * t2);
      const float ccz = -((cam[2] * t0 + cam[6] * t1) + cam[10] * t2);
      const float wx = X - ccx, wy = Y - ccy, wz = Z - ccz;
      const float nw = sqrtf((wx * wx + wy * wy) + wz * wz);
      const float dn = fmaxf(nw, 1e-12f);
      const float ex = wx / dn, ey = wy / dn, ez = wz / dn;
      float drgb[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) drgb[ch] = A.r.rgb[3 * vi + ch] > 0.f ? in[6 + ch] : 0.f;        // max(. + 0.5, 0)
      float bs[16], bx[16], by[16], bz[16];
      sh_basis_grad(ex, ey, ez, bs, bx, by, bz);
      float dex = 0.f, dey = 0.f, dez = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < nb) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float coef = k == 0 ? A.f_dc[3 * i + ch] : A.f_rest[(i * (A.n_coef - 1) + (k - 1)) * 3 + ch];
            a_sh[3 * k + ch] += drgb[ch] * bs[k];
            const float dcf = drgb[ch] * coef;
            dex += dcf * bx[k];
            dey += dcf * by[k];
            dez += dcf * bz[k];
          }
        }
      float dwx, dwy, dwz;
      if (nw > 1e-12f) {
        const float pr = (ex * dex + ey * dey) + ez * dez;
        dwx = (dex - ex * pr) / dn;
        dwy = (dey - ey * pr) / dn;
        dwz = (dez - ez * pr) / dn;
      } else {
        dwx = dex / dn;
        dwy = dey / dn;
        dwz = dez / dn;
      }
      // centre_k = -sum_r W[r][k] t[r]; d centre = -d w
      dcam[0] += dwx * t0; dcam[1] += dwy * t0; dcam[2] += dwz * t0;
      dcam[4] += dwx * t1; dcam[5] += dwy * t1; dcam[6] += dwz * t1;
      dcam[8] += dwx * t2; dcam[9] += dwy * t2; dcam[10] += dwz * t2;
      const float dt0 = (dwx * cam[0] + dwy * cam[1]) + dwz * cam[2];
      const float dt1 = (dwx * cam[4] + dwy * cam[5]) + dwz * cam[6];
      const float dt2 = (dwx * cam[8] + dwy * cam[9]) + dwz * cam[10];
      // ---- step 1: p = W xyz + t
      dcam[0] += dpx * X; dcam[1] += dpx * Y; dcam[2] += dpx * Z; dcam[3] = dpx + dt0;
      dcam[4] += dpy * X; dcam[5] += dpy * Y; dcam[6] += dpy * Z; dcam[7] = dpy + dt1;
      dcam[8] += dpz * X; dcam[9] += dpz * Y; dcam[10] += dpz * Z; dcam[11] = dpz + dt2;
      a_xyz[0] += ((dpx * cam[0] + dpy * cam[4]) + dpz * cam[8]) + dwx;
      a_xyz[1] += ((dpx * cam[1] + dpy * cam[5]) + dpz * cam[9]) + dwy;
      a_xyz[2] += ((dpx * cam[2] + dpy * cam[6]) + dpz * cam[10]) + dwz;
#pragma unroll
      for (int k = 0; k < 3; ++k) a_scale[k] += l_scale[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) a_rot[k] += l_rot[k];
      // ---- step 9
      if (A.opacity_is_logit) {       // o' = e / (1 + e)^2, e = exp(-opacity): o (1 - o) would cancel for o near 1
        const float e = expf(-op), d1 = 1.f + e;
        a_op += in[5] * (e / (d1 * d1));
      } else {
        a_op += in[5];
      }
    }
    if (A.cam_part) {             // the fixed tree over the block: lanes by xor 32 .. 1, then waves 0 .. 3
#pragma unroll
      for (int k = 0; k < 16; ++k) dcam[k] = sdg_wave_sum(dcam[k]);
      if (lane == 0)
#pragma unroll
        for (int k = 0; k < 16; ++k) s_cam[16 * wave + k] = dcam[k];
      __syncthreads();
      if (tid < 16) A.cam_part[((size_t)view * gridDim.x + blockIdx.x) * 16 + tid] = ((s_cam[tid] + s_cam[16 + tid]) + s_cam[32 + tid]) + s_cam[48 + tid];
      __syncthreads();
    }
  }
  if (!mine) return;
  if (A.d_xyz)
#pragma unroll
    for (int k = 0; k < 3; ++k) A.d_xyz[3 * i + k] = a_xyz[k];
  if (A.d_scale)
#pragma unroll
    for (int k = 0; k < 3; ++k) A.d_scale[3 * i + k] = a_scale[k];
  if (A.d_rot)
#pragma unroll
    for (int k = 0; k < 4; ++k) A.d_rot[4 * i + k] = a_rot[k];
  if (A.d_opacity) A.d_opacity[i] = a_op;
  if (A.d_f_dc)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) A.d_f_dc[3 * i + ch] = a_sh[ch];
  if (A.d_f_rest)
#pragma unroll
    for (int k = 1; k < 16; ++k)
      if (k < A.n_coef)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) A.d_f_rest[(i * (A.n_coef - 1) + (k - 1)) * 3 + ch] = a_sh[3 * k + ch];
}

// d_cams[view][16] = the block partials added in block order: one workgroup per view stages 256 blocks' partials at a time in LDS
// (coalesced), lanes 0 .. 15 add them one after the other
__global__ __launch_bounds__(256) void k_raster_cams_bwd(const int64_t* __restrict__ total, int64_t max_instances, const float* __restrict__ part,
                                                         int blocks, float* __restrict__ d_cams) {
  __shared__ float s_part[256 * 16];
  if (*total > max_instances) return;
  const int view = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ p = part + (size_t)view * blocks * 16;
  float acc = 0.f;
  for (int b0 = 0; b0 < blocks; b0 += 256) {
    const int m = min(256, blocks - b0);
    __syncthreads();
    for (int e = tid; e < m * 16; e += 256) s_part[e] = p[(size_t)b0 * 16 + e];
    __syncthreads();
    if (tid < 16)
      for (int b = 0; b < m; ++b) acc += s_part[b * 16 + tid];
  }
  if (tid < 16) d_cams[view * 16 + tid] = acc;
}

// ---- densification statistics (include/sixdgs.h, sixdgs_densify_stats) -------------------------------------------------------------
// One lane per Gaussian, views in ascending order: d u, d v of a visible (view, Gaussian) are the sums of its slots' entries 0 and 1
// in slot order from 0.f -- the bits k_raster_project_bwd chained -- and the three statistics are updated in registers.  Reads both
// workspaces, writes neither.
struct StatsArgs {
  const int64_t *cnt, *offs;
  const float* slots;
  const int32_t* radii;
  float* grad_accum;
  int32_t *denom, *max_radii;
  float* grad2d;
  const int32_t* status;
  int64_t n, max_instances;
  int views;
  float half_w, half_h;
};

__global__ __launch_bounds__(256) void k_densify_stats(StatsArgs A) {
  if (A.offs[(int64_t)A.views * A.n] > A.max_instances) return;
  if (A.status && (*A.status & ps::kStatusCapacity)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  float acc = A.grad_accum[i];
  int32_t den = A.denom[i], rad = A.max_radii[i];
  for (int view = 0; view < A.views; ++view) {
    const int64_t vi = (int64_t)view * A.n + i;
    const int64_t cnt = A.cnt[vi];
    float du = 0.f, dv = 0.f;
    if (cnt > 0) {
      const float* __restrict__ sl = A.slots + (size_t)A.offs[vi] * kSlot;
      for (int64_t t = 0; t < cnt; ++t) {
        du += sl[t * kSlot];
        dv += sl[t * kSlot + 1];
      }
      const float a = A.half_w * du, b = A.half_h * dv;
      acc += sqrtf(a * a + b * b);
      den += 1;
      rad = max(rad, A.radii[vi]);
    }
    if (A.grad2d) {
      A.grad2d[2 * vi] = du;
      A.grad2d[2 * vi + 1] = dv;
    }
  }
  A.grad_accum[i] = acc;
  A.denom[i] = den;
  A.max_radii[i] = rad;
}

struct BwdLayout : SdgBump {
  size_t slots, cam_part;
};

BwdLayout bwd_layout(int64_t n, int views, int64_t max_instances) {
  BwdLayout L = {};
  L.slots = L.take((size_t)max_instances * kSlot * sizeof(float));
  L.cam_part = L.take((size_t)views * (size_t)sdg_cdiv(n, 256) * 16 * sizeof(float));
  return L;
}

// ---- contributions (include/sixdgs.h, sixdgs_raster_contrib) -----------------------------------------------------------------------
//   walk    k_raster_contrib_walk    one workgroup per tile and view, one pixel per lane: the forward's walk, operation by operation, in
//           rounds of 256 staged in LDS.  All lanes stay in step per list entry; a lane that skipped or has stopped counts 0.f / 0.  Where
//           the wave's ballot says some lane added or stopped, the wave reduces w = alpha T (sum and max by xor 32 .. 1) and counts the
//           two ballots; lane 0 leaves the partial in LDS.  After the round thread tid adds waves 0 .. 3 in order into instance tid's OWN
//           slot offs[vi] + (ty - y0)(x1 - x0) + (tx - x0): every slot is written exactly once, no memset, no atomic
//   gather  k_raster_contrib_gather  one lane per Gaussian, views in ascending order, slots in order; accumulators in registers, one
//           read-modify-write per output
// Reads the forward's workspace, writes only its own slots and the outputs.
struct ContribWalkArgs {
  Records r;
  const int64_t* total;
  const int2* ranges;
  const uint32_t *vals0, *vals1;
  const uint32_t* which;
  uint4* slots;                 // per instance: bits of the sum of w, bits of the largest w, pixels that added, pixels it stopped
  int64_t n, max_instances;
  int width, height, gx, gy;
};

__global__ __launch_bounds__(256) void k_raster_contrib_walk(ContribWalkArgs B) {
  __shared__ float4 s_co[256];
  __shared__ float2 s_uv[256];
  __shared__ uint4 s_part[256 * 4];            // [entry j][wave]
  if (*B.total > B.max_instances) return;
  const int tid = threadIdx.x, view = blockIdx.z, wave = tid >> 6, lane = tid & 63;
  const int2 rg = B.ranges[((int64_t)view * B.gy + blockIdx.y) * B.gx + blockIdx.x];
  if (rg.y <= rg.x) return;
  const uint32_t* __restrict__ vals = *B.which ? B.vals1 : B.vals0;
  const int x = blockIdx.x * kTile + (tid & 15), y = blockIdx.y * kTile + (tid >> 4);
  const bool inside = x < B.width && y < B.height;
  const float xf = (float)x, yf = (float)y;
  const int64_t rec0 = (int64_t)view * B.n;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);          // (0.f, 0.f, 0, 0)
  bool done = !inside;
  float T = 1.f;
  for (int base = rg.x; base < rg.y; base += 256) {
    const bool over = __syncthreads_and(done);            // (also: everybody has left the previous round's LDS)
    const int m = min(256, rg.y - base);
    int64_t slot = -1, rec = 0;
    if (tid < m) {
      rec = rec0 + vals[base + tid];
      const ushort4 rc = B.r.rect[rec];
      slot = B.r.offs[rec] + (int64_t)((int)blockIdx.y - (int)rc.y) * ((int)rc.z - (int)rc.x) + ((int)blockIdx.x - (int)rc.x);
      if (slot < 0 || slot >= B.max_instances) slot = -1;          // (cannot happen with the workspace of a completed forward)
    }
    if (over) {                   // every pixel has stopped: zeros
      if (slot >= 0) B.slots[slot] = zero;
      continue;
    }
    if (tid < m) {
      s_co[tid] = B.r.co[rec];
      s_uv[tid] = B.r.uv[rec];
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) s_part[tid * 4 + w] = zero;
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      if (__ballot(!done) == 0) break;          // (uniform in the wave) its partials of the rest stay zero
      float w = 0.f;
      bool add = false, stop = false;
      if (!done) {
        const float2 uv = s_uv[j];
        const float4 co = s_co[j];
        const float dx = (uv.x - xf) - 0.5f, dy = (uv.y - yf) - 0.5f;
        const float power = -0.5f * ((co.x * dx) * dx + (co.z * dy) * dy) - (co.y * dx) * dy;
        if (!(power > 0.f)) {
          const float alpha = fminf(0.99f, co.w * expf(power));
          if (!(alpha < 1.f / 255.f)) {
            const float Tn = T * (1.f - alpha);
            if (Tn < 1e-4f) {
              done = true;
              stop = true;
            } else {
              w = alpha * T;
              add = true;
              T = Tn;
            }
          }
        }
      }
      const u64 adds = __ballot(add), stops = __ballot(stop);
      if ((adds | stops) != 0) {      // (uniform in the wave)
        const float sum = sdg_wave_sum(w), peak = sdg_wave_max(w);
        if (lane == 0) s_part[j * 4 + wave] = make_uint4(__float_as_uint(sum), __float_as_uint(peak), (uint32_t)__popcll(adds), (uint32_t)__popcll(stops));
      }
    }
    __syncthreads();
    if (slot >= 0) {
      const uint4 p0 = s_part[tid * 4], p1 = s_part[tid * 4 + 1], p2 = s_part[tid * 4 + 2], p3 = s_part[tid * 4 + 3];
      const float sum = ((__uint_as_float(p0.x) + __uint_as_float(p1.x)) + __uint_as_float(p2.x)) + __uint_as_float(p3.x);
      const float peak = fmaxf(fmaxf(__uint_as_float(p0.y), __uint_as_float(p1.y)), fmaxf(__uint_as_float(p2.y), __uint_as_float(p3.y)));
      B.slots[slot] = make_uint4(__float_as_uint(sum), __float_as_uint(peak), ((p0.z + p1.z) + p2.z) + p3.z, ((p0.w + p1.w) + p2.w) + p3.w);
    }
  }
}

struct ContribGatherArgs {
  const int64_t *cnt, *offs;
  const uint4* slots;
  float *weight, *peak;
  int64_t *pixels, *stops;
  int32_t* seen;
  float* view_weight;
  int32_t* view_pixels;
  int64_t n, max_instances;
  int views;
};

__global__ __launch_bounds__(256) void k_raster_contrib_gather(ContribGatherArgs A) {
  if (A.offs[(int64_t)A.views * A.n] > A.max_instances) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  float weight = A.weight ? A.weight[i] : 0.f, peak = A.peak ? A.peak[i] : 0.f;
  int64_t pixels = A.pixels ? A.pixels[i] : 0, stops = A.stops ? A.stops[i] : 0;
  int32_t seen = A.seen ? A.seen[i] : 0;
  for (int view = 0; view < A.views; ++view) {
    const int64_t vi = (int64_t)view * A.n + i;
    const int64_t cnt = A.cnt[vi];
    float w = 0.f, pk = 0.f;
    int32_t px = 0, st = 0;
    if (cnt > 0) {
      const uint4* __restrict__ sl = A.slots + A.offs[vi];
      for (int64_t t = 0; t < cnt; ++t) {
        const uint4 s = sl[t];
        w += __uint_as_float(s.x);
        pk = fmaxf(pk, __uint_as_float(s.y));
        px += (int32_t)s.z;
        st += (int32_t)s.w;
      }
    }
    weight += w;
    peak = fmaxf(peak, pk);
    pixels += px;
    stops += st;
    seen += px > 0;
    if (A.view_weight) A.view_weight[vi] = w;
    if (A.view_pixels) A.view_pixels[vi] = px;
  }
  if (A.weight) A.weight[i] = weight;
  if (A.peak) A.peak[i] = peak;
  if (A.pixels) A.pixels[i] = pixels;
  if (A.stops) A.stops[i] = stops;
  if (A.seen) A.seen[i] = seen;
}

inline size_t contrib_bytes(int64_t max_instances) { return sdg_align((size_t)max_instances * sizeof(uint4)); }

// ---- depth maps (include/sixdgs.h, sixdgs_raster_depth) ----------------------------------------------------------------------------
//   walk    k_raster_depth    one workgroup per tile and view, one pixel per lane: the blend's walk, its arithmetic as k_raster_blend
//           writes it, with one accumulator -- the depth channel D += (z alpha) T -- in the place of the three colours, and the first
//           Gaussian behind which T is below 0.5.  Rounds of 256 staged in LDS: conic + opacity, centre, z and the Gaussian's index (8 KB);
//           every lane reads the same entry (a broadcast).  Each pixel owns its elements of the outputs: no atomics, no scratch
// Reads the forward's workspace, writes only the outputs.
struct DepthArgs {
  Records r;
  const int64_t* total;
  const int2* ranges;
  const uint32_t *vals0, *vals1;
  const uint32_t* which;
  const float* cams;
  float *expected, *median;
  int32_t* median_index;
  float *alpha, *points;
  int64_t n, max_instances;
  int width, height, gx, gy, points_kind;
};

__global__ __launch_bounds__(256) void k_raster_depth(DepthArgs B) {
  __shared__ float4 s_co[256];
  __shared__ float2 s_uv[256];
  __shared__ float s_z[256];
  __shared__ uint32_t s_id[256];
  if (*B.total > B.max_instances) return;
  const int tid = threadIdx.x, view = blockIdx.z;
  const int2 rg = B.ranges[((int64_t)view * B.gy + blockIdx.y) * B.gx + blockIdx.x];
  const uint32_t* __restrict__ vals = *B.which ? B.vals1 : B.vals0;
  const int x = blockIdx.x * kTile + (tid & 15), y = blockIdx.y * kTile + (tid >> 4);
  const bool inside = x < B.width && y < B.height;
  const float xf = (float)x, yf = (float)y;
  const int64_t rec0 = (int64_t)view * B.n;
  bool done = !inside;
  float T = 1.f, D = 0.f, med = 0.f;
  int med_i = -1;
  for (int base = rg.x; base < rg.y; base += 256) {
    if (__syncthreads_and(done)) break;          // (also: everybody has left the previous round's LDS)
    const int m = min(256, rg.y - base);
    if (tid < m) {
      const uint32_t i = vals[base + tid];
      const int64_t rec = rec0 + i;
      s_co[tid] = B.r.co[rec];
      s_uv[tid] = B.r.uv[rec];
      s_z[tid] = __uint_as_float(B.r.depth[rec]);
      s_id[tid] = i;
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
      D += (s_z[j] * alpha) * T;
      if (med_i < 0 && Tn < 0.5f) {
        med = s_z[j];
        med_i = (int)s_id[j];
      }
      T = Tn;
    }
  }
  if (!inside) return;
  const float oa = 1.f - T;
  const int64_t p = ((int64_t)view * B.height + y) * B.width + x;
  if (B.expected) B.expected[p] = D;
  if (B.median) B.median[p] = med;
  if (B.median_index) B.median_index[p] = med_i;
  if (B.alpha) B.alpha[p] = oa;
  if (B.points) {
    float X = 0.f, Y = 0.f, Z = 0.f;
    if (B.points_kind == 0 ? med_i >= 0 : oa > 0.f) {
      const float* __restrict__ cam = B.cams + 16 * (size_t)view;
      const float d = B.points_kind == 0 ? med : D / oa;
      // the point of the pixel's ray at camera depth d: q = d r - t, X = W^T q
      const float qx = d * (((xf + 0.5f) - cam[14]) / cam[12]) - cam[3];
      const float qy = d * (((yf + 0.5f) - cam[15]) / cam[13]) - cam[7];
      const float qz = d - cam[11];
      X = (cam[0] * qx + cam[4] * qy) + cam[8] * qz;
      Y = (cam[1] * qx + cam[5] * qy) + cam[9] * qz;
      Z = (cam[2] * qx + cam[6] * qy) + cam[10] * qz;
    }
    float* o = B.points + 3 * p;
    o[0] = X; o[1] = Y; o[2] = Z;
  }
}

constexpr size_t kDepthBytes = 256;          // the walk needs no workspace of its own: the siblings' smallest piece

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
  const rp::Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  SDG_CHECK_ARG(channels == 3 || channels == 4);
  SDG_CHECK_ARG(rp::scene_ok(S, sh_degree));
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && rp::scene_present(S));
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
    // for the backward: which index buffer holds the sorted order (the scan's temporary storage is free by now)
    e = hipMemsetAsync(w + L.scan_tmp, vals == (const uint32_t*)(w + L.vals1) ? 1 : 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
  }
  if (image_f32 || image_u8) {
    SdgProfileScope t(prof, s, 0, 0);
    BlendArgs B = {r, r.offs + vn, ranges, vals, background, image_f32, image_u8, n, max_instances, width, height, gx, gy, channels};
    hipLaunchKernelGGL(k_raster_blend, dim3((unsigned)gx, (unsigned)gy, (unsigned)views), dim3(256), 0, s, B);
    SDG_LAUNCH_OK();
  }
  return 0;
}

size_t sixdgs_raster_views_backward_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (!sizes_ok(n, views, width, height, max_instances)) return 0;
  return bwd_layout(n, views, max_instances).total;
}

int sixdgs_raster_views_backward(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity,
                                 int opacity_is_logit, const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n,
                                 const float* cams, int views, int width, int height, float scale_modifier, const float* background,
                                 const float* grad_image, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes, float* d_xyz,
                                 float* d_scale, float* d_rot, float* d_opacity, float* d_f_dc, float* d_f_rest, float* d_cams, void* ws,
                                 size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof) {
  const rp::Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  SDG_CHECK_ARG(sizes_ok(n, views, width, height, max_instances));
  SDG_CHECK_ARG(rp::scene_ok(S, sh_degree));
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && rp::scene_present(S) && grad_image && fwd_ws);
  const Layout F = layout(n, views, width, height, max_instances);
  const BwdLayout L = bwd_layout(n, views, max_instances);
  if (fwd_ws_bytes < F.total || ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ((uintptr_t)fwd_ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  if (n == 0) {
    if (d_cams) {
      hipError_t e = hipMemsetAsync(d_cams, 0, (size_t)views * 16 * sizeof(float), s);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  if (!(d_xyz || d_scale || d_rot || d_opacity || d_f_dc || d_f_rest || d_cams)) return 0;
  char* f = (char*)const_cast<void*>(fwd_ws);
  char* w = (char*)ws;
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const int64_t vn = (int64_t)views * n;
  const int blocks = (int)sdg_cdiv(n, 256);
  Records r = {(float4*)(f + F.co), (float2*)(f + F.uv), (float*)(f + F.rgb), (uint32_t*)(f + F.depth), (ushort4*)(f + F.rect),
               (int64_t*)(f + F.cnt), (int64_t*)(f + F.offs)};
  float* slots = (float*)(w + L.slots);
  float* cam_part = d_cams ? (float*)(w + L.cam_part) : nullptr;
  {
    SdgProfileScope t(prof, s, 0, 0);
    BlendBwdArgs B = {r, r.offs + vn, (const int2*)(f + F.ranges), (const uint32_t*)(f + F.vals0), (const uint32_t*)(f + F.vals1),
                      (const uint32_t*)(f + F.scan_tmp), background, grad_image, slots, n, max_instances, width, height, gx, gy};
    hipLaunchKernelGGL(k_raster_blend_bwd, dim3((unsigned)gx, (unsigned)gy, (unsigned)views), dim3(256), 0, s, B);
    SDG_LAUNCH_OK();
  }
  {
    SdgProfileScope t(prof, s, 0, 0);
    ProjectBwdArgs A = {xyz, scale, rot, opacity, f_dc, f_rest, cams, r, slots, d_xyz, d_scale, d_rot, d_opacity, d_f_dc, d_f_rest, cam_part,
                        n, max_instances, views, scale_is_log, opacity_is_logit, sh_degree, n_coef, width, height, scale_modifier};
    hipLaunchKernelGGL(k_raster_project_bwd, dim3((unsigned)blocks), dim3(256), 0, s, A);
    SDG_LAUNCH_OK();
  }
  if (d_cams) {
    SdgProfileScope t(prof, s, 0, 0);
    hipLaunchKernelGGL(k_raster_cams_bwd, dim3((unsigned)views), dim3(256), 0, s, r.offs + vn, max_instances, cam_part, blocks, d_cams);
    SDG_LAUNCH_OK();
  }
  return 0;
}

int sixdgs_densify_stats(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                         const void* bwd_ws, size_t bwd_ws_bytes, const int32_t* radii, float* grad_accum, int32_t* denom, int32_t* max_radii,
                         float* grad2d, const int32_t* status, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(sizes_ok(n, views, width, height, max_instances));
  if (views == 0 || n == 0) return 0;
  SDG_CHECK_ARG(fwd_ws && bwd_ws && radii && grad_accum && denom && max_radii);
  SDG_CHECK_ARG(rp::aligned4(radii) && rp::aligned4(grad_accum) && rp::aligned4(denom) && rp::aligned4(max_radii) && rp::aligned4(grad2d) &&
                rp::aligned4(status));
  const Layout F = layout(n, views, width, height, max_instances);
  const BwdLayout L = bwd_layout(n, views, max_instances);
  if (fwd_ws_bytes < F.total || bwd_ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(((uintptr_t)fwd_ws & 255) == 0 && ((uintptr_t)bwd_ws & 255) == 0);
  const char* f = (const char*)fwd_ws;
  StatsArgs A = {(const int64_t*)(f + F.cnt), (const int64_t*)(f + F.offs), (const float*)((const char*)bwd_ws + L.slots), radii, grad_accum,
                 denom, max_radii, grad2d, status, n, max_instances, views, 0.5f * (float)width, 0.5f * (float)height};
  hipLaunchKernelGGL(k_densify_stats, dim3((unsigned)sdg_cdiv(n, 256)), dim3(256), 0, sdg_stream(stream), A);
  SDG_LAUNCH_OK();
  return 0;
}

size_t sixdgs_raster_contrib_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (!sizes_ok(n, views, width, height, max_instances)) return 0;
  return contrib_bytes(max_instances);
}

int sixdgs_raster_contrib(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                          float* weight, float* peak, int64_t* pixels, int64_t* stops, int32_t* seen, float* view_weight,
                          int32_t* view_pixels, void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof) {
  SDG_CHECK_ARG(sizes_ok(n, views, width, height, max_instances));
  if (views == 0 || n == 0) return 0;
  SDG_CHECK_ARG(fwd_ws);
  SDG_CHECK_ARG(rp::aligned4(weight) && rp::aligned4(peak) && ((uintptr_t)pixels & 7) == 0 && ((uintptr_t)stops & 7) == 0 && rp::aligned4(seen) &&
                rp::aligned4(view_weight) && rp::aligned4(view_pixels));
  const Layout F = layout(n, views, width, height, max_instances);
  if (fwd_ws_bytes < F.total || ws_bytes < contrib_bytes(max_instances)) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ((uintptr_t)fwd_ws & 255) == 0);
  if (!(weight || peak || pixels || stops || seen || view_weight || view_pixels)) return 0;
  hipStream_t s = sdg_stream(stream);
  const char* f = (const char*)fwd_ws;
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const int64_t vn = (int64_t)views * n;
  Records r = {(float4*)(f + F.co), (float2*)(f + F.uv), (float*)(f + F.rgb), (uint32_t*)(f + F.depth), (ushort4*)(f + F.rect),
               (int64_t*)(f + F.cnt), (int64_t*)(f + F.offs)};
  uint4* slots = (uint4*)ws;
  {
    SdgProfileScope t(prof, s, 0, 0);
    ContribWalkArgs B = {r, r.offs + vn, (const int2*)(f + F.ranges), (const uint32_t*)(f + F.vals0), (const uint32_t*)(f + F.vals1),
                         (const uint32_t*)(f + F.scan_tmp), slots, n, max_instances, width, height, gx, gy};
    hipLaunchKernelGGL(k_raster_contrib_walk, dim3((unsigned)gx, (unsigned)gy, (unsigned)views), dim3(256), 0, s, B);
    SDG_LAUNCH_OK();
  }
  {
    SdgProfileScope t(prof, s, 0, 0);
    ContribGatherArgs A = {r.cnt, r.offs, slots, weight, peak, pixels, stops, seen, view_weight, view_pixels, n, max_instances, views};
    hipLaunchKernelGGL(k_raster_contrib_gather, dim3((unsigned)sdg_cdiv(n, 256)), dim3(256), 0, s, A);
    SDG_LAUNCH_OK();
  }
  return 0;
}

size_t sixdgs_raster_depth_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances) {
  if (!sizes_ok(n, views, width, height, max_instances)) return 0;
  return kDepthBytes;
}

int sixdgs_raster_depth(int64_t n, int views, int width, int height, int64_t max_instances, const void* fwd_ws, size_t fwd_ws_bytes,
                        const float* cams, float* expected, float* median, int32_t* median_index, float* alpha, float* points,
                        int points_kind, void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof) {
  SDG_CHECK_ARG(sizes_ok(n, views, width, height, max_instances));
  SDG_CHECK_ARG(points_kind == 0 || points_kind == 1);
  if (views == 0) return 0;
  SDG_CHECK_ARG(fwd_ws && (cams || !points));
  SDG_CHECK_ARG(rp::aligned4(cams) && rp::aligned4(expected) && rp::aligned4(median) && rp::aligned4(median_index) && rp::aligned4(alpha) &&
                rp::aligned4(points));
  const Layout F = layout(n, views, width, height, max_instances);
  if (fwd_ws_bytes < F.total || ws_bytes < kDepthBytes) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ((uintptr_t)fwd_ws & 255) == 0);
  if (!(expected || median || median_index || alpha || points)) return 0;
  hipStream_t s = sdg_stream(stream);
  const size_t px = (size_t)views * (size_t)height * (size_t)width;
  if (n == 0) {           // no Gaussian, no list: every pixel keeps the values it starts the walk with
    float* const zeroed[] = {expected, median, alpha};
    for (float* o : zeroed)
      if (o) {
        const hipError_t e = hipMemsetAsync(o, 0, px * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
      }
    hipError_t e = median_index ? hipMemsetAsync(median_index, 0xFF, px * sizeof(int32_t), s) : hipSuccess;
    if (e == hipSuccess && points) e = hipMemsetAsync(points, 0, px * 3 * sizeof(float), s);
    return (int)e;
  }
  const char* f = (const char*)fwd_ws;
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const int64_t vn = (int64_t)views * n;
  Records r = {(float4*)(f + F.co), (float2*)(f + F.uv), (float*)(f + F.rgb), (uint32_t*)(f + F.depth), (ushort4*)(f + F.rect),
               (int64_t*)(f + F.cnt), (int64_t*)(f + F.offs)};
  {
    SdgProfileScope t(prof, s, 0, 0);
    DepthArgs B = {r, r.offs + vn, (const int2*)(f + F.ranges), (const uint32_t*)(f + F.vals0), (const uint32_t*)(f + F.vals1),
                   (const uint32_t*)(f + F.scan_tmp), cams, expected, median, median_index, alpha, points, n, max_instances, width, height,
                   gx, gy, points_kind};
    hipLaunchKernelGGL(k_raster_depth, dim3((unsigned)gx, (unsigned)gy, (unsigned)views), dim3(256), 0, s, B);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
