// metrics.hip -- held-out-view metrics (include/sixdgs.h: sixdgs_image_metrics, sixdgs_evaluate_views): per view L1, SSIM and the squared
// error, whole and per channel, between an image and a target after the clamp of the reference's training_report or after its 8-bit
// round trip; and the loop that renders chunks of views and measures them without the host in between.
//
// k_metrics_fwd is k_photo_fwd's structure (photometric.hip: one 256-thread workgroup per 16 x 16 tile and view, the 26 x 26 halo of both
// images in LDS with a row stride of 48 floats, per channel a horizontal and a vertical pass over five moments) with the input rule
// applied while the halo is staged, no derivative maps, and five sums per tile instead of two.  The two blur passes are restated here,
// the same statements in the same order, so that photometric.hip's code objects stay as they are; the SSIM sum of a pair already in
// [0, 1] is therefore photometric_loss's bit for bit.  The value of a byte, float(u) / 255.0f, is read from a 256-entry table in LDS that
// the workgroup fills with that very quotient: an fp32 division is a dozen instructions, and the 8-bit rule would need six per halo
// element.  With quantise the L1 and squared-error sums are integers: 32 bits per tile
// (256 * 3 * 65025 < 2^26), 64 per view, one fp64 division per view.
#include <math.h>

#include "render_pass.h"

namespace {

using namespace rp;

constexpr int kTile = 16;                 // the rasteriser's tile
constexpr int kTaps = 11, kRad = 5;
constexpr int kHalo = kTile + 2 * kRad;   // 26
constexpr int kHaloStride = 48;
constexpr int kMaxDim = 16384;
constexpr int kSums = 5;                  // per tile: m, |a - b|, then (a - b)^2 of r, g, b
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;

__constant__ float c_w[kTaps] = SIXDGS_SSIM_WINDOW;

bool sizes_ok(int views, int width, int height) {
  if (views < 0 || views > kMaxViews || width < 1 || width > kMaxDim || height < 1 || height > kMaxDim) return false;
  return (int64_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile) < ((int64_t)1 << 31);
}

size_t part_bytes(int views, int width, int height) {
  return sdg_align((size_t)views * (size_t)(sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile)) * kSums * sizeof(uint32_t));
}

// the byte of a value by the 8-bit rule; NaN -> 0 (fmaxf returns its other operand)
__device__ __forceinline__ int to_byte(float x) { return (int)truncf(fminf(fmaxf(x * 255.0f + 0.5f, 0.f), 255.f)); }

// s_val[u] = float(u) / 255.0f: the 256 quotients are formed once per workgroup, one per thread, instead of six per halo element
template <bool kQ>
__device__ __forceinline__ float input_rule(float x, const float* __restrict__ s_val) {
  return kQ ? s_val[to_byte(x)] : fminf(fmaxf(x, 0.f), 1.f);
}

template <int NQ, typename Load>
__device__ __forceinline__ void blur_rows(float* __restrict__ s_h, Load load) {
  for (int e = threadIdx.x; e < kHalo * kTile; e += 256) {
    const int row = e >> 4, col = e & 15;
    float acc[NQ], v[NQ];
    load(row, col, v);
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = c_w[0] * v[q];
#pragma unroll
    for (int k = 1; k < kTaps; ++k) {
      load(row, col + k, v);
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = acc[q] + c_w[k] * v[q];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) s_h[q * (kHalo * kTile) + e] = acc[q];
  }
}

template <int NQ>
__device__ __forceinline__ void blur_cols(const float* __restrict__ s_h, int ty, int tx, float* out) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float* __restrict__ p = s_h + q * (kHalo * kTile) + ty * kTile + tx;
    float acc = c_w[0] * p[0];
#pragma unroll
    for (int k = 1; k < kTaps; ++k) acc = acc + c_w[k] * p[k * kTile];
    out[q] = acc;
  }
}

struct FwdArgs {
  const float* image;
  const void* target;
  uint32_t* part;       // [views][gy * gx][5]: the tile's sums, floats' bits or -- with quantise, slots 1 .. 4 -- integers
  uint8_t* render;      // [views][height][width][3] or NULL
  int width, height, image_stride, target_stride;
};

template <bool kU8, bool kQ>
__global__ __launch_bounds__(256) void k_metrics_fwd(FwdArgs A) {
  __shared__ float s_a[3 * kHalo * kHaloStride], s_b[3 * kHalo * kHaloStride];
  __shared__ float s_h[5 * kHalo * kTile];
  __shared__ uint32_t s_sum[4 * kSums];
  __shared__ float s_val[256];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, view = blockIdx.z;
  if (kU8 || kQ) {
    s_val[tid] = (float)tid / 255.0f;
    __syncthreads();
  }
  const int x0 = blockIdx.x * kTile - kRad, y0 = blockIdx.y * kTile - kRad;
  const size_t pixels = (size_t)A.width * A.height;
  const float* __restrict__ img = A.image + (size_t)view * pixels * A.image_stride;
  // (a byte target may sit at an odd address: no float pointer is formed from it)
  const float* __restrict__ tf = kU8 ? nullptr : (const float*)A.target + (size_t)view * pixels * A.target_stride;
  const uint8_t* __restrict__ tu = kU8 ? (const uint8_t*)A.target + (size_t)view * pixels * 3 : nullptr;
  for (int e = tid; e < kHalo * kHalo; e += 256) {
    const int r = e / kHalo, c = e - r * kHalo, x = x0 + c, y = y0 + r;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    if (x >= 0 && x < A.width && y >= 0 && y < A.height) {
      const size_t p = (size_t)y * A.width + x;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        a[ch] = input_rule<kQ>(img[p * A.image_stride + ch], s_val);
        b[ch] = kU8 ? s_val[tu[p * 3 + ch]] : input_rule<kQ>(tf[p * A.target_stride + ch], s_val);
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      s_a[(ch * kHalo + r) * kHaloStride + c] = a[ch];
      s_b[(ch * kHalo + r) * kHaloStride + c] = b[ch];
    }
  }
  __syncthreads();
  const int px = blockIdx.x * kTile + tx, py = blockIdx.y * kTile + ty;
  const bool inside = px < A.width && py < A.height;
  float sum_m = 0.f, sum_l1 = 0.f, sq[3] = {0.f, 0.f, 0.f};
  uint32_t isum_l1 = 0, isq[3] = {0, 0, 0};
  int bytes[3] = {0, 0, 0};
  for (int ch = 0; ch < 3; ++ch) {
    const float* __restrict__ ca = s_a + ch * kHalo * kHaloStride;
    const float* __restrict__ cb = s_b + ch * kHalo * kHaloStride;
    blur_rows<5>(s_h, [&](int row, int col, float* v) {
      const float a = ca[row * kHaloStride + col], b = cb[row * kHaloStride + col];
      v[0] = a; v[1] = b; v[2] = a * a; v[3] = b * b; v[4] = a * b;
    });
    __syncthreads();
    float mo[5];
    blur_cols<5>(s_h, ty, tx, mo);
    __syncthreads();              // s_h is rewritten by the next channel
    if (inside) {
      const float mu1 = mo[0], mu2 = mo[1];
      const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float s1 = mo[2] - mu1sq, s2 = mo[3] - mu2sq, s12 = mo[4] - mu12;
      const float A1 = 2.f * mu12 + kC1, A2 = 2.f * s12 + kC2, B1 = (mu1sq + mu2sq) + kC1, B2 = (s1 + s2) + kC2;
      const float den = B1 * B2;
      const float m = (A1 * A2) / den;
      const float a = ca[(ty + kRad) * kHaloStride + tx + kRad], b = cb[(ty + kRad) * kHaloStride + tx + kRad];
      sum_m = ch == 0 ? m : sum_m + m;
      // the 8-bit rule maps the value of a byte, and the byte of a clamped value, to the byte of the value itself
      bytes[ch] = to_byte(a);
      if (kQ) {
        const int d = bytes[ch] - to_byte(b);
        isum_l1 += (uint32_t)(d < 0 ? -d : d);
        isq[ch] = (uint32_t)(d * d);
      } else {
        const float d = a - b;
        sum_l1 = ch == 0 ? fabsf(d) : sum_l1 + fabsf(d);
        sq[ch] = d * d;
      }
    }
  }
  if (A.render && inside) {
    uint8_t* __restrict__ o = A.render + ((size_t)view * pixels + (size_t)py * A.width + px) * 3;
    o[0] = (uint8_t)bytes[0];
    o[1] = (uint8_t)bytes[1];
    o[2] = (uint8_t)bytes[2];
  }
  // the tile's fixed tree: the 256 pixels in 4 groups of 64 (rows-of-16 order), lanes by xor 32 .. 1, then the groups in order
  sum_m = sdg_wave_sum(sum_m);
  uint32_t* __restrict__ mine = s_sum + kSums * sdg_wave();
  if (kQ) {
    isum_l1 = sdg_wave_sum(isum_l1);
    for (int ch = 0; ch < 3; ++ch) isq[ch] = sdg_wave_sum(isq[ch]);
    if (sdg_lane() == 0) {
      mine[0] = __float_as_uint(sum_m);
      mine[1] = isum_l1;
      for (int ch = 0; ch < 3; ++ch) mine[2 + ch] = isq[ch];
    }
  } else {
    sum_l1 = sdg_wave_sum(sum_l1);
    for (int ch = 0; ch < 3; ++ch) sq[ch] = sdg_wave_sum(sq[ch]);
    if (sdg_lane() == 0) {
      mine[0] = __float_as_uint(sum_m);
      mine[1] = __float_as_uint(sum_l1);
      for (int ch = 0; ch < 3; ++ch) mine[2 + ch] = __float_as_uint(sq[ch]);
    }
  }
  __syncthreads();
  if (tid < kSums) {
    uint32_t out;
    if (kQ && tid > 0)
      out = ((s_sum[tid] + s_sum[kSums + tid]) + s_sum[2 * kSums + tid]) + s_sum[3 * kSums + tid];
    else
      out = __float_as_uint(((__uint_as_float(s_sum[tid]) + __uint_as_float(s_sum[kSums + tid])) + __uint_as_float(s_sum[2 * kSums + tid])) +
                            __uint_as_float(s_sum[3 * kSums + tid]));
    A.part[((size_t)view * (gridDim.x * gridDim.y) + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSums + tid] = out;
  }
}

// A view's tiles added in row-major order (staged 256 tiles at a time, lanes 0 .. 4 add them one after the other), then the six outputs.
template <bool kQ>
__global__ __launch_bounds__(256) void k_metrics_reduce(const uint32_t* __restrict__ part, int tiles, int width, int height,
                                                        float* __restrict__ metrics) {
  __shared__ uint32_t s_part[256 * kSums];
  __shared__ float s_f[kSums];
  __shared__ unsigned long long s_i[kSums];
  const int view = blockIdx.x, tid = threadIdx.x;
  const uint32_t* __restrict__ p = part + (size_t)view * tiles * kSums;
  float acc = 0.f;
  unsigned long long iacc = 0;
  for (int t0 = 0; t0 < tiles; t0 += 256) {
    const int m = min(256, tiles - t0);
    __syncthreads();
    for (int e = tid; e < kSums * m; e += 256) s_part[e] = p[(size_t)t0 * kSums + e];
    __syncthreads();
    if (tid < kSums)      // one loop for the five lanes: a lane keeps the sum of its kind and ignores the other
      for (int t = 0; t < m; ++t) {
        const uint32_t w = s_part[kSums * t + tid];
        acc += __uint_as_float(w);
        if (kQ) iacc += w;
      }
  }
  if (tid < kSums) {
    s_f[tid] = acc;
    s_i[tid] = iacc;
  }
  __syncthreads();
  if (tid == 0) {
    float* __restrict__ o = metrics + 6 * (size_t)view;
    const int64_t hw = (int64_t)width * height;
    const float n3 = (float)(3 * hw), n1 = (float)hw;
    o[1] = s_f[0] / n3;
    if (kQ) {
      o[0] = (float)((double)s_i[1] / (255.0 * (double)(3 * hw)));
      o[2] = (float)((double)(s_i[2] + s_i[3] + s_i[4]) / (65025.0 * (double)(3 * hw)));
      for (int ch = 0; ch < 3; ++ch) o[3 + ch] = (float)((double)s_i[2 + ch] / (65025.0 * (double)hw));
    } else {
      o[0] = s_f[1] / n3;
      o[2] = ((s_f[2] + s_f[3]) + s_f[4]) / n3;
      for (int ch = 0; ch < 3; ++ch) o[3 + ch] = s_f[2 + ch] / n1;
    }
  }
}

// Behind a chunk of sixdgs_evaluate_views: the largest count, and NaN rows with bit 1 when the rasteriser's capacity did not hold it
__global__ __launch_bounds__(64) void k_eval_record(const int64_t* __restrict__ count, int64_t max_instances, int views, float* __restrict__ metrics,
                                                    int32_t* __restrict__ status, int64_t* __restrict__ instances_needed) {
  const int64_t cnt = *count;
  const bool over = cnt > max_instances;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (cnt > *instances_needed) *instances_needed = cnt;
    if (over) *status |= 2;
  }
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (over && e < 6 * views) metrics[e] = NAN;
}

struct EvalLayout : SdgBump {
  size_t fwd, metrics, image, count;
  size_t fwd_bytes, metrics_bytes;
};

// 0 total = outside the limits
EvalLayout eval_layout(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  EvalLayout L = {};
  if (chunk < 1 || !sizes_ok(chunk, width, height)) return L;
  L.fwd_bytes = sixdgs_raster_views_workspace_bytes(n, chunk, width, height, max_instances);
  L.metrics_bytes = part_bytes(chunk, width, height);
  if (L.fwd_bytes == 0) return L;
  L.fwd = L.take(L.fwd_bytes);
  L.metrics = L.take(L.metrics_bytes);
  L.image = L.take((size_t)chunk * (size_t)height * (size_t)width * 4 * sizeof(float));
  L.count = L.take(sizeof(int64_t));
  return L;
}

}  // namespace

extern "C" {

size_t sixdgs_image_metrics_workspace_bytes(int views, int width, int height) {
  if (!sizes_ok(views, width, height)) return 0;
  return part_bytes(views, width, height);
}

int sixdgs_image_metrics(const float* image, int image_stride, const void* target, int target_is_u8, int target_stride, int views, int width,
                         int height, int quantise, float* metrics, uint8_t* render_u8, void* ws, size_t ws_bytes, sixdgs_stream_t stream,
                         sixdgs_profile* prof) {
  const Image I = {image, image_stride};
  const Target T = {target, target_is_u8, target_stride};
  SDG_CHECK_ARG(sizes_ok(views, width, height));
  SDG_CHECK_ARG(image_ok(I) && target_ok(T) && quantise_ok(quantise));
  if (views == 0) return 0;
  SDG_CHECK_ARG(image_present(I) && target_present(T));
  SDG_CHECK_ARG(metrics && aligned4(metrics));
  const size_t need = part_bytes(views, width, height);
  if (ws_bytes < need) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)views);
  uint32_t* part = (uint32_t*)ws;
  const double px = (double)views * width * height;
  {
    SdgProfileScope t(prof, s, 0, px * (4.0 * image_stride + (target_is_u8 ? 3.0 : 4.0 * target_stride) + (render_u8 ? 3.0 : 0.0)));
    const FwdArgs A = {image, target, part, render_u8, width, height, image_stride, target_stride};
    if (target_is_u8) {
      if (quantise)
        hipLaunchKernelGGL((k_metrics_fwd<true, true>), grid, dim3(256), 0, s, A);
      else
        hipLaunchKernelGGL((k_metrics_fwd<true, false>), grid, dim3(256), 0, s, A);
    } else {
      if (quantise)
        hipLaunchKernelGGL((k_metrics_fwd<false, true>), grid, dim3(256), 0, s, A);
      else
        hipLaunchKernelGGL((k_metrics_fwd<false, false>), grid, dim3(256), 0, s, A);
    }
    SDG_LAUNCH_OK();
  }
  {
    SdgProfileScope t(prof, s, 0, (double)views * gx * gy * 4.0 * kSums);
    if (quantise)
      hipLaunchKernelGGL(k_metrics_reduce<true>, dim3((unsigned)views), dim3(256), 0, s, (const uint32_t*)part, gx * gy, width, height, metrics);
    else
      hipLaunchKernelGGL(k_metrics_reduce<false>, dim3((unsigned)views), dim3(256), 0, s, (const uint32_t*)part, gx * gy, width, height, metrics);
    SDG_LAUNCH_OK();
  }
  return 0;
}

size_t sixdgs_evaluate_views_workspace_bytes(int64_t n, int chunk, int width, int height, int64_t max_instances) {
  return eval_layout(n, chunk, width, height, max_instances).total;
}

int sixdgs_evaluate_views(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                          const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* cams, int views, int width,
                          int height, float scale_modifier, const float* background, const void* target, int target_is_u8, int target_stride,
                          int quantise, int chunk, int64_t max_instances, float* metrics, uint8_t* render_u8, int32_t* status,
                          int64_t* instances_needed, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const EvalLayout L = eval_layout(n, chunk, width, height, max_instances);
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  const Target T = {target, target_is_u8, target_stride};
  SDG_CHECK_ARG(L.total != 0 && views >= 0 && views <= kMaxViews);
  SDG_CHECK_ARG(scene_ok(S, sh_degree) && target_ok(T) && quantise_ok(quantise));
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && scene_present(S) && target_present(T));
  SDG_CHECK_ARG(metrics && status && instances_needed);
  SDG_CHECK_ARG(aligned4(cams) && aligned4(metrics) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  float* image = (float*)(w + L.image);
  int64_t* count = (int64_t*)(w + L.count);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(instances_needed, 0, sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  const size_t pixels = (size_t)width * height;
  const size_t target_view = pixels * (size_t)target_stride * (target_is_u8 ? 1 : sizeof(float));
  for (int v0 = 0; v0 < views; v0 += chunk) {
    const int nv = views - v0 < chunk ? views - v0 : chunk;
    int st = sixdgs_raster_views(S.xyz, S.scale, S.scale_is_log, S.rot, S.opacity, S.opacity_is_logit, S.f_dc, S.f_rest, sh_degree, S.n_coef, S.n,
                                 cams + 16 * (size_t)v0, nv, width, height, S.scale_modifier, S.background, image, nullptr, 3, nullptr,
                                 max_instances, count, w + L.fwd, L.fwd_bytes, stream, nullptr);
    if (st != 0) return st;
    float* rows = metrics + 6 * (size_t)v0;
    st = sixdgs_image_metrics(image, 4, (const char*)target + (size_t)v0 * target_view, target_is_u8, target_stride, nv, width, height, quantise,
                              rows, render_u8 ? render_u8 + (size_t)v0 * pixels * 3 : nullptr, w + L.metrics, L.metrics_bytes, stream, nullptr);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_eval_record, dim3((unsigned)sdg_cdiv(6 * nv, 64)), dim3(64), 0, s, (const int64_t*)count, max_instances, nv, rows, status,
                       instances_needed);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
