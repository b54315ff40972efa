// splat.hip -- synthetic query views of a 3DGS scene: every Gaussian as a flat, z-buffered disc (include/sixdgs.h,
// sixdgs_splat_views).  NOT the 3DGS rasteriser: no blending, no anisotropic footprint, no anti-aliasing.  The image is
// defined pixel by pixel in the header; tests/splat_reference.py restates that definition in fp64.
//
//   pass 1  k_splat_project  one lane per (view, Gaussian): project, cull, colour once (the emitters' SH evaluation) as
//           packed RGBA8, then a 64-bit atomicMin of (float bits of p.z << 32 | index) on the depth buffer for every
//           covered pixel.  p.z > 0, so its bit pattern orders like its value; the index in the low half is the tie rule
//           (equal depth -> smaller index), which makes the image independent of scheduling.  Discs of at most
//           kLaneWalkPixels bounding-box pixels are walked by their own lane; larger ones by the whole wave, one after
//           the other, row-major (neighbouring lanes on neighbouring pixels).
//   pass 2  k_splat_resolve  one thread per pixel: unpack the winner, gather its colour, write the uint8 pixel.
#include "common.h"
#include "device_math.h"

namespace {

using namespace sdg;

typedef unsigned long long u64;

constexpr int kLaneWalkPixels = 16;     // bounding boxes up to this many pixels stay on their lane
constexpr u64 kNoWinner = ~0ull;        // what hipMemsetAsync(0xFF) leaves

struct SplatArgs {
  const float* xyz;
  const float* scale;
  const float* f_dc;
  const float* f_rest;
  const float* cams;       // [views][16]: w2c rows 0..2 (3 x 4), fx, fy, cx, cy
  u64* depth;              // [views][H][W]
  uint32_t* color;         // [views][n] packed RGBA8 (A = 255), written for the Gaussians that reach the frame
  int64_t n;
  int scale_is_log, sh_degree, n_coef;
  int width, height;
  float extent, near_z;
};

// the z-test of one pixel.  The plain read may be stale, but the buffer only ever decreases: a stale value is a larger
// one and costs an atomic that changes nothing, never a missed write.
__device__ __forceinline__ void splat_pixel(u64* __restrict__ depth, int width, int x, int y, float u, float v, float r2, u64 key) {
  const float dx = ((float)x + 0.5f) - u, dy = ((float)y + 0.5f) - v;
  if (dx * dx + dy * dy <= r2) {
    u64* p = depth + (size_t)y * width + x;
    if (*p > key) atomicMin(p, key);
  }
}

__global__ __launch_bounds__(256) void k_splat_project(SplatArgs A) {
  const int view = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float* __restrict__ cam = A.cams + 16 * (size_t)view;
  u64* __restrict__ depth = A.depth + (size_t)view * A.height * A.width;

  bool active = false;
  int x0 = 0, y0 = 0, bw = 0, bh = 0;
  float u = 0.f, v = 0.f, r2 = 0.f;
  u64 key = kNoWinner;
  if (i < A.n) {
    const float X = A.xyz[3 * i], Y = A.xyz[3 * i + 1], Z = A.xyz[3 * i + 2];
    const float pz = ((cam[8] * X + cam[9] * Y) + cam[10] * Z) + cam[11];
    if (pz > A.near_z) {                  // (false for NaN too)
      const float px = ((cam[0] * X + cam[1] * Y) + cam[2] * Z) + cam[3];
      const float py = ((cam[4] * X + cam[5] * Y) + cam[6] * Z) + cam[7];
      const float fx = cam[12], fy = cam[13];
      u = fx * px / pz + cam[14];
      v = fy * py / pz + cam[15];
      float s0 = A.scale[3 * i], s1 = A.scale[3 * i + 1], s2 = A.scale[3 * i + 2];
      if (A.scale_is_log) { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }
      const float r = fmaxf(A.extent * fmaxf(fmaxf(s0, s1), s2) * fx / pz, 0.7072f);
      r2 = r * r;
      // pixel x is covered only if |x + 0.5 - u| <= r.  Clamped as floats first: u, v and r may be huge or not finite.
      const float fx0 = fmaxf(floorf(u - r - 0.5f), 0.f), fx1 = fminf(ceilf(u + r - 0.5f), (float)(A.width - 1));
      const float fy0 = fmaxf(floorf(v - r - 0.5f), 0.f), fy1 = fminf(ceilf(v + r - 0.5f), (float)(A.height - 1));
      if (fx0 <= fx1 && fy0 <= fy1) {     // (false for NaN; a disc entirely outside the frame ends here)
        active = true;
        x0 = (int)fx0; y0 = (int)fy0;
        bw = (int)fx1 - x0 + 1; bh = (int)fy1 - y0 + 1;
        key = ((u64)__float_as_uint(pz) << 32) | (u64)(uint32_t)i;
        // colour: the camera centre is -W^T t; view direction = normalize(xyz - centre)
        const float t0 = cam[3], t1 = cam[7], t2 = cam[11];
        const float cx = -((cam[0] * t0 + cam[4] * t1) + cam[8] * t2);
        const float cy = -((cam[1] * t0 + cam[5] * t1) + cam[9] * t2);
        const float cz = -((cam[2] * t0 + cam[6] * t1) + cam[10] * t2);
        const V3 d = normalize_eps(v3(X - cx, Y - cy, Z - cz));
        float sh[48];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sh[ch] = A.f_dc[3 * i + ch];
#pragma unroll
        for (int k = 1; k < 16; ++k)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) sh[3 * k + ch] = k < A.n_coef ? A.f_rest[(i * (A.n_coef - 1) + (k - 1)) * 3 + ch] : 0.f;
        uint32_t rgba = 0xff000000u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float c = fminf(sh_channel(sh + ch, 3, A.sh_degree, d.x, d.y, d.z), 1.f);
          rgba |= (uint32_t)rintf(255.f * c) << (8 * ch);
        }
        A.color[(size_t)view * A.n + i] = rgba;
      }
    }
  }

  const int area = bw * bh;
  const bool own = active && area <= kLaneWalkPixels;
  if (own) {
    for (int y = y0; y < y0 + bh; ++y)
      for (int x = x0; x < x0 + bw; ++x) splat_pixel(depth, A.width, x, y, u, v, r2, key);
  }
  // the larger discs of this wave, one at a time, over its 64 lanes
  u64 todo = __ballot(active && !own);
  const int lane = sdg_lane();
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sw = __shfl(bw, src, 64), sarea = __shfl(area, src, 64);
    const float su = __shfl(u, src, 64), sv = __shfl(v, src, 64), sr2 = __shfl(r2, src, 64);
    const u64 skey = ((u64)(uint32_t)__shfl((int)(key >> 32), src, 64) << 32) | (u64)(uint32_t)__shfl((int)(uint32_t)key, src, 64);
    for (int p = lane; p < sarea; p += 64) {
      const int row = p / sw;
      splat_pixel(depth, A.width, sx0 + (p - row * sw), sy0 + row, su, sv, sr2, skey);
    }
  }
}

__global__ __launch_bounds__(256) void k_splat_resolve(const u64* __restrict__ depth, const uint32_t* __restrict__ color, int64_t n,
                                                       int64_t pixels_per_view, int64_t pixels, int channels,
                                                       const float* __restrict__ background, uint8_t* __restrict__ image,
                                                       int32_t* __restrict__ winner) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const u64 key = depth[p];
  const bool hit = key != kNoWinner;
  uint32_t rgba = 0;
  if (hit) {
    rgba = color[(p / pixels_per_view) * n + (int64_t)(uint32_t)key];
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgba |= (uint32_t)rintf(255.f * fminf(fmaxf(background[ch], 0.f), 1.f)) << (8 * ch);
  }
  if (channels == 4) {
    reinterpret_cast<uint32_t*>(image)[p] = rgba;            // alpha: 255 on a covered pixel (set in pass 1), 0 elsewhere
  } else {
    uint8_t* o = image + 3 * p;
    o[0] = (uint8_t)rgba; o[1] = (uint8_t)(rgba >> 8); o[2] = (uint8_t)(rgba >> 16);
  }
  if (winner) winner[p] = hit ? (int32_t)(uint32_t)key : -1;
}

constexpr int kMaxSide = 16384;

}  // namespace

extern "C" {

size_t sixdgs_splat_views_workspace_bytes(int64_t n, int views, int width, int height) {
  if (n < 0 || views < 0 || width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return 0;
  return sdg_align((size_t)views * height * width * sizeof(u64)) + sdg_align((size_t)views * (size_t)n * sizeof(uint32_t));
}

int sixdgs_splat_views(const float* xyz, const float* scale, int scale_is_log, const float* f_dc, const float* f_rest, int sh_degree,
                       int n_coef, int64_t n, const float* cams, int views, int width, int height, int channels, float extent,
                       float near_z, const float* background, uint8_t* image, int32_t* winner, void* ws, size_t ws_bytes,
                       sixdgs_stream_t stream) {
  SDG_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) && views >= 0 && views <= 65535);
  SDG_CHECK_ARG(width >= 1 && height >= 1 && width <= kMaxSide && height <= kMaxSide);
  SDG_CHECK_ARG(channels == 3 || channels == 4);
  SDG_CHECK_ARG(extent > 0.f && extent < INFINITY && near_z >= 0.f);
  SDG_CHECK_ARG(sh_degree >= 0 && sh_degree <= 3 && n_coef >= (sh_degree + 1) * (sh_degree + 1) && n_coef <= 16);
  if (views == 0) return 0;
  SDG_CHECK_ARG(cams && background && image);
  SDG_CHECK_ARG(n == 0 || (xyz && scale && f_dc && (n_coef == 1 || f_rest)));
  const size_t depth_bytes = (size_t)views * height * width * sizeof(u64);
  if (ws_bytes < sixdgs_splat_views_workspace_bytes(n, views, width, height)) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  u64* depth = (u64*)ws;
  uint32_t* color = (uint32_t*)((char*)ws + sdg_align(depth_bytes));
  hipError_t e = hipMemsetAsync(depth, 0xFF, depth_bytes, s);
  if (e != hipSuccess) return (int)e;
  if (n > 0) {
    SplatArgs A = {xyz, scale, f_dc, f_rest, cams, depth, color, n, scale_is_log, sh_degree, n_coef, width, height, extent, near_z};
    hipLaunchKernelGGL(k_splat_project, dim3((unsigned)sdg_cdiv(n, 256), (unsigned)views), dim3(256), 0, s, A);
    SDG_LAUNCH_OK();
  }
  const int64_t ppv = (int64_t)width * height, pixels = ppv * views;
  hipLaunchKernelGGL(k_splat_resolve, dim3((unsigned)sdg_cdiv(pixels, 256)), dim3(256), 0, s, depth, color, n, ppv, pixels, channels,
                     background, image, winner);
  SDG_LAUNCH_OK();
  return 0;
}

}  // extern "C"
