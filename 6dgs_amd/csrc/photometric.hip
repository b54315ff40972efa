// photometric.hip -- the fused photometric loss (1 - lambda) L1 + lambda (1 - SSIM) and its gradient by the image
// (sixdgs_photometric_loss in include/sixdgs.h defines both operation by operation; the step numbers below are the header's).
//
// One 256-thread workgroup per 16 x 16 tile and view, the rasteriser's tiles.  Forward: the 26 x 26 halo of the image and of the target,
// all three channels, goes to LDS (zeros outside the image); per channel a horizontal pass writes the five blurred rows
// (a, b, a^2, b^2, ab) of the 26 halo rows to LDS, a vertical pass leaves the five moments of a thread's pixel in registers.  From them
// the SSIM value, the three derivative maps (to the workspace, planar) and the pixel's share of the two sums; the tile's sums go to the
// view's slot array, k_photo_reduce adds a view's tiles in order.  Gradient: the same two passes over the halo of the three maps.
//
// LDS rows: the halo arrays have a row stride of 48 floats and the horizontal pass's output one of 16.  ds_read_b32 / ds_write_b32
// bank by (address / 4) mod 32 within each 32-lane half, and a half is two rows of 16 lanes in both passes: with a stride of 16 mod 32
// the two rows fall on opposite halves of the banks, so neither pass has a conflict (a stride of 26 or 27 would cost 2-way on 11 banks).
// The halo's staging writes are not conflict-free: 32 consecutive halo elements run over a row's end, lanes 26 .. 31 start the next row
// at +48 floats (banks 16 .. 21) and meet lanes 16 .. 21 there, 2-way on 6 banks, 3 rounds of stores per array and channel: accepted,
// the staging waits on the global loads.
#include <math.h>

#include "common.h"

namespace {

constexpr int kTile = 16;                 // the rasteriser's tile
constexpr int kTaps = 11, kRad = 5;
constexpr int kHalo = kTile + 2 * kRad;   // 26
constexpr int kHaloStride = 48;
constexpr int kMaxDim = 16384, kMaxViews = 65535;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;

__constant__ float c_w[kTaps] = SIXDGS_SSIM_WINDOW;

bool sizes_ok(int views, int width, int height) {
  if (views < 0 || views > kMaxViews || width < 1 || width > kMaxDim || height < 1 || height > kMaxDim) return false;
  return (int64_t)views * sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile) < ((int64_t)1 << 31);
}

struct Layout : SdgBump {
  size_t part, maps;
};

Layout layout(int views, int width, int height, int want_grad) {
  Layout L = {};
  L.part = L.take((size_t)views * (size_t)(sdg_cdiv(width, kTile) * sdg_cdiv(height, kTile)) * 2 * sizeof(float));
  L.maps = L.take(want_grad ? (size_t)views * 9 * (size_t)width * (size_t)height * sizeof(float) : 0);
  return L;
}

// The horizontal pass of NQ quantities over the 26 halo rows: s_h[q][row][col] = sum_k w[k] f_q(row, col + k), k ascending.
// load(row, col, out[NQ]) gives the NQ values at a halo position.
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

// The vertical pass for the thread's pixel (ty, tx): out[q] = sum_k w[k] s_h[q][ty + k][tx], k ascending.
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
  float* part;      // [views][gy * gx][2]: the tile's sums of |a - b| and of m
  float* maps;      // [views][3 maps][3 channels][height][width] or NULL
  int width, height, image_stride, target_stride;
};

template <bool kU8>
__global__ __launch_bounds__(256) void k_photo_fwd(FwdArgs A) {
  __shared__ float s_a[3 * kHalo * kHaloStride], s_b[3 * kHalo * kHaloStride];
  __shared__ float s_h[5 * kHalo * kTile];
  __shared__ float s_sum[8];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, view = blockIdx.z;
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
        a[ch] = img[p * A.image_stride + ch];
        b[ch] = kU8 ? (float)tu[p * 3 + ch] / 255.0f : tf[p * A.target_stride + ch];
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
  float sum_l1 = 0.f, sum_m = 0.f;
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
      sum_l1 = ch == 0 ? fabsf(a - b) : sum_l1 + fabsf(a - b);
      sum_m = ch == 0 ? m : sum_m + m;
      if (A.maps) {
        const float d_s1 = -(m / B2);
        const float d_s12 = (2.f * A1) / den;
        const float d_mu1 = (((2.f * mu2) * A2) / den - ((2.f * mu1) * m) / B1) - ((2.f * mu1) * d_s1 + mu2 * d_s12);
        float* __restrict__ mp = A.maps + ((size_t)view * 9 + ch) * pixels + (size_t)py * A.width + px;
        mp[0] = d_mu1;
        mp[3 * pixels] = d_s1;
        mp[6 * pixels] = d_s12;
      }
    }
  }
  // the tile's fixed tree: the 256 pixels in 4 groups of 64 (rows-of-16 order), lanes by xor 32 .. 1, then the groups in order
  sum_l1 = sdg_wave_sum(sum_l1);
  sum_m = sdg_wave_sum(sum_m);
  if (sdg_lane() == 0) {
    s_sum[2 * sdg_wave()] = sum_l1;
    s_sum[2 * sdg_wave() + 1] = sum_m;
  }
  __syncthreads();
  if (tid < 2)
    A.part[((size_t)view * (gridDim.x * gridDim.y) + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + tid] =
        ((s_sum[tid] + s_sum[2 + tid]) + s_sum[4 + tid]) + s_sum[6 + tid];
}

// A view's tiles added in row-major order (staged 256 tiles at a time, lanes 0 and 1 add them one after the other), then the means.
__global__ __launch_bounds__(256) void k_photo_reduce(const float* __restrict__ part, int tiles, float count, float lambda,
                                                      float* __restrict__ loss, float* __restrict__ parts) {
  __shared__ float s_part[512];
  const int view = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ p = part + (size_t)view * tiles * 2;
  float acc = 0.f;
  for (int t0 = 0; t0 < tiles; t0 += 256) {
    const int m = min(256, tiles - t0);
    __syncthreads();
    for (int e = tid; e < 2 * m; e += 256) s_part[e] = p[(size_t)t0 * 2 + e];
    __syncthreads();
    if (tid < 2)
      for (int t = 0; t < m; ++t) acc += s_part[2 * t + tid];
  }
  __syncthreads();
  if (tid < 2) s_part[tid] = acc / count;
  __syncthreads();
  if (tid == 0) {
    const float l1 = s_part[0], ssim = s_part[1];
    if (parts) {
      parts[2 * view] = l1;
      parts[2 * view + 1] = ssim;
    }
    if (loss) loss[view] = (1.f - lambda) * l1 + lambda * (1.f - ssim);
  }
}

struct GradArgs {
  const float* image;
  const void* target;
  const float* maps;
  const float* grad_loss;       // [views] or NULL
  float* grad_image;
  int width, height, image_stride, target_stride;
  float c_l1, c_ssim;           // (1 - lambda) / count, lambda / count
};

template <bool kU8>
__global__ __launch_bounds__(256) void k_photo_grad(GradArgs A) {
  __shared__ float s_m[3 * kHalo * kHaloStride];
  __shared__ float s_h[3 * kHalo * kTile];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, view = blockIdx.z;
  const int x0 = blockIdx.x * kTile - kRad, y0 = blockIdx.y * kTile - kRad;
  const size_t pixels = (size_t)A.width * A.height;
  const int px = blockIdx.x * kTile + tx, py = blockIdx.y * kTile + ty;
  const bool inside = px < A.width && py < A.height;
  const size_t p = (size_t)view * pixels + (inside ? (size_t)py * A.width + px : 0);
  const float gl = A.grad_loss ? A.grad_loss[view] : 1.f;
  float g[3];
  for (int ch = 0; ch < 3; ++ch) {
    const float* __restrict__ mp = A.maps + ((size_t)view * 9 + ch) * pixels;
    __syncthreads();              // the passes of the channel before are done with s_m
    for (int e = tid; e < kHalo * kHalo; e += 256) {
      const int r = e / kHalo, c = e - r * kHalo, x = x0 + c, y = y0 + r;
      const bool in = x >= 0 && x < A.width && y >= 0 && y < A.height;
      const size_t at = in ? (size_t)y * A.width + x : 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) s_m[(q * kHalo + r) * kHaloStride + c] = in ? mp[3 * q * pixels + at] : 0.f;
    }
    __syncthreads();
    blur_rows<3>(s_h, [&](int row, int col, float* v) {
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] = s_m[(q * kHalo + row) * kHaloStride + col];
    });
    __syncthreads();
    float bl[3];
    blur_cols<3>(s_h, ty, tx, bl);
    g[ch] = 0.f;
    if (inside) {
      const float a = A.image[p * A.image_stride + ch];
      const float b = kU8 ? (float)((const uint8_t*)A.target)[p * 3 + ch] / 255.0f : ((const float*)A.target)[p * A.target_stride + ch];
      const float d = a - b;
      const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      const float x = (bl[0] + (2.f * a) * bl[1]) + b * bl[2];
      g[ch] = gl * (A.c_l1 * sg - A.c_ssim * x);
    }
  }
  if (inside) {
    float* __restrict__ o = A.grad_image + p * A.image_stride;
    o[0] = g[0];
    o[1] = g[1];
    o[2] = g[2];
    if (A.image_stride == 4) o[3] = 0.f;
  }
}

}  // namespace

extern "C" {

size_t sixdgs_photometric_loss_workspace_bytes(int views, int width, int height, int want_grad) {
  if (!sizes_ok(views, width, height)) return 0;
  return layout(views, width, height, want_grad).total;
}

int sixdgs_photometric_loss(const float* image, int image_stride, const void* target, int target_is_u8, int target_stride, int views,
                            int width, int height, float lambda, const float* grad_loss, float* loss, float* parts, float* grad_image,
                            void* ws, size_t ws_bytes, sixdgs_stream_t stream, sixdgs_profile* prof) {
  SDG_CHECK_ARG(sizes_ok(views, width, height));
  SDG_CHECK_ARG(image_stride == 3 || image_stride == 4);
  SDG_CHECK_ARG(target_is_u8 == 0 || target_is_u8 == 1);
  SDG_CHECK_ARG(target_is_u8 ? target_stride == 3 : (target_stride == 3 || target_stride == 4));
  SDG_CHECK_ARG(lambda >= 0.f && lambda <= 1.f);
  if (views == 0) return 0;
  SDG_CHECK_ARG(image && target);
  SDG_CHECK_ARG(((uintptr_t)image & 3) == 0 && (target_is_u8 || ((uintptr_t)target & 3) == 0));
  SDG_CHECK_ARG(((uintptr_t)grad_loss & 3) == 0 && ((uintptr_t)loss & 3) == 0 && ((uintptr_t)parts & 3) == 0 && ((uintptr_t)grad_image & 3) == 0);
  if (!(loss || parts || grad_image)) return 0;
  const int want_grad = grad_image != nullptr;
  const Layout L = layout(views, width, height, want_grad);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  const int gx = (int)sdg_cdiv(width, kTile), gy = (int)sdg_cdiv(height, kTile);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)views);
  float* part = (float*)(w + L.part);
  float* maps = want_grad ? (float*)(w + L.maps) : nullptr;
  const float count = (float)(3 * (int64_t)width * height);
  const double px = (double)views * width * height;
  {
    SdgProfileScope t(prof, s, 0, px * (3.0 * (target_is_u8 ? 5.0 : 8.0) + (want_grad ? 36.0 : 0.0)));
    FwdArgs A = {image, target, part, maps, width, height, image_stride, target_stride};
    if (target_is_u8)
      hipLaunchKernelGGL(k_photo_fwd<true>, grid, dim3(256), 0, s, A);
    else
      hipLaunchKernelGGL(k_photo_fwd<false>, grid, dim3(256), 0, s, A);
    SDG_LAUNCH_OK();
  }
  if (loss || parts) {
    SdgProfileScope t(prof, s, 0, (double)views * gx * gy * 8.0);
    hipLaunchKernelGGL(k_photo_reduce, dim3((unsigned)views), dim3(256), 0, s, part, gx * gy, count, lambda, loss, parts);
    SDG_LAUNCH_OK();
  }
  if (want_grad) {
    SdgProfileScope t(prof, s, 0, px * (36.0 + 3.0 * (target_is_u8 ? 5.0 : 8.0) + 4.0 * image_stride));
    GradArgs G = {image, target, maps, grad_loss, grad_image, width, height, image_stride, target_stride, (1.f - lambda) / count, lambda / count};
    if (target_is_u8)
      hipLaunchKernelGGL(k_photo_grad<true>, grid, dim3(256), 0, s, G);
    else
      hipLaunchKernelGGL(k_photo_grad<false>, grid, dim3(256), 0, s, G);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
