// image_prep_rules.h -- the rules of sixdgs_image_prep, usable from device AND host code (include/sixdgs.h defines the operation; vit.hip's
// k_image_prep runs it; hostcheck.cpp instantiates the same text for the CPU tests): the span and the normalised weights of one output index
// of the antialiased bicubic resize, the launcher's plan (tap count, band height, LDS rows and bytes) and the row window of a band.  No
// contraction into fused multiply-adds: every translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef SDG_HD
#define SDG_HD __host__ __device__ __forceinline__
#endif

namespace sdg {
namespace ip {

constexpr int kMaxTaps = 64;                  // padded taps per output index the kernel takes (scale <= 15)
constexpr size_t kLdsBudget = 150 * 1024;     // bytes of LDS one workgroup may ask for

SDG_HD float aa_cubic(float x) {      // upsample_antialias::BicubicFilterFunctor, a = -0.5
  const float a = -0.5f;
  x = fabsf(x);
  if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
  if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
  return 0.f;
}

// span [xmin, xmin + xsize) of output index i (of the resized grid) along an axis of n input samples, clipped to the input; -> its centre
SDG_HD float aa_span(int i, int n, float scale, float support, int& xmin, int& xsize) {
  const float center = scale * ((float)i + 0.5f);
  const int lo = (int)(center - support + 0.5f), hi = (int)(center + support + 0.5f);
  xmin = lo > 0 ? lo : 0;
  xsize = (hi < n ? hi : n) - xmin;
  return center;
}

// span and normalised weights of output index i (of the resized grid) along an axis of n input samples; w[0 .. kt): zero beyond xsize
SDG_HD void aa_weights(int i, int n, float scale, float support, int kt, float* w, int* meta) {
  int xmin, xsize;
  const float center = aa_span(i, n, scale, support, xmin, xsize);
  const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
  const float xmc = (float)xmin - center;
  float total = 0.f;
  for (int j = 0; j < kt; ++j) {
    float v = 0.f;
    if (j < xsize) {
      v = aa_cubic(((float)j + xmc + 0.5f) * invscale);
      total += v;
    }
    w[j] = v;
  }
  if (total != 0.f)
    for (int j = 0; j < xsize && j < kt; ++j) w[j] /= total;
  meta[0] = xmin;
  meta[1] = xsize < kt ? xsize : kt;
}

// what the launcher decides for a call: input / resized size and support per axis, kt = padded taps per output index, rb = output rows one
// workgroup handles as a band, nrmax = x-reduced input rows it reserves in LDS for a band, the LDS bytes of that layout
struct Plan {
  float sh, sw, sup_h, sup_w;       // support = 2 scale (scale >= 1), else 2
  int kt, rb, nrmax;
  size_t lds_bytes;
  bool supported;                   // false: kt beyond kMaxTaps (rb = 0), or not even a band of one row fits kLdsBudget (rb = 0)
};

SDG_HD Plan plan(int batch, int height, int width, int resized_h, int resized_w, int out_size) {
  Plan p;
  p.sh = (float)height / (float)resized_h;                 // area_pixel_compute_scale, align_corners = false, no scale factor given
  p.sw = (float)width / (float)resized_w;
  p.sup_h = p.sh >= 1.f ? 2.f * p.sh : 2.f;                // (interp_size 4) / 2 * scale
  p.sup_w = p.sw >= 1.f ? 2.f * p.sw : 2.f;
  const float sup = p.sup_h > p.sup_w ? p.sup_h : p.sup_w;
  const int taps = (int)ceilf(sup) * 2 + 1;                // the op's own window size
  p.kt = (taps + 3) & ~3;
  p.rb = 0;
  p.nrmax = 0;
  p.lds_bytes = 0;
  p.supported = false;
  if (p.kt > kMaxTaps) return p;                           // (scale > 15: not a query image of this pipeline)
  // band height: 8 output rows for batches that fill the chip anyway, 4 below (more workgroups, shorter each); fewer when the x-reduced rows do not fit the budget
  for (p.rb = (int64_t)batch * ((out_size + 7) / 8) >= 256 ? 8 : 4; p.rb >= 1; p.rb >>= 1) {
    p.nrmax = (int)((float)p.rb * p.sh + 2.f * p.sup_h) + 3;
    p.lds_bytes = sizeof(float) * (256 + (size_t)out_size * p.kt + 2 * (size_t)out_size + (size_t)p.rb * p.kt + 2 * (size_t)p.rb + (size_t)p.nrmax * 3 * out_size);
    if (p.lds_bytes <= kLdsBudget) break;
  }
  p.supported = p.rb >= 1;
  return p;
}

// the input rows [r0, r1) the band of output rows [oy0, oy0 + rows) of the crop reads, as the kernel forms them: r0 = the first row's span start,
// r1 = the largest span end (a span's size capped at kt, as aa_weights stores it)
SDG_HD void band_window(int top, int oy0, int rows, int height, float sh, float sup_h, int kt, int& r0, int& r1) {
  int xmin, xsize;
  aa_span(top + oy0, height, sh, sup_h, xmin, xsize);
  r0 = xmin;
  r1 = r0;
  for (int ry = 0; ry < rows; ++ry) {
    aa_span(top + oy0 + ry, height, sh, sup_h, xmin, xsize);
    const int end = xmin + (xsize < kt ? xsize : kt);
    r1 = end > r1 ? end : r1;
  }
}

}  // namespace ip
}  // namespace sdg
