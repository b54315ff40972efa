// pyramid_rules.h -- the rules of a coarse-to-fine refinement schedule, usable from device AND host code (include/sixdgs.h:
// sixdgs_target_pyramid and sixdgs_refine_poses_levels define every operation; pyramid.hip and refine.hip run them; hostcheck.cpp
// instantiates the same text for the CPU tests): a level's geometry, the value of a level's target pixel from exact integer block
// sums, and the rule that keeps the input pose.  No contraction into fused multiply-adds: every translation unit that includes this is
// built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef SDG_HD
#define SDG_HD __host__ __device__ __forceinline__
#endif

namespace sdg {
namespace pyr {

constexpr int kMaxLevels = 8;
// 1 <= d <= 256.  A block has d d <= 2^16 bytes, so S = sum of bytes <= 255 * 2^16 < 2^24 and 255 d d <= 255 * 2^16 < 2^24: both are
// integers an fp32 holds exactly, and float(S) / float(255 d d) has ONE rounding, the division's.  S2 = sum (255 - u_a) obeys the same
// bound.  S1 = sum u_c u_a <= 255^2 * 2^16 = 4 261 478 400 < 2^32 = 4 294 967 296: it fits 32 unsigned bits (at d = 257 it would not).
constexpr int kMaxDownscale = 256;
constexpr int kMaxSide = 32768;      // of the query image: a level's rows and columns index a launch grid

// the level of downscale d of a W x H query: w x h pixels, each the mean of a d x d block of the centred crop that starts at (ox, oy)
struct Level {
  int w, h, ox, oy;
};
SDG_HD Level level_geometry(int W, int H, int d) {
  Level g;
  g.w = W / d;
  g.h = H / d;
  g.ox = (W - g.w * d) / 2;
  g.oy = (H - g.h * d) / 2;
  return g;
}

// (fx, fy, cx, cy) of the level: fx / d, fy / d, (cx - ox) / d, (cy - oy) / d, with d, ox and oy converted to fp32 first
SDG_HD void level_intrinsics(const float* k4, int d, int ox, int oy, float* out4) {
  const float df = (float)d;
  out4[0] = k4[0] / df;
  out4[1] = k4[1] / df;
  out4[2] = (k4[2] - (float)ox) / df;
  out4[3] = (k4[3] - (float)oy) / df;
}

// without compositing: S = the integer sum of the block's d d bytes of one channel
SDG_HD float value_plain(uint32_t S, int d) { return (float)S / (float)(255 * d * d); }

// 255 bg_c, formed once per channel and call
SDG_HD float background_term(float bg_c) { return 255.0f * bg_c; }

// with compositing: S1 = sum u_c u_a, S2 = sum (255 - u_a), both integer; bg255 = background_term(bg_c).  Term by term:
SDG_HD float value_composite(uint32_t S1, uint32_t S2, float bg255, int d) {
  const float s1 = (float)S1;               // rounds above 2^24
  const float s2 = (float)S2;               // exact
  const float over = bg255 * s2;
  const float num = s1 + over;
  const float den = 65025.0f * (float)(d * d);
  return num / den;
}

// A view keeps the input pose exactly when NOT (best_loss_last < loss_input): a NaN on either side keeps it, and so does a tie.
SDG_HD bool keep_input(float best_loss_last, float loss_input) { return !(best_loss_last < loss_input); }

}  // namespace pyr
}  // namespace sdg
