// densify_rules.h -- the per-entry rules of one densification round, usable from device AND host code (include/sixdgs.h:
// sixdgs_densify defines every operation; densify.hip runs them one lane per candidate slot; hostcheck.cpp instantiates the same text
// for the CPU tests).  Classification compares STORED values with thresholds the host converted once into the stored domain, so it
// uses no transcendental; the only function that is not restatable to the bit is the expf of a child's position.  No contraction into
// fused multiply-adds: every translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include "device_math.h"

namespace sdg {
namespace dn {

constexpr int kKeep = 0, kClone = 1, kSplit = 2;
constexpr int kSegments = 4;                   // candidate segments: originals not split, clones, children copy 0, children copy 1
constexpr float kLogSplit = 0.470003629f;      // logf(1.6): the reference's / (0.8 * 2)
constexpr float kSplit16 = 1.6f;

// thresholds in the domain the arrays are stored in
struct Thresholds {
  float grad, dense, world, opacity;
  int prune_big, screen_size;
};

// HOST: each conversion once, in double, rounded to float.  percent_dense * extent and 0.1 * extent are products in double of the float
// arguments (0.1 the double constant); log for scale_is_log, log(p / (1 - p)) for opacity_is_logit (p = 0 gives -inf: nothing is below)
inline Thresholds thresholds(float grad_threshold, float percent_dense, float extent, float min_opacity, int scale_is_log,
                             int opacity_is_logit, int prune_big, int screen_size) {
  const double dense = (double)percent_dense * (double)extent, world = 0.1 * (double)extent, p = (double)min_opacity;
  Thresholds t;
  t.grad = grad_threshold;
  t.dense = (float)(scale_is_log ? log(dense) : dense);
  t.world = (float)(scale_is_log ? log(world) : world);
  t.opacity = (float)(opacity_is_logit ? log(p / (1.0 - p)) : p);
  t.prune_big = prune_big;
  t.screen_size = screen_size;
  return t;
}

SDG_HD float avg_grad(float accum, int32_t denom) { return denom > 0 ? accum / (float)denom : 0.f; }
SDG_HD float max3(const float* s) { return fmaxf(fmaxf(s[0], s[1]), s[2]); }

SDG_HD int classify(float avg, float smax, const Thresholds& t) {
  if (!(avg >= t.grad)) return kKeep;
  return smax > t.dense ? kSplit : kClone;
}

SDG_HD float child_scale(float s, bool is_log) { return is_log ? s - kLogSplit : s / kSplit16; }

// a candidate on its own stored values; radius = max_radii of an original, 0 for clones and children
SDG_HD bool pruned(float opacity, float smax, int32_t radius, const Thresholds& t) {
  bool out = opacity < t.opacity;
  if (t.prune_big) {
    out = out || smax > t.world;
    if (t.screen_size > 0) out = out || radius > t.screen_size;
  }
  return out;
}

// xyz + R (sigma * z): sigma_k = expf(scale_k) (the stored value when not log), the 3-term products added in index order
SDG_HD void child_xyz(const float* xyz, const float* rot, const float* scale, bool is_log, const float* z, float* out) {
  float R[9];
  quat_to_rotmat(rot, R);
  float y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = (is_log ? expf(scale[k]) : scale[k]) * z[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = xyz[r] + ((R[3 * r] * y[0] + R[3 * r + 1] * y[1]) + R[3 * r + 2] * y[2]);
}

// what one Gaussian contributes to the four candidate segments: flags[seg] = 1 when the candidate exists and survives the prune
SDG_HD int candidate_flags(float accum, int32_t denom, const float* scale, float opacity, int32_t radius, bool scale_is_log, const Thresholds& t,
                           int* flags) {
  const float smax = max3(scale);
  const int cls = classify(avg_grad(accum, denom), smax, t);
  const float cs[3] = {child_scale(scale[0], scale_is_log), child_scale(scale[1], scale_is_log), child_scale(scale[2], scale_is_log)};
  flags[0] = cls != kSplit && !pruned(opacity, smax, radius, t);
  flags[1] = cls == kClone && !pruned(opacity, smax, 0, t);
  flags[2] = flags[3] = cls == kSplit && !pruned(opacity, max3(cs), 0, t);
  return cls;
}

}  // namespace dn
}  // namespace sdg
