// adam_step.h -- per-entry fp32 arithmetic of fitting a scene's Gaussians, usable from device AND host code: one entry of Adam over a
// parameter group and one entry of the opacity reset (include/sixdgs.h: sixdgs_gaussian_adam / sixdgs_opacity_reset define every
// operation; fit.hip streams the groups through these; hostcheck.cpp instantiates the same text for the CPU tests).  The formula and
// the host-made constants are pose_step.h's (ps::Adam, ps::adam_at).  No contraction into fused multiply-adds: every translation unit
// that includes this is built with -ffp-contract=off.
#pragma once
#include "pose_step.h"

namespace sdg {
namespace ga {

constexpr int kGroups = 6;      // xyz, f_dc, f_rest, opacity, scale, rot -- this order everywhere
constexpr int kStatusNotFinite = ps::kStatusNotFinite, kStatusCapacity = ps::kStatusCapacity;

// floats per Gaussian of group k
SDG_HD int group_width(int k, int n_coef) {
  return k == 0 ? 3 : k == 1 ? 3 : k == 2 ? 3 * (n_coef - 1) : k == 3 ? 1 : k == 4 ? 3 : 4;
}

// what one step shares between the entries of a group: ps::Adam with the group's rate folded into the step size
struct Rate {
  float step, beta1, omb1, beta2, omb2, c2, eps;
};
SDG_HD Rate rate(const ps::Adam& p, float lr) { return Rate{lr / p.c1, p.beta1, 1.f - p.beta1, p.beta2, 1.f - p.beta2, p.c2, p.eps}; }

// One entry.  false (and nothing written) when g is not finite.
SDG_HD bool adam_entry(const Rate& r, float g, float& p, float& m, float& v) {
  if (!ps::finite(g)) return false;
  m = r.beta1 * m + r.omb1 * g;
  v = r.beta2 * v + r.omb2 * (g * g);
  p = p - r.step * (m / (sqrtf(v) / r.c2 + r.eps));
  return true;
}

// One opacity: o = min(a, ceiling), a = sigmoid(x) in logit form and x itself otherwise; stored back in the form it came in
SDG_HD float reset_entry(float x, bool is_logit, float ceiling) {
  const float a = is_logit ? 1.f / (1.f + expf(-x)) : x;
  const float o = fminf(a, ceiling);
  return is_logit ? logf(o / (1.f - o)) : o;
}

}  // namespace ga
}  // namespace sdg
