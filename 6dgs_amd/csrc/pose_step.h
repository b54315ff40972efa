// pose_step.h -- per-view fp32 arithmetic of render-and-compare pose refinement, usable from device AND host code: compose, its
// chain rule to the 6-vector, Adam, and the best-iterate bookkeeping (include/sixdgs.h: sixdgs_pose_compose / sixdgs_pose_step define
// every operation; refine.hip runs one thread per view through step_view; hostcheck.cpp instantiates the same text for the CPU tests).
// No contraction into fused multiply-adds: every translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef SDG_HD
#define SDG_HD __host__ __device__ __forceinline__
#endif

namespace sdg {
namespace ps {

constexpr float kSeriesBelow = 1.0f;      // theta^2 < 1: the series in theta^2; otherwise sin and the half angle
constexpr int kStatusNotFinite = 1;       // bit 0 of status[v]
constexpr int kStatusCapacity = 2;        // bit 1

// a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3 from x = th^2.  The series are Horner in x with the
// coefficients (-1)^k / (2k + 1)!, (-1)^k / (2k + 2)!, (-1)^k / (2k + 3)!, k = 0 .. 5; their first dropped term is below 2e-10 of
// the value at x = 1.  Above, b = 2 sin^2(th / 2) / th^2 has no cancellation; (th - sin th) keeps at least 1/6 of th there.
struct Coeffs {
  float a, b, c;
};
SDG_HD Coeffs rot_coeffs(float x) {
  Coeffs k;
  if (x < kSeriesBelow) {
    float a = -1.f / 39916800.f, b = -1.f / 479001600.f, c = -1.f / 6227020800.f;
    a = 1.f / 362880.f + x * a;
    b = 1.f / 3628800.f + x * b;
    c = 1.f / 39916800.f + x * c;
    a = -1.f / 5040.f + x * a;
    b = -1.f / 40320.f + x * b;
    c = -1.f / 362880.f + x * c;
    a = 1.f / 120.f + x * a;
    b = 1.f / 720.f + x * b;
    c = 1.f / 5040.f + x * c;
    a = -1.f / 6.f + x * a;
    b = -1.f / 24.f + x * b;
    c = -1.f / 120.f + x * c;
    k.a = 1.f + x * a;
    k.b = 1.f / 2.f + x * b;
    k.c = 1.f / 6.f + x * c;
  } else {
    const float th = sqrtf(x), s = sinf(th), h = sinf(0.5f * th);
    k.a = s / th;
    k.b = (2.f * (h * h)) / x;
    k.c = (th - s) / (x * th);
  }
  return k;
}

SDG_HD bool finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN

// dR = (I + a K) + b K^2, K = [w]x, the 3 x 3 products as three terms added in index order
SDG_HD void delta_rotation(const float* w, const Coeffs& k, float* dR) {
  const float K[9] = {0.f, -w[2], w[1], w[2], 0.f, -w[0], -w[1], w[0], 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
      dR[3 * i + j] = ((i == j ? 1.f : 0.f) + k.a * K[3 * i + j]) + k.b * k2;
    }
}

SDG_HD float theta2(const float* w) { return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]; }

// rows = [dR R | dR t + dt | fx fy cx cy]; start and rows must not overlap
SDG_HD void compose(const float* start, const float* delta, float* rows) {
  float dR[9];
  delta_rotation(delta + 3, rot_coeffs(theta2(delta + 3)), dR);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) rows[4 * i + j] = (dR[3 * i] * start[j] + dR[3 * i + 1] * start[4 + j]) + dR[3 * i + 2] * start[8 + j];
    rows[4 * i + 3] = rows[4 * i + 3] + delta[i];
  }
#pragma unroll
  for (int j = 12; j < 16; ++j) rows[j] = start[j];
}

// g[6] = d L / d delta from G = the 3 x 4 part of d L / d rows: the exact derivative of compose
SDG_HD void chain(const float* start, const float* delta, const float* d_rows, float* g) {
  const float* w = delta + 3;
  const Coeffs k = rot_coeffs(theta2(w));
  float dR[9], A[9], M[9];
  delta_rotation(w, k, dR);
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = d_rows[4 * i + 3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      A[3 * i + r] = ((d_rows[4 * i] * start[4 * r] + d_rows[4 * i + 1] * start[4 * r + 1]) + d_rows[4 * i + 2] * start[4 * r + 2]) +
                     d_rows[4 * i + 3] * start[4 * r + 3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 3; ++r) M[3 * i + r] = (A[3 * i] * dR[3 * r] + A[3 * i + 1] * dR[3 * r + 1]) + A[3 * i + 2] * dR[3 * r + 2];
  const float tau[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
  const float k1[3] = {w[1] * tau[2] - w[2] * tau[1], w[2] * tau[0] - w[0] * tau[2], w[0] * tau[1] - w[1] * tau[0]};      // K tau
  const float k2[3] = {w[1] * k1[2] - w[2] * k1[1], w[2] * k1[0] - w[0] * k1[2], w[0] * k1[1] - w[1] * k1[0]};          // K^2 tau
#pragma unroll
  for (int i = 0; i < 3; ++i) g[3 + i] = (tau[i] - k.b * k1[i]) + k.c * k2[i];
}

struct Adam {
  float lr, beta1, beta2, eps;
  float c1, c2;      // 1 - beta1^t and sqrt(1 - beta2^t), formed in double by the host and rounded to float
};

// host: the parameters of Adam's step t = step + 1
inline Adam adam_at(int step, float lr, float beta1, float beta2, float eps) {
  const double t = (double)step + 1.0;
  return Adam{lr, beta1, beta2, eps, (float)(1.0 - pow((double)beta1, t)), (float)sqrt(1.0 - pow((double)beta2, t))};
}

// torch.optim.Adam's plain form on the six entries of one view
SDG_HD void adam(const Adam& p, const float* g, float* delta, float* m, float* v) {
  const float step = p.lr / p.c1, omb1 = 1.f - p.beta1, omb2 = 1.f - p.beta2;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    m[i] = p.beta1 * m[i] + omb1 * g[i];
    v[i] = p.beta2 * v[i] + omb2 * (g[i] * g[i]);
    delta[i] = delta[i] - step * (m[i] / (sqrtf(v[i]) / p.c2 + p.eps));
  }
}

// One view's part of step `step`: records the loss of the iterate in `rows`, keeps the first minimum, and -- unless evaluate_only or
// the view is frozen -- moves delta by one Adam step and writes the next iterate's rows.  Every pointer is the view's own slice.
// count is the instance count the rasteriser left for the whole call (0 when the caller passes none).
SDG_HD void step_view(const float* start, const float* d_rows, float loss, int64_t count, int64_t max_instances, int step, bool evaluate_only,
                      const Adam& p, float* delta, float* m, float* v, float* rows, float* best_loss, int32_t* best_step, float* best_rows,
                      float* history, int32_t* status) {
  int32_t st = *status;
  if (count > max_instances) st |= kStatusCapacity;
  if (st & kStatusCapacity) {      // the images of this step are unspecified: nothing of it is recorded, now or later
    *history = NAN;
    *status = st;
    return;
  }
  *history = loss;
  if (loss < *best_loss) {
    *best_loss = loss;
    *best_step = step;
#pragma unroll
    for (int j = 0; j < 16; ++j) best_rows[j] = rows[j];
  }
  bool ok = finite(loss);
  if (!evaluate_only) {
#pragma unroll
    for (int j = 0; j < 12; ++j) ok = ok && finite(d_rows[j]);
  }
  if (!ok) st |= kStatusNotFinite;
  *status = st;
  if (evaluate_only || (st & kStatusNotFinite)) return;
  float g[6];
  chain(start, delta, d_rows, g);
  adam(p, g, delta, m, v);
  compose(start, delta, rows);
}

}  // namespace ps
}  // namespace sdg
