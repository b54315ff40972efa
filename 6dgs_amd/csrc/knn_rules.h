// knn_rules.h -- the per-pair and per-box rules of the exact 3-nearest-neighbour search, usable from device AND host code
// (include/sixdgs.h: sixdgs_knn_mean_dist2 defines every operation; knn.hip runs them one lane per query; hostcheck.cpp instantiates
// the same text for the CPU tests).  Every fp32 operation here is monotone in its operands, which is what makes the box distance a
// lower bound of the pair distance IN fp32 and the pruning exact.  No contraction into fused multiply-adds: every translation unit
// that includes this is built with -ffp-contract=off.
#pragma once
#include "device_math.h"

namespace sdg {
namespace kn {

constexpr int kBox = 256;           // points per box = lanes per workgroup of the search
constexpr int kCells = 1024;        // Morton cells per axis (10 bits)

// d2(i, j): the differences first, then (dx dx + dy dy) + dz dz
SDG_HD float pair_d2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// the cell of coordinate c on an axis of the bounding box [lo, hi]: 0 on an axis of zero extent, clamped to [0, 1023] otherwise (a NaN
// lands in cell 0).  A sort key only: never an index.
SDG_HD uint32_t axis_cell(float c, float lo, float hi) {
  if (!(hi > lo)) return 0u;
  const float t = (c - lo) / (hi - lo) * (float)(kCells - 1);
  if (!(t > 0.f)) return 0u;
  return t >= (float)(kCells - 1) ? (uint32_t)(kCells - 1) : (uint32_t)t;
}

// 10 bits -> every third bit of 30
SDG_HD uint32_t spread3(uint32_t v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

SDG_HD uint32_t morton(const float* p, const float* lo, const float* hi) {
  return (spread3(axis_cell(p[0], lo[0], hi[0])) << 2) | (spread3(axis_cell(p[1], lo[1], hi[1])) << 1) | spread3(axis_cell(p[2], lo[2], hi[2]));
}

// one axis of the distance between the intervals [qlo, qhi] and [lo, hi]; with qlo == qhi == q it is q < lo ? lo - q : (q > hi ? q - hi : 0)
SDG_HD float axis_gap(float qlo, float qhi, float lo, float hi) { return qhi < lo ? lo - qhi : (qlo > hi ? qlo - hi : 0.f); }

// squared distance from the point q to the box [lo, hi], summed in d2's order: <= d2(q, p) for every p inside the box, in fp32 itself
SDG_HD float box_d2(float qx, float qy, float qz, const float* lo, const float* hi) {
  const float dx = axis_gap(qx, qx, lo[0], hi[0]), dy = axis_gap(qy, qy, lo[1], hi[1]), dz = axis_gap(qz, qz, lo[2], hi[2]);
  return (dx * dx + dy * dy) + dz * dz;
}

// the same between two boxes: <= box_d2(q, .) for every q inside [qlo, qhi]
SDG_HD float box_box_d2(const float* qlo, const float* qhi, const float* lo, const float* hi) {
  const float dx = axis_gap(qlo[0], qhi[0], lo[0], hi[0]), dy = axis_gap(qlo[1], qhi[1], lo[1], hi[1]), dz = axis_gap(qlo[2], qhi[2], lo[2], hi[2]);
  return (dx * dx + dy * dy) + dz * dz;
}

// the three smallest values seen so far, b0 <= b1 <= b2 (start at +inf); d is never a NaN under the call's precondition
SDG_HD void insert3(float d, float& b0, float& b1, float& b2) {
  b2 = fminf(b2, fmaxf(b1, d));
  b1 = fminf(b1, fmaxf(b0, d));
  b0 = fminf(b0, d);
}

SDG_HD float mean3(float b0, float b1, float b2) { return ((b0 + b1) + b2) / 3.0f; }

}  // namespace kn
}  // namespace sdg
