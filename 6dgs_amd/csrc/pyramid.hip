// pyramid.hip -- the targets of a coarse-to-fine refinement schedule below the C ABI (include/sixdgs.h: sixdgs_target_pyramid).  One
// streaming kernel, launched once per level: the centred crop, the optional compositing over the background and the d x d block mean
// of the query bytes, with the arithmetic of pyramid_rules.h -- exact integer block sums, then one stated fp32 expression.  One owner
// per output, no atomics, the same bytes on every call.
#include <math.h>

#include "common.h"
#include "pyramid_rules.h"

namespace {

using namespace sdg;

constexpr int kBlock = 256;
constexpr int kPx = 4;                        // pixel columns a thread sums down the block rows
constexpr int kRunPx = kBlock * kPx;          // pixel columns of one workgroup's strip: at least 4 output columns at d = 256
constexpr int kStage = kRunPx * 4 + 16;       // bytes of one staged input row of the strip, plus its 16-byte phase

struct PyrArgs {
  const uint8_t* in;      // [views][H][W][C]
  float* out;             // [views][h][w][3]
  int W, H, d, w, h, ox, oy;
  int ncols;              // output columns per workgroup
  float bg255[3];         // pyr::background_term of each channel
};

// A workgroup owns `cols` output pixels of one output row of one view: a strip of d input rows by cols d pixel columns, inside the
// crop.  Per input row the strip's bytes are one contiguous run.  WIDE: the run goes to LDS as it lies -- the bytes up to the first
// 16-byte boundary one by one, then 16 bytes per lane, then the bytes behind the last boundary --, so the wide part is there whatever
// the row's alignment, and nothing outside [run start, run end) is read.  Not WIDE (four channels of which the fourth is ignored): a
// lane reads the three bytes of its pixels itself, so the fourth is never touched.  Either way a thread then adds its own pixel
// columns' bytes (or products) to integer registers; after the d rows the column sums meet in LDS and one thread per output and channel
// adds d of them and evaluates the value.
template <int C, bool COMPOSITE, bool WIDE>
__global__ __launch_bounds__(kBlock) void k_target_level(PyrArgs A) {
  constexpr int NC = COMPOSITE ? 4 : 3;
  __shared__ __attribute__((aligned(16))) uint8_t stage[WIDE ? 2 : 1][WIDE ? kStage : 16];
  __shared__ uint32_t colsum[kRunPx * NC];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * A.ncols;
  const int cols = min(A.ncols, A.w - x0);
  const int y = blockIdx.y, v = blockIdx.z;
  const int np = cols * A.d;            // pixel columns of the strip, <= kRunPx
  const int run = np * C;               // bytes of the strip per input row
  uint32_t acc[kPx][NC];
#pragma unroll
  for (int j = 0; j < kPx; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[j][c] = 0u;
  for (int r = 0; r < A.d; ++r) {
    const uint8_t* p = A.in + (((size_t)v * A.H + (size_t)(A.oy + y * A.d + r)) * A.W + (size_t)(A.ox + x0 * A.d)) * C;
    const uint8_t* src = p;
    if (WIDE) {
      uint8_t* buf = stage[r & 1];
      const int shift = (int)((uintptr_t)p & 15);
      const int head = min(run, (16 - shift) & 15);
      const int nbody = (run - head) >> 4;      // <= kRunPx * 4 / 16 = kBlock
      const int tail = run - head - 16 * nbody;
      if (t < head) buf[shift + t] = p[t];
      if (t < nbody) *reinterpret_cast<uint4*>(buf + shift + head + 16 * t) = *reinterpret_cast<const uint4*>(p + head + 16 * t);
      if (t >= 64 && t - 64 < tail) buf[shift + head + 16 * nbody + (t - 64)] = p[head + 16 * nbody + (t - 64)];
      __syncthreads();      // one per row: the rows alternate between the two stages
      src = buf + shift;
    }
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      const int px = t + kBlock * j;
      if (px < np) {
        const uint8_t* q = src + px * C;
        if (COMPOSITE) {
          const uint32_t a = q[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[j][c] += (uint32_t)q[c] * a;
          acc[j][3] += 255u - a;
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[j][c] += (uint32_t)q[c];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    const int px = t + kBlock * j;
    if (px < np)
#pragma unroll
      for (int c = 0; c < NC; ++c) colsum[px * NC + c] = acc[j][c];
  }
  __syncthreads();
  float* out = A.out + (((size_t)v * A.h + (size_t)y) * A.w + (size_t)x0) * 3;
  for (int o = t; o < cols * 3; o += kBlock) {
    const int x = o / 3, c = o - 3 * x;
    const uint32_t* s = colsum + (size_t)x * A.d * NC;
    uint32_t S = 0u, S2 = 0u;
    for (int i = 0; i < A.d; ++i) {
      S += s[i * NC + c];
      if (COMPOSITE) S2 += s[i * NC + 3];
    }
    out[o] = COMPOSITE ? pyr::value_composite(S, S2, A.bg255[c], A.d) : pyr::value_plain(S, A.d);
  }
}

}  // namespace

extern "C" {

int sixdgs_target_pyramid(const uint8_t* images, int views, int height, int width, int channels, int composite, const float* h_background,
                          int levels, const int32_t* h_downscale, float* const* h_out, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(views >= 0 && views <= 65535);
  SDG_CHECK_ARG(width >= 1 && width <= pyr::kMaxSide && height >= 1 && height <= pyr::kMaxSide);
  SDG_CHECK_ARG((channels == 3 || channels == 4) && (composite == 0 || (composite == 1 && channels == 4)));
  SDG_CHECK_ARG(levels >= 1 && levels <= pyr::kMaxLevels && h_downscale && h_out);
  PyrArgs A[pyr::kMaxLevels];
  for (int l = 0; l < levels; ++l) {
    const int d = h_downscale[l];
    SDG_CHECK_ARG(d >= 1 && d <= pyr::kMaxDownscale);
    const pyr::Level g = pyr::level_geometry(width, height, d);
    SDG_CHECK_ARG(g.w >= 1 && g.h >= 1);
    A[l] = PyrArgs{images, h_out[l], width, height, d, g.w, g.h, g.ox, g.oy, kRunPx / d, {0.f, 0.f, 0.f}};
  }
  if (composite) {
    SDG_CHECK_ARG(h_background);
    for (int c = 0; c < 3; ++c) {
      SDG_CHECK_ARG(fabsf(h_background[c]) < INFINITY);
      for (int l = 0; l < levels; ++l) A[l].bg255[c] = pyr::background_term(h_background[c]);
    }
  }
  if (views == 0) return 0;
  SDG_CHECK_ARG(images);
  for (int l = 0; l < levels; ++l) SDG_CHECK_ARG(h_out[l] && ((uintptr_t)h_out[l] & 3) == 0);
  hipStream_t s = sdg_stream(stream);
  for (int l = 0; l < levels; ++l) {
    const dim3 grid((unsigned)sdg_cdiv(A[l].w, A[l].ncols), (unsigned)A[l].h, (unsigned)views);
    if (composite)
      hipLaunchKernelGGL((k_target_level<4, true, true>), grid, dim3(kBlock), 0, s, A[l]);
    else if (channels == 3)
      hipLaunchKernelGGL((k_target_level<3, false, true>), grid, dim3(kBlock), 0, s, A[l]);
    else
      hipLaunchKernelGGL((k_target_level<4, false, false>), grid, dim3(kBlock), 0, s, A[l]);
    SDG_LAUNCH_OK();
  }
  return 0;
}

}  // extern "C"
