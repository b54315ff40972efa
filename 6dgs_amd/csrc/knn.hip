// knn.hip -- the mean squared distance of every point to its three nearest other points, below the C ABI (include/sixdgs.h:
// sixdgs_knn_mean_dist2): the isotropic start scale of a scene made from a point cloud.  The rules are knn_rules.h's; the result is
// the one a brute force over all pairs gives, to the bit, because the box distance that prunes is a lower bound in fp32 itself.
//
//   bbox     k_knn_bbox_partial  grid-stride min / max per block -> partial [blocks][6];  k_knn_bbox_final  one block -> bbox [6]
//   codes    k_knn_codes         one lane per point: its 30-bit Morton code inside the bounding box (a sort key) and its index
//   sort     rocPRIM radix_sort_pairs of (code, index)
//   gather   k_knn_gather        one workgroup per box of kBox consecutive sorted points: the points into three SoA planes (padded
//                                with +inf to whole boxes, so a pad is never among the nearest) and the box's AABB -> boxes [nb][8]
//   search   k_knn_search        one workgroup per box, one lane per query, every wave on its own: the own box first, then the
//                                other boxes outward in Morton order.  A box is skipped for the whole wave when its distance to the
//                                AABB of the wave's queries is >= the wave's largest third-best value; otherwise the lanes whose own
//                                box distance is below their third-best value walk its points.  Box table and candidates are read
//                                at wave-uniform addresses from read-only memory, so they arrive through the scalar cache and
//                                feed the vector ALU as scalar operands: no LDS, no barrier, nothing derived from a coordinate
//                                is an index, every loop is bounded by the box count or kBox.
//
// One owner per output, no atomics, no host read: the same bytes on every call.
#include "common.h"
#include "knn_rules.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

using namespace sdg;

constexpr int kBlock = kn::kBox;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPartial = 1024;
constexpr int kBoxRow = 8;                         // floats per row of the box table: lo xyz, hi xyz, two pads
constexpr size_t kTmpFixed = (size_t)1 << 20;      // rocPRIM's temporary storage is reserved by bound, as raster.hip does
inline size_t sort_tmp_bound(size_t items) { return sdg_align(kTmpFixed + 16 * items); }

struct Layout : SdgBump {
  size_t partial, bbox, keys0, keys1, vals0, vals1, sort_tmp, sx, sy, sz, boxes;
  size_t sort_tmp_bytes;
  int64_t nb;
};

Layout layout(int64_t n) {
  Layout L = {};
  L.nb = sdg_cdiv(n, kBlock);
  const size_t padded = (size_t)L.nb * kBlock;
  L.partial = L.take((size_t)kMaxPartial * 6 * sizeof(float));
  L.bbox = L.take(8 * sizeof(float));
  L.keys0 = L.take((size_t)n * sizeof(uint32_t));
  L.keys1 = L.take((size_t)n * sizeof(uint32_t));
  L.vals0 = L.take((size_t)n * sizeof(uint32_t));
  L.vals1 = L.take((size_t)n * sizeof(uint32_t));
  L.sort_tmp_bytes = sort_tmp_bound((size_t)n);
  L.sort_tmp = L.take(L.sort_tmp_bytes);
  L.sx = L.take(padded * sizeof(float));
  L.sy = L.take(padded * sizeof(float));
  L.sz = L.take(padded * sizeof(float));
  L.boxes = L.take((size_t)L.nb * kBoxRow * sizeof(float));
  return L;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// min / max of six running values over the block -> out[0..2] = lo, out[3..5] = hi (lane 0 writes)
__device__ __forceinline__ void block_minmax(float* lo, float* hi, float* out) {
  __shared__ float s[kWaves][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min(lo[a]);
    hi[a] = sdg_wave_max(hi[a]);
  }
  if (sdg_lane() == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[sdg_wave()][a] = lo[a];
      s[sdg_wave()][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float l = s[0][a], h = s[0][3 + a];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        l = fminf(l, s[w][a]);
        h = fmaxf(h, s[w][3 + a]);
      }
      out[a] = l;
      out[3 + a] = h;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_knn_bbox_partial(const float* __restrict__ xyz, int64_t n, float* __restrict__ partial) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float c = xyz[3 * i + a];
      lo[a] = fminf(lo[a], c);
      hi[a] = fmaxf(hi[a], c);
    }
  }
  block_minmax(lo, hi, partial + 6 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_knn_bbox_final(const float* __restrict__ partial, int blocks, float* __restrict__ bbox) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < blocks; b += kBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], partial[6 * b + a]);
      hi[a] = fmaxf(hi[a], partial[6 * b + 3 + a]);
    }
  }
  block_minmax(lo, hi, bbox);
}

__global__ __launch_bounds__(kBlock) void k_knn_codes(const float* __restrict__ xyz, int64_t n, const float* __restrict__ bbox,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const float lo[3] = {bbox[0], bbox[1], bbox[2]}, hi[3] = {bbox[3], bbox[4], bbox[5]};
  keys[i] = kn::morton(p, lo, hi);
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_knn_gather(const float* __restrict__ xyz, int64_t n, const uint32_t* __restrict__ order,
                                                       float* __restrict__ sx, float* __restrict__ sy, float* __restrict__ sz,
                                                       float* __restrict__ boxes) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // < nb kBox: inside the padded planes
  float p[3] = {INFINITY, INFINITY, INFINITY};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (s < n) {
    const int64_t i = (int64_t)order[s];                             // a permutation of [0, n): written by k_knn_codes, moved by the sort
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = lo[a] = hi[a] = xyz[3 * i + a];
  }
  sx[s] = p[0];
  sy[s] = p[1];
  sz[s] = p[2];
  block_minmax(lo, hi, boxes + (int64_t)kBoxRow * blockIdx.x);
}

// One box of candidates against the lane's query.  base is wave-uniform, so the three planes are read through the scalar cache.
template <bool kOwn>
__device__ __forceinline__ void walk_box(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int64_t base,
                                         int self, float qx, float qy, float qz, float& b0, float& b1, float& b2) {
#pragma unroll 16
  for (int j = 0; j < kBlock; ++j) {
    float d = kn::pair_d2(qx, qy, qz, sx[base + j], sy[base + j], sz[base + j]);
    if (kOwn) d = j == self ? INFINITY : d;      // distinct by index, not by position
    kn::insert3(d, b0, b1, b2);
  }
}

__global__ __launch_bounds__(kBlock) void k_knn_search(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                                                       const float* __restrict__ boxes, const uint32_t* __restrict__ order, int64_t n,
                                                       int nb, float* __restrict__ mean_d2) {
  const int own = (int)blockIdx.x;
  const int64_t s = (int64_t)own * kBlock + threadIdx.x;
  const bool valid = s < n;
  if (!__any(valid)) return;                     // a wave of the last box without a query (no barrier in this kernel)
  const float qx = sx[s], qy = sy[s], qz = sz[s];      // a pad (+inf) on a lane without a query
  // the AABB of the wave's queries; a lane without a query is the identity of min and max
  float wlo[3] = {wave_min(qx), wave_min(qy), wave_min(qz)};
  float whi[3] = {sdg_wave_max(valid ? qx : -INFINITY), sdg_wave_max(valid ? qy : -INFINITY), sdg_wave_max(valid ? qz : -INFINITY)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wlo[a] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wlo[a])));
    whi[a] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, whi[a])));
  }
  // a lane without a query holds -inf: it never passes a box test and never raises the wave's maximum
  float b0 = valid ? INFINITY : -INFINITY, b1 = b0, b2 = b0;
  if (valid) walk_box<true>(sx, sy, sz, (int64_t)own * kBlock, (int)threadIdx.x, qx, qy, qz, b0, b1, b2);
  float wmax = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sdg_wave_max(b2))));
  const int reach = own > nb - 1 - own ? own : nb - 1 - own;
  for (int step = 1; step <= reach; ++step) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int c = side ? own + step : own - step;
      if (c < 0 || c >= nb) continue;
      const float* box = boxes + (int64_t)kBoxRow * c;
      const float lo[3] = {box[0], box[1], box[2]}, hi[3] = {box[3], box[4], box[5]};
      if (kn::box_box_d2(wlo, whi, lo, hi) >= wmax) continue;      // can at most tie a third-best value: changes none
      if (valid && kn::box_d2(qx, qy, qz, lo, hi) < b2) walk_box<false>(sx, sy, sz, (int64_t)c * kBlock, 0, qx, qy, qz, b0, b1, b2);
      wmax = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sdg_wave_max(b2))));
    }
  }
  if (valid) mean_d2[order[s]] = kn::mean3(b0, b1, b2);
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" {

size_t sixdgs_knn_workspace_bytes(int64_t n) {
  if (n < 4 || n >= ((int64_t)1 << 31)) return 0;
  return layout(n).total;
}

int sixdgs_knn_mean_dist2(int64_t n, const float* xyz, float* mean_d2, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  if (n == 0) return 0;
  SDG_CHECK_ARG(n >= 4 && n < ((int64_t)1 << 31));
  SDG_CHECK_ARG(xyz && mean_d2 && aligned4(xyz) && aligned4(mean_d2));
  {
    const uintptr_t a = (uintptr_t)xyz, b = (uintptr_t)mean_d2;
    SDG_CHECK_ARG(a + 12 * (uintptr_t)n <= b || b + 4 * (uintptr_t)n <= a);
  }
  const Layout L = layout(n);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  float* partial = (float*)(w + L.partial);
  float* bbox = (float*)(w + L.bbox);
  float *sx = (float*)(w + L.sx), *sy = (float*)(w + L.sy), *sz = (float*)(w + L.sz), *boxes = (float*)(w + L.boxes);
  const int64_t nb = L.nb;
  const int blocks = (int)(nb < kMaxPartial ? nb : kMaxPartial);
  hipLaunchKernelGGL(k_knn_bbox_partial, dim3((unsigned)blocks), dim3(kBlock), 0, s, xyz, n, partial);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_knn_bbox_final, dim3(1), dim3(kBlock), 0, s, (const float*)partial, blocks, bbox);
  SDG_LAUNCH_OK();
  rocprim::double_buffer<uint32_t> keys((uint32_t*)(w + L.keys0), (uint32_t*)(w + L.keys1));
  rocprim::double_buffer<uint32_t> vals((uint32_t*)(w + L.vals0), (uint32_t*)(w + L.vals1));
  hipLaunchKernelGGL(k_knn_codes, dim3((unsigned)nb), dim3(kBlock), 0, s, xyz, n, (const float*)bbox, keys.current(), vals.current());
  SDG_LAUNCH_OK();
  size_t need = 0;
  hipError_t e = rocprim::radix_sort_pairs((void*)nullptr, need, keys, vals, (size_t)n, 0u, 30u, s);
  if (e != hipSuccess) return (int)e;
  if (need > L.sort_tmp_bytes) return SIXDGS_E_WORKSPACE;
  need = L.sort_tmp_bytes;
  e = rocprim::radix_sort_pairs((void*)(w + L.sort_tmp), need, keys, vals, (size_t)n, 0u, 30u, s);
  if (e != hipSuccess) return (int)e;
  const uint32_t* order = vals.current();
  hipLaunchKernelGGL(k_knn_gather, dim3((unsigned)nb), dim3(kBlock), 0, s, xyz, n, order, sx, sy, sz, boxes);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_knn_search, dim3((unsigned)nb), dim3(kBlock), 0, s, (const float*)sx, (const float*)sy, (const float*)sz,
                     (const float*)boxes, order, n, (int)nb, mean_d2);
  SDG_LAUNCH_OK();
  return 0;
}

}  // extern "C"
