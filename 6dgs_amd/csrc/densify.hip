// densify.hip -- one round of adaptive density control below the C ABI (include/sixdgs.h: sixdgs_densify): clone, split and prune a
// scene's Gaussians out of place, with Adam's m and v carried along.  The rules are densify_rules.h's.
//
//   classify  k_densify_classify  one lane per Gaussian: its class and, for each of the four candidate segments (originals not split,
//             clones, children copy 0, children copy 1), whether the candidate exists and survives the prune -> flags [4][n]; the
//             numbers of clones and split sources by a block reduction and one integer atomic add per block
//   scan      rocPRIM exclusive scan of the flags (one element more: the last offset is n_out)
//   scatter   k_densify_scatter   one lane per candidate slot: a surviving candidate writes its row of the six arrays and of m, v at
//             its scanned offset; n_out is read on the device, and with n_out > n_cap nothing is written but counts and the status bit
//
// One owner per output, no floating-point atomics, no random numbers (the caller supplies the normals): the same input gives the
// same bytes.
#include "adam_step.h"
#include "common.h"
#include "densify_rules.h"

#include <rocprim/device/device_scan.hpp>

namespace {

using namespace sdg;

constexpr int kBlock = 256;
constexpr size_t kTmpFixed = (size_t)1 << 20;      // rocPRIM's temporary storage is reserved by bound, as raster.hip does
inline size_t scan_tmp_bound(size_t items) { return sdg_align(kTmpFixed + 2 * items); }

struct Layout : SdgBump {
  size_t flags, offs, scan_tmp;
  size_t scan_tmp_bytes;
};

Layout layout(int64_t n) {
  Layout L = {};
  const size_t items = (size_t)dn::kSegments * (size_t)n + 1;
  L.flags = L.take(items * sizeof(uint32_t));
  L.offs = L.take(items * sizeof(uint32_t));
  L.scan_tmp_bytes = scan_tmp_bound(items);
  L.scan_tmp = L.take(L.scan_tmp_bytes);
  return L;
}

struct Args {
  const float* p[ga::kGroups];      // xyz, f_dc, f_rest, opacity, scale, rot
  float* p_out[ga::kGroups];
  const float *m, *v, *grad_accum, *noise;
  float *m_out, *v_out;
  const int32_t *denom, *max_radii;
  uint32_t *flags, *offs;
  int64_t* counts;
  int32_t* status;
  int64_t n, n_cap;
  int n_coef, scale_is_log;
  dn::Thresholds t;
};

__global__ __launch_bounds__(kBlock) void k_densify_classify(Args A) {
  __shared__ unsigned s_clone[kBlock / 64], s_split[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int cls = dn::kKeep;
  if (i < A.n) {
    const float* sc = A.p[4] + 3 * i;
    const float s[3] = {sc[0], sc[1], sc[2]};
    int f[dn::kSegments];
    cls = dn::candidate_flags(A.grad_accum[i], A.denom[i], s, A.p[3][i], A.max_radii[i], A.scale_is_log != 0, A.t, f);
#pragma unroll
    for (int g = 0; g < dn::kSegments; ++g) A.flags[(int64_t)g * A.n + i] = (uint32_t)f[g];
    if (i == 0) A.flags[(int64_t)dn::kSegments * A.n] = 0u;
  }
  const unsigned clones = sdg_wave_sum<unsigned>(cls == dn::kClone), splits = sdg_wave_sum<unsigned>(cls == dn::kSplit);
  if (sdg_lane() == 0) {
    s_clone[sdg_wave()] = clones;
    s_split[sdg_wave()] = splits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0, s = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      c += s_clone[w];
      s += s_split[w];
    }
    if (c) atomicAdd((unsigned long long*)(A.counts + 1), (unsigned long long)c);
    if (s) atomicAdd((unsigned long long*)(A.counts + 2), (unsigned long long)s);
  }
}

__global__ __launch_bounds__(kBlock) void k_densify_scatter(Args A) {
  const int64_t slots = (int64_t)dn::kSegments * A.n;
  const int64_t n_out = (int64_t)A.offs[slots];
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool over = n_out > A.n_cap;
  if (s == 0) {
    A.counts[0] = n_out;
    A.counts[3] = (A.n + A.counts[1] + A.counts[2]) - n_out;
    if (over) atomicOr(A.status, ga::kStatusCapacity);
  }
  if (over || s >= slots || !A.flags[s]) return;
  const int seg = (int)(s / A.n);
  const int64_t i = s - (int64_t)seg * A.n, d = (int64_t)A.offs[s];
  int64_t cum = 0;                   // floats per Gaussian of the groups before k: the slices of m and v start at n cum and n_out cum
#pragma unroll
  for (int k = 0; k < ga::kGroups; ++k) {
    const int w = ga::group_width(k, A.n_coef);
    const float* __restrict__ src = A.p[k] + i * w;
    float* __restrict__ dst = A.p_out[k] + d * w;
    if (seg >= 2 && k == 0) {
      dn::child_xyz(src, A.p[5] + 4 * i, A.p[4] + 3 * i, A.scale_is_log != 0, A.noise + (i * 2 + (seg - 2)) * 3, dst);
    } else if (seg >= 2 && k == 4) {
      for (int j = 0; j < 3; ++j) dst[j] = dn::child_scale(src[j], A.scale_is_log != 0);
    } else {
      for (int j = 0; j < w; ++j) dst[j] = src[j];
    }
    float* __restrict__ mo = A.m_out + n_out * cum + d * w;
    float* __restrict__ vo = A.v_out + n_out * cum + d * w;
    if (seg == 0) {                  // a surviving original keeps its rows of m and v
      const float* __restrict__ mi = A.m + A.n * cum + i * w;
      const float* __restrict__ vi = A.v + A.n * cum + i * w;
      for (int j = 0; j < w; ++j) {
        mo[j] = mi[j];
        vo[j] = vi[j];
      }
    } else {
      for (int j = 0; j < w; ++j) {
        mo[j] = 0.f;
        vo[j] = 0.f;
      }
    }
    cum += w;
  }
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" {

size_t sixdgs_densify_workspace_bytes(int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
  return layout(n).total;
}

int sixdgs_densify(int64_t n, int n_coef, const float* xyz, const float* f_dc, const float* f_rest, const float* opacity, const float* scale,
                   const float* rot, int scale_is_log, int opacity_is_logit, const float* m, const float* v, const float* grad_accum,
                   const int32_t* denom, const int32_t* max_radii, const float* noise, float grad_threshold, float percent_dense, float extent,
                   float min_opacity, int prune_big, int screen_size, int64_t n_cap, float* xyz_out, float* f_dc_out, float* f_rest_out,
                   float* opacity_out, float* scale_out, float* rot_out, float* m_out, float* v_out, int64_t* counts, int32_t* status, void* ws,
                   size_t ws_bytes, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) && n_coef >= 1 && n_coef <= 16 && n_cap >= 0 && n_cap < ((int64_t)1 << 31));
  SDG_CHECK_ARG((scale_is_log == 0 || scale_is_log == 1) && (opacity_is_logit == 0 || opacity_is_logit == 1));
  SDG_CHECK_ARG(grad_threshold > 0.f && grad_threshold < INFINITY);
  SDG_CHECK_ARG(percent_dense > 0.f && percent_dense < INFINITY && extent > 0.f && extent < INFINITY);
  SDG_CHECK_ARG(min_opacity >= 0.f && min_opacity < 1.f && screen_size >= 0);
  SDG_CHECK_ARG(counts && status && ((uintptr_t)counts & 7) == 0 && aligned4(status));
  hipStream_t s = sdg_stream(stream);
  if (n == 0) {
    hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s);
    return e == hipSuccess ? 0 : (int)e;
  }
  Args A = {};
  const float* const p[ga::kGroups] = {xyz, f_dc, f_rest, opacity, scale, rot};
  float* const p_out[ga::kGroups] = {xyz_out, f_dc_out, f_rest_out, opacity_out, scale_out, rot_out};
  for (int k = 0; k < ga::kGroups; ++k) {
    if (ga::group_width(k, n_coef) > 0) {
      SDG_CHECK_ARG(p[k] && aligned4(p[k]) && aligned4(p_out[k]) && p[k] != p_out[k] && (n_cap == 0 || p_out[k]));
      A.p[k] = p[k];
      A.p_out[k] = p_out[k];
    }
  }
  SDG_CHECK_ARG(m && v && grad_accum && denom && max_radii && noise && (n_cap == 0 || (m_out && v_out && m_out != v_out)));
  SDG_CHECK_ARG(m != m_out && v != v_out && m != v_out && v != m_out);
  SDG_CHECK_ARG(aligned4(m) && aligned4(v) && aligned4(grad_accum) && aligned4(denom) && aligned4(max_radii) && aligned4(noise) && aligned4(m_out) &&
                aligned4(v_out));
  const Layout L = layout(n);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  char* w = (char*)ws;
  A.m = m; A.v = v; A.grad_accum = grad_accum; A.noise = noise;
  A.m_out = m_out; A.v_out = v_out;
  A.denom = denom; A.max_radii = max_radii;
  A.flags = (uint32_t*)(w + L.flags);
  A.offs = (uint32_t*)(w + L.offs);
  A.counts = counts;
  A.status = status;
  A.n = n; A.n_cap = n_cap;
  A.n_coef = n_coef; A.scale_is_log = scale_is_log;
  A.t = dn::thresholds(grad_threshold, percent_dense, extent, min_opacity, scale_is_log, opacity_is_logit, prune_big != 0, screen_size);
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_densify_classify, dim3((unsigned)sdg_cdiv(n, kBlock)), dim3(kBlock), 0, s, A);
  SDG_LAUNCH_OK();
  const size_t items = (size_t)dn::kSegments * (size_t)n + 1;
  size_t need = 0;
  e = rocprim::exclusive_scan((void*)nullptr, need, A.flags, A.offs, (uint32_t)0, items, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return (int)e;
  if (need > L.scan_tmp_bytes) return SIXDGS_E_WORKSPACE;
  need = L.scan_tmp_bytes;
  e = rocprim::exclusive_scan((void*)(w + L.scan_tmp), need, A.flags, A.offs, (uint32_t)0, items, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_densify_scatter, dim3((unsigned)sdg_cdiv((int64_t)items - 1, kBlock)), dim3(kBlock), 0, s, A);
  SDG_LAUNCH_OK();
  return 0;
}

}  // extern "C"
