// fit.hip -- fitting a scene's Gaussians to posed views below the C ABI (include/sixdgs.h: sixdgs_gaussian_adam,
// sixdgs_opacity_reset, sixdgs_fit_scene, sixdgs_fit_scene_steps).  The arithmetic is adam_step.h's, one owner per output, no
// floating-point atomics; the loop enqueues the rasteriser, the photometric loss, the rasteriser's backward, the densification
// statistics where asked for, the Adam step and the opacity reset on one stream through their own entry points and never reads anything
// back.  The number of Gaussians is fixed within a call; a fit that densifies is cut into sixdgs_fit_scene_steps calls around
// sixdgs_densify (densify.hip).
#include <math.h>

#include "adam_step.h"
#include "render_pass.h"

namespace {

using namespace sdg;
using namespace rp;

constexpr int kBlock = 256;
constexpr int kVec = 4;                      // floats per 16-byte access
constexpr int kChunk = kBlock * kVec;        // entries a workgroup takes at a time
constexpr int kMaxBlocks = 2048;             // 256 CUs x 8 workgroups; the rest of the chunks by grid stride

// One parameter group of the step.  count = 0: frozen, it owns no chunk.
struct Group {
  float* p;
  const float* g;
  float *m, *v;
  int64_t count;          // entries
  int64_t chunk_end;      // this group's chunks are [the previous group's chunk_end, chunk_end) of the flat chunk index
  ga::Rate rate;
  int vec;                // p, g, m and v are all 16-byte aligned
};

struct AdamArgs {
  Group grp[ga::kGroups];
  int64_t chunks;
  const int64_t* instances;
  int64_t max_instances;
  int32_t* status;
};

// All six groups in one launch: a workgroup walks the flat chunk index by grid stride, finds the chunk's group in the table (uniform
// per workgroup) and streams kChunk entries: p, g, m, v in, p, m, v out.  16-byte accesses where the group's pointers allow them and
// the four entries lie inside the group, 4-byte accesses otherwise -- the arithmetic is per entry, so the bits are the same.
__global__ __launch_bounds__(kBlock) void k_gaussian_adam(AdamArgs A) {
  const int32_t st = *A.status;
  const bool over = A.instances && *A.instances > A.max_instances;
  if (over && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(A.status, ga::kStatusCapacity);
  if (over || (st & ga::kStatusCapacity)) return;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < A.chunks; c += gridDim.x) {
    Group G = A.grp[0];
    int64_t first = 0;
#pragma unroll
    for (int k = 1; k < ga::kGroups; ++k)
      if (c >= A.grp[k - 1].chunk_end) {
        G = A.grp[k];
        first = A.grp[k - 1].chunk_end;
      }
    const int64_t base = (c - first) * kChunk;
    const int64_t i4 = base + (int64_t)threadIdx.x * kVec;
    if (G.vec && i4 + kVec <= G.count) {
      float4 p = *reinterpret_cast<const float4*>(G.p + i4);
      const float4 g = *reinterpret_cast<const float4*>(G.g + i4);
      float4 m = *reinterpret_cast<const float4*>(G.m + i4);
      float4 v = *reinterpret_cast<const float4*>(G.v + i4);
      bad |= !ga::adam_entry(G.rate, g.x, p.x, m.x, v.x);
      bad |= !ga::adam_entry(G.rate, g.y, p.y, m.y, v.y);
      bad |= !ga::adam_entry(G.rate, g.z, p.z, m.z, v.z);
      bad |= !ga::adam_entry(G.rate, g.w, p.w, m.w, v.w);
      *reinterpret_cast<float4*>(G.p + i4) = p;
      *reinterpret_cast<float4*>(G.m + i4) = m;
      *reinterpret_cast<float4*>(G.v + i4) = v;
    } else if (G.vec) {      // the group's last, partial quad
      for (int64_t i = i4; i < G.count; ++i) {
        float p = G.p[i], m = G.m[i], v = G.v[i];
        if (ga::adam_entry(G.rate, G.g[i], p, m, v)) {
          G.p[i] = p;
          G.m[i] = m;
          G.v[i] = v;
        } else {
          bad = true;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const int64_t i = base + (int64_t)j * kBlock + threadIdx.x;
        if (i < G.count) {
          float p = G.p[i], m = G.m[i], v = G.v[i];
          if (ga::adam_entry(G.rate, G.g[i], p, m, v)) {
            G.p[i] = p;
            G.m[i] = m;
            G.v[i] = v;
          } else {
            bad = true;
          }
        }
      }
    }
  }
  if (bad) atomicOr(A.status, ga::kStatusNotFinite);
}

// status (may be NULL): the reset is skipped once bit 1 is set
__global__ __launch_bounds__(kBlock) void k_opacity_reset(float* __restrict__ opacity, int64_t n, int is_logit, float* __restrict__ m,
                                                          float* __restrict__ v, float ceiling, const int32_t* status) {
  if (status && (*status & ga::kStatusCapacity)) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  opacity[i] = ga::reset_entry(opacity[i], is_logit != 0, ceiling);
  if (m) m[i] = 0.f;
  if (v) v[i] = 0.f;
}

// history row of one step of sixdgs_fit_scene: the batch's losses, or NaN from the step that overflowed on; thread 0 keeps the
// largest count and sets bit 1, which the Adam step and the reset behind it read on entry
__global__ __launch_bounds__(64) void k_fit_record(const float* __restrict__ loss, int batch, const int64_t* count, int64_t max_instances,
                                                   float* __restrict__ history_row, int32_t* status, int64_t* instances_needed) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int64_t cnt = *count;
  const bool over = cnt > max_instances || (*status & ga::kStatusCapacity);
  if (b == 0) {
    if (cnt > *instances_needed) *instances_needed = cnt;
    if (cnt > max_instances) atomicOr(status, ga::kStatusCapacity);
  }
  if (b < batch) history_row[b] = over ? NAN : loss[b];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool lr_ok(const float* lr) {
  if (!lr) return false;
  for (int k = 0; k < ga::kGroups; ++k)
    if (!(lr[k] >= 0.f && lr[k] < INFINITY)) return false;
  return true;
}
bool sizes_ok(int64_t n, int n_coef, int64_t max_instances) {
  return n >= 0 && n < ((int64_t)1 << 31) && n_coef >= 1 && n_coef <= 16 && max_instances >= 1 && max_instances < ((int64_t)1 << 31);
}

int64_t state_floats(int64_t n, int n_coef) { return n * (11 + 3 * (int64_t)n_coef); }

int launch_reset(float* opacity, int64_t n, int is_logit, float* m, float* v, float ceiling, const int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_opacity_reset, dim3((unsigned)sdg_cdiv(n, kBlock)), dim3(kBlock), 0, s, opacity, n, is_logit, m, v, ceiling, status);
  SDG_LAUNCH_OK();
  return 0;
}

struct Layout : PassLayout {
  size_t target, g[ga::kGroups], radii;
};

// 0 total = outside the limits.  with_radii: sixdgs_fit_scene_steps' workspace, which ends with the radii [batch][n] of a step's render
Layout layout(int64_t n, int n_coef, int batch, int width, int height, int64_t max_instances, bool with_radii = false) {
  Layout L = {};
  if (n_coef < 1 || n_coef > 16 || batch < 1 || !pass_layout(L, n, batch, width, height, max_instances)) return L;
  L.target = L.take((size_t)batch * (size_t)height * (size_t)width * 4 * sizeof(float));      // the widest of the three target forms
  for (int k = 0; k < ga::kGroups; ++k) L.g[k] = L.take((size_t)n * ga::group_width(k, n_coef) * sizeof(float));
  if (with_radii) L.radii = L.take((size_t)batch * (size_t)n * sizeof(int32_t));
  return L;
}

// what sixdgs_fit_scene and sixdgs_fit_scene_steps share: the arguments as the former takes them, and the latter's additions
struct Fit {
  float *xyz, *scale, *rot, *opacity, *f_dc, *f_rest;
  int scale_is_log, opacity_is_logit, n_coef;
  int64_t n;
  const float* cams;
  int views, width, height;
  float scale_modifier;
  const float* background;
  const void* target;
  int target_is_u8, target_stride;
  float lambda;
  int steps, batch;
  const int32_t* h_view;
  const float* h_lr;
  const int32_t* h_sh_degree;
  const uint8_t *h_reset, *h_update, *h_stats;      // h_update NULL: every step updates; h_stats NULL: no statistics
  int first_adam_step, group_mask;
  float beta1, beta2, eps, reset_ceiling;
  int64_t max_instances;
  float *m, *v, *history;
  int32_t* status;
  int64_t* instances_needed;
  float* grad_accum;
  int32_t *denom, *max_radii;
  void* ws;
  size_t ws_bytes;
  sixdgs_stream_t stream;
};

// the checks and the loop body; zero_state: m, v, status and instances_needed start from zero (sixdgs_fit_scene)
int fit_steps(const Fit& F, bool zero_state) {
  float *const xyz = F.xyz, *const scale = F.scale, *const rot = F.rot, *const opacity = F.opacity, *const f_dc = F.f_dc, *const f_rest = F.f_rest;
  const int scale_is_log = F.scale_is_log, opacity_is_logit = F.opacity_is_logit, n_coef = F.n_coef, views = F.views, width = F.width,
            height = F.height, target_is_u8 = F.target_is_u8, target_stride = F.target_stride, steps = F.steps, batch = F.batch,
            group_mask = F.group_mask;
  const int64_t n = F.n, max_instances = F.max_instances;
  const float *const cams = F.cams, *const background = F.background, *const h_lr = F.h_lr;
  const float scale_modifier = F.scale_modifier, lambda = F.lambda, beta1 = F.beta1, beta2 = F.beta2, eps = F.eps, reset_ceiling = F.reset_ceiling;
  const void* const target = F.target;
  const int32_t *const h_view = F.h_view, *const h_sh_degree = F.h_sh_degree;
  const uint8_t* const h_reset = F.h_reset;
  float *const m = F.m, *const v = F.v, *const history = F.history;
  int32_t* const status = F.status;
  int64_t* const instances_needed = F.instances_needed;
  void* const ws = F.ws;
  const size_t ws_bytes = F.ws_bytes;
  sixdgs_stream_t stream = F.stream;
  const Layout L = layout(n, n_coef, batch, width, height, max_instances, !zero_state);
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  Target T = {target, target_is_u8, target_stride};
  SDG_CHECK_ARG(L.total != 0);
  SDG_CHECK_ARG(views >= 1 && views <= kMaxViews);
  SDG_CHECK_ARG((scale_is_log == 0 || scale_is_log == 1) && (opacity_is_logit == 0 || opacity_is_logit == 1));
  SDG_CHECK_ARG(target_ok(T) && loop_ok(lambda, steps));
  SDG_CHECK_ARG(group_mask > 0 && group_mask < (1 << ga::kGroups));
  SDG_CHECK_ARG(hyper_ok(beta1, beta2, eps));
  SDG_CHECK_ARG(reset_ceiling > 0.f && reset_ceiling < 1.f);
  SDG_CHECK_ARG(h_view && h_lr && h_sh_degree && h_reset);
  for (int s = 0; s < steps; ++s) {
    for (int b = 0; b < batch; ++b) SDG_CHECK_ARG(h_view[(size_t)s * batch + b] >= 0 && h_view[(size_t)s * batch + b] < views);
    SDG_CHECK_ARG(lr_ok(h_lr + (size_t)s * ga::kGroups));
    SDG_CHECK_ARG(scene_ok(S, h_sh_degree[s]));
    SDG_CHECK_ARG(h_reset[s] == 0 || opacity_is_logit);
  }
  SDG_CHECK_ARG(cams && scene_present(S) && target_present(T) && history && status && instances_needed);
  SDG_CHECK_ARG(n == 0 || (m && v && m != v));
  SDG_CHECK_ARG(F.first_adam_step >= 0 && F.first_adam_step < INT32_MAX - steps);
  bool any_stats = false;
  if (F.h_stats)
    for (int s = 0; s < steps; ++s) any_stats = any_stats || F.h_stats[s] != 0;
  SDG_CHECK_ARG(!any_stats || n == 0 || (F.grad_accum && F.denom && F.max_radii));
  SDG_CHECK_ARG(aligned4(F.grad_accum) && aligned4(F.denom) && aligned4(F.max_radii));
  SDG_CHECK_ARG(aligned4(xyz) && aligned4(scale) && aligned4(rot) && aligned4(opacity) && aligned4(f_dc) && aligned4(f_rest) && aligned4(cams) &&
                aligned4(m) && aligned4(v) && aligned4(history) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws;
  float* rows = (float*)(w + L.rows);
  char* tgt = w + L.target;
  float* loss = (float*)(w + L.loss);
  int64_t* count = (int64_t*)(w + L.count);
  // group order: xyz, f_dc, f_rest, opacity, scale, rot; a cleared bit of group_mask leaves the gradient NULL everywhere below
  float* d[ga::kGroups];
  for (int k = 0; k < ga::kGroups; ++k)
    d[k] = (n > 0 && ((group_mask >> k) & 1) && ga::group_width(k, n_coef) > 0) ? (float*)(w + L.g[k]) : nullptr;
  const size_t state_bytes = (size_t)state_floats(n, n_coef) * sizeof(float);
  hipError_t e = hipSuccess;
  if (zero_state) {
    if (state_bytes) {
      if ((e = hipMemsetAsync(m, 0, state_bytes, s)) != hipSuccess) return (int)e;
      if ((e = hipMemsetAsync(v, 0, state_bytes, s)) != hipSuccess) return (int)e;
    }
    if ((e = hipMemsetAsync(status, 0, sizeof(int32_t), s)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(instances_needed, 0, sizeof(int64_t), s)) != hipSuccess) return (int)e;
  }
  int32_t* const radii = zero_state ? nullptr : (int32_t*)(w + L.radii);
  int adam_step = F.first_adam_step;      // Adam's counter counts the updates actually made
  const size_t view_bytes = (size_t)height * (size_t)width * (size_t)target_stride * (target_is_u8 ? 1 : sizeof(float));
  const int64_t op_off = n * 3 * ((int64_t)n_coef + 1);      // the opacity slice of m and v: behind xyz, f_dc and f_rest
  for (int step = 0; step < steps; ++step) {
    const int32_t* view = h_view + (size_t)step * batch;
    const float* step_rows = batch > 1 ? rows : cams + 16 * (size_t)view[0];      // one view is read where it lies, more are gathered
    T.data = batch > 1 ? tgt : (const char*)target + view_bytes * (size_t)view[0];
    if (batch > 1)
      for (int b = 0; b < batch; ++b) {
        if ((e = hipMemcpyAsync(rows + 16 * (size_t)b, cams + 16 * (size_t)view[b], 16 * sizeof(float), hipMemcpyDeviceToDevice, s)) != hipSuccess)
          return (int)e;
        if ((e = hipMemcpyAsync(tgt + view_bytes * (size_t)b, (const char*)target + view_bytes * (size_t)view[b], view_bytes,
                                hipMemcpyDeviceToDevice, s)) != hipSuccess)
          return (int)e;
      }
    const bool stats = any_stats && n > 0 && F.h_stats[step] != 0;
    int st = render_pass(S, h_sh_degree[step], step_rows, batch, width, height, T, lambda, max_instances, L, w, (float*)(w + L.grad), d[0],
                             d[4], d[5], d[3], d[1], d[2], nullptr, stream, stats ? radii : nullptr);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_fit_record, dim3((unsigned)sdg_cdiv(batch, 64)), dim3(64), 0, s, loss, batch, count, max_instances,
                       history + (size_t)step * batch, status, instances_needed);
    SDG_LAUNCH_OK();
    if (n == 0) continue;
    if (stats) {      // behind k_fit_record, whose bit 1 it reads
      st = sixdgs_densify_stats(n, batch, width, height, max_instances, w + L.fwd, L.fwd_bytes, w + L.bwd, L.bwd_bytes, radii, F.grad_accum,
                                F.denom, F.max_radii, nullptr, status, stream);
      if (st != 0) return st;
    }
    if (!F.h_update || F.h_update[step])
      st = sixdgs_gaussian_adam(n, n_coef, adam_step++, xyz, f_dc, f_rest, opacity, scale, rot, d[0], d[1], d[2], d[3], d[4], d[5], m, v,
                              h_lr + (size_t)step * ga::kGroups, beta1, beta2, eps, count, max_instances, status, stream);
    if (st != 0) return st;
    if (h_reset[step]) {
      st = launch_reset(opacity, n, opacity_is_logit, m + op_off, v + op_off, reset_ceiling, status, s);
      if (st != 0) return st;
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int sixdgs_gaussian_adam(int64_t n, int n_coef, int step, float* xyz, float* f_dc, float* f_rest, float* opacity, float* scale, float* rot,
                         const float* d_xyz, const float* d_f_dc, const float* d_f_rest, const float* d_opacity, const float* d_scale,
                         const float* d_rot, float* m, float* v, const float* lr, float beta1, float beta2, float eps, const int64_t* instances,
                         int64_t max_instances, int32_t* status, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(sizes_ok(n, n_coef, max_instances));
  SDG_CHECK_ARG(step >= 0 && step < INT32_MAX);
  SDG_CHECK_ARG(lr_ok(lr) && hyper_ok(beta1, beta2, eps));
  if (n == 0) return 0;
  float* const p[ga::kGroups] = {xyz, f_dc, f_rest, opacity, scale, rot};
  const float* const g[ga::kGroups] = {d_xyz, d_f_dc, d_f_rest, d_opacity, d_scale, d_rot};
  SDG_CHECK_ARG(m && v && status && m != v);
  SDG_CHECK_ARG(aligned4(m) && aligned4(v) && aligned4(status) && ((uintptr_t)instances & 7) == 0);
  const ps::Adam adam = ps::adam_at(step, 0.f, beta1, beta2, eps);
  AdamArgs A = {};
  int64_t off = 0, chunks = 0;
  for (int k = 0; k < ga::kGroups; ++k) {
    const int64_t count = n * ga::group_width(k, n_coef);
    Group& G = A.grp[k];
    if (count > 0 && g[k]) {
      SDG_CHECK_ARG(p[k] && aligned4(p[k]) && aligned4(g[k]));
      G.p = p[k];
      G.g = g[k];
      G.m = m + off;
      G.v = v + off;
      G.count = count;
      G.rate = ga::rate(adam, lr[k]);
      G.vec = aligned16(G.p) && aligned16(G.g) && aligned16(G.m) && aligned16(G.v);
      chunks += sdg_cdiv(count, kChunk);
    }
    G.chunk_end = chunks;
    off += count;
  }
  A.chunks = chunks;
  A.instances = instances;
  A.max_instances = max_instances;
  A.status = status;
  const int64_t blocks = chunks < 1 ? 1 : (chunks < kMaxBlocks ? chunks : kMaxBlocks);
  hipLaunchKernelGGL(k_gaussian_adam, dim3((unsigned)blocks), dim3(kBlock), 0, sdg_stream(stream), A);
  SDG_LAUNCH_OK();
  return 0;
}

int sixdgs_opacity_reset(float* opacity, int64_t n, int opacity_is_logit, float* m_opacity, float* v_opacity, float ceiling,
                         sixdgs_stream_t stream) {
  SDG_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31));
  SDG_CHECK_ARG(opacity_is_logit == 0 || opacity_is_logit == 1);
  SDG_CHECK_ARG(ceiling > 0.f && ceiling < 1.f);
  if (n == 0) return 0;
  SDG_CHECK_ARG(opacity && aligned4(opacity) && aligned4(m_opacity) && aligned4(v_opacity));
  SDG_CHECK_ARG(opacity != m_opacity && opacity != v_opacity && (!m_opacity || m_opacity != v_opacity));
  return launch_reset(opacity, n, opacity_is_logit, m_opacity, v_opacity, ceiling, nullptr, sdg_stream(stream));
}

size_t sixdgs_fit_scene_workspace_bytes(int64_t n, int n_coef, int batch, int width, int height, int64_t max_instances) {
  return layout(n, n_coef, batch, width, height, max_instances).total;
}

int sixdgs_fit_scene(float* xyz, float* scale, int scale_is_log, float* rot, float* opacity, int opacity_is_logit, float* f_dc, float* f_rest,
                     int n_coef, int64_t n, const float* cams, int views, int width, int height, float scale_modifier, const float* background,
                     const void* target, int target_is_u8, int target_stride, float lambda, int steps, int batch, const int32_t* h_view,
                     const float* h_lr, const int32_t* h_sh_degree, const uint8_t* h_reset, int group_mask, float beta1, float beta2, float eps,
                     float reset_ceiling, int64_t max_instances, float* m, float* v, float* history, int32_t* status, int64_t* instances_needed,
                     void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const Fit F = {xyz, scale, rot, opacity, f_dc, f_rest, scale_is_log, opacity_is_logit, n_coef, n, cams, views, width, height, scale_modifier,
                 background, target, target_is_u8, target_stride, lambda, steps, batch, h_view, h_lr, h_sh_degree, h_reset, nullptr, nullptr, 0,
                 group_mask, beta1, beta2, eps, reset_ceiling, max_instances, m, v, history, status, instances_needed, nullptr, nullptr, nullptr,
                 ws, ws_bytes, stream};
  return fit_steps(F, true);
}

size_t sixdgs_fit_scene_steps_workspace_bytes(int64_t n, int n_coef, int batch, int width, int height, int64_t max_instances) {
  return layout(n, n_coef, batch, width, height, max_instances, true).total;
}

int sixdgs_fit_scene_steps(float* xyz, float* scale, int scale_is_log, float* rot, float* opacity, int opacity_is_logit, float* f_dc,
                           float* f_rest, int n_coef, int64_t n, const float* cams, int views, int width, int height, float scale_modifier,
                           const float* background, const void* target, int target_is_u8, int target_stride, float lambda, int steps, int batch,
                           const int32_t* h_view, const float* h_lr, const int32_t* h_sh_degree, const uint8_t* h_reset, const uint8_t* h_update,
                           const uint8_t* h_stats, int first_adam_step, int group_mask, float beta1, float beta2, float eps, float reset_ceiling,
                           int64_t max_instances, float* m, float* v, float* history, int32_t* status, int64_t* instances_needed,
                           float* grad_accum, int32_t* denom, int32_t* max_radii, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const Fit F = {xyz, scale, rot, opacity, f_dc, f_rest, scale_is_log, opacity_is_logit, n_coef, n, cams, views, width, height, scale_modifier,
                 background, target, target_is_u8, target_stride, lambda, steps, batch, h_view, h_lr, h_sh_degree, h_reset, h_update, h_stats,
                 first_adam_step, group_mask, beta1, beta2, eps, reset_ceiling, max_instances, m, v, history, status, instances_needed, grad_accum,
                 denom, max_radii, ws, ws_bytes, stream};
  return fit_steps(F, false);
}

}  // extern "C"
