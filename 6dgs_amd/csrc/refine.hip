// refine.hip -- render-and-compare pose refinement below the C ABI (include/sixdgs.h: sixdgs_pose_compose, sixdgs_pose_step,
// sixdgs_refine_poses, sixdgs_pose_rebase, sixdgs_refine_poses_levels).  The pose arithmetic is pose_step.h's, one thread per view, one
// owner per output, no atomics; the loop enqueues the rasteriser, the photometric loss, the rasteriser's backward and the pose step on
// one stream through their own entry points and never reads anything back.  A level schedule is that loop once per level, each level
// started from the one before's best camera, with the rules of pyramid_rules.h.
#include <math.h>

#include "pose_step.h"
#include "pyramid_rules.h"
#include "render_pass.h"

namespace {

using namespace sdg;
using namespace rp;

constexpr int kBlock = 64;

struct StepArgs {
  const float* start;
  const float* loss;
  const float* d_rows;
  const int64_t* instances;
  int64_t max_instances;
  int views, step, evaluate_only;
  ps::Adam adam;
  float *delta, *m, *v, *rows, *best_loss;
  int32_t* best_step;
  float *best_rows, *history;
  int32_t* status;
  int64_t* instances_needed;
};

__global__ __launch_bounds__(kBlock) void k_pose_compose(const float* __restrict__ start, const float* __restrict__ delta, int views,
                                                         float* __restrict__ rows) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  ps::compose(start + 16 * (size_t)v, delta + 6 * (size_t)v, rows + 16 * (size_t)v);
}

// the state sixdgs_refine_poses starts from: delta = m = v = 0, iterate 0, nothing seen yet
__global__ __launch_bounds__(kBlock) void k_pose_init(const float* __restrict__ start, int views, float* delta, float* m, float* vv, float* rows,
                                                      float* best_loss, int32_t* best_step, float* best_rows, int32_t* status,
                                                      int64_t* instances_needed) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  for (int i = 0; i < 6; ++i) delta[6 * (size_t)v + i] = m[6 * (size_t)v + i] = vv[6 * (size_t)v + i] = 0.f;
  ps::compose(start + 16 * (size_t)v, delta + 6 * (size_t)v, rows + 16 * (size_t)v);
  for (int j = 0; j < 16; ++j) best_rows[16 * (size_t)v + j] = start[16 * (size_t)v + j];
  best_loss[v] = INFINITY;
  best_step[v] = 0;
  status[v] = 0;
  if (v == 0) *instances_needed = 0;
}

__global__ __launch_bounds__(kBlock) void k_pose_step(StepArgs A) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= A.views) return;
  const int64_t count = A.instances ? *A.instances : 0;
  if (v == 0 && count > *A.instances_needed) *A.instances_needed = count;
  const size_t r = 16 * (size_t)v, d = 6 * (size_t)v;
  ps::step_view(A.start + r, A.d_rows ? A.d_rows + r : nullptr, A.loss[v], count, A.max_instances, A.step, A.evaluate_only != 0, A.adam,
                A.delta + d, A.m + d, A.v + d, A.rows + r, A.best_loss + v, A.best_step + v, A.best_rows + r, A.history + v, A.status + v);
}

bool adam_ok(float lr, float beta1, float beta2, float eps) { return lr > 0.f && lr < INFINITY && hyper_ok(beta1, beta2, eps); }

int launch_step(const StepArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_step, dim3((unsigned)sdg_cdiv(A.views, kBlock)), dim3(kBlock), 0, s, A);
  SDG_LAUNCH_OK();
  return 0;
}

struct Layout : PassLayout {
  size_t d_rows, delta, m, v;
};

// 0 total = outside the limits
Layout layout(int64_t n, int views, int width, int height, int64_t max_instances) {
  Layout L = {};
  if (!pass_layout(L, n, views, width, height, max_instances)) return L;
  L.d_rows = L.take((size_t)views * 16 * sizeof(float));
  for (size_t* at : {&L.delta, &L.m, &L.v}) *at = L.take((size_t)views * 6 * sizeof(float));      // the motion and Adam's moments
  return L;
}

// rows_out[v] = (the 12 w2c entries of rows_in[v], intrinsics[v][4]): a copy of bits, through integer registers.  rows_out may be
// rows_in, so neither is __restrict__
__global__ __launch_bounds__(kBlock) void k_pose_rebase(const uint32_t* rows_in, const uint32_t* __restrict__ intrinsics, int views,
                                                        uint32_t* rows_out) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  for (int j = 0; j < 12; ++j) rows_out[16 * (size_t)v + j] = rows_in[16 * (size_t)v + j];
  for (int j = 0; j < 4; ++j) rows_out[16 * (size_t)v + 12 + j] = intrinsics[4 * (size_t)v + j];
}

// the state a level of sixdgs_refine_poses_levels starts from: k_pose_init's, with status and instances_needed left as they are
__global__ __launch_bounds__(kBlock) void k_level_init(const float* __restrict__ start, int views, float* delta, float* m, float* vv, float* rows,
                                                       float* best_loss, int32_t* best_step, float* best_rows) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  for (int i = 0; i < 6; ++i) delta[6 * (size_t)v + i] = m[6 * (size_t)v + i] = vv[6 * (size_t)v + i] = 0.f;
  ps::compose(start + 16 * (size_t)v, delta + 6 * (size_t)v, rows + 16 * (size_t)v);
  for (int j = 0; j < 16; ++j) best_rows[16 * (size_t)v + j] = start[16 * (size_t)v + j];
  best_loss[v] = INFINITY;
  best_step[v] = 0;
}

// the input's loss at the last level: NaN, and bit 1 of every status, when the rasteriser's capacity did not hold it; the first
// writer of status, and view 0 keeps the count
__global__ __launch_bounds__(kBlock) void k_input_record(const float* __restrict__ loss, const int64_t* count, int64_t max_instances, int views,
                                                         float* __restrict__ loss_input, int32_t* __restrict__ status,
                                                         int64_t* instances_needed) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  const int64_t cnt = *count;
  if (v == 0 && cnt > *instances_needed) *instances_needed = cnt;
  const bool over = cnt > max_instances;
  loss_input[v] = over ? NAN : loss[v];
  status[v] = over ? ps::kStatusCapacity : 0;
}

__global__ __launch_bounds__(kBlock) void k_levels_select(const float* __restrict__ start_rows, const float* __restrict__ best_rows,
                                                          const float* __restrict__ best_loss_last, const float* __restrict__ loss_input,
                                                          int views, float* __restrict__ out_rows, int32_t* __restrict__ kept_input) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= views) return;
  const bool keep = pyr::keep_input(best_loss_last[v], loss_input[v]);
  const float* from = (keep ? start_rows : best_rows) + 16 * (size_t)v;
  for (int j = 0; j < 16; ++j) out_rows[16 * (size_t)v + j] = from[j];
  kept_input[v] = keep ? 1 : 0;
}

// The loop sixdgs_refine_poses documents, in the workspace w laid out by L: the state's start, then steps + 1 passes, each followed by
// the pose step.  fresh: status and instances_needed start from zero too (sixdgs_refine_poses); otherwise they are carried
// (a level of sixdgs_refine_poses_levels).  delta may be NULL.
int refine_loop(const Scene& S, int sh_degree, const float* start_rows, int views, int width, int height, const Target& T, float lambda, int steps,
                float lr, float beta1, float beta2, float eps, int64_t max_instances, const Layout& L, char* w, float* delta, float* best_rows,
                float* best_loss, int32_t* best_step, float* history, int32_t* status, int64_t* instances_needed, bool fresh,
                sixdgs_stream_t stream) {
  hipStream_t s = sdg_stream(stream);
  float* rows = (float*)(w + L.rows);
  float* d_rows = (float*)(w + L.d_rows);
  float* loss = (float*)(w + L.loss);
  float* dl = delta ? delta : (float*)(w + L.delta);
  float* m = (float*)(w + L.m);
  float* v = (float*)(w + L.v);
  int64_t* count = (int64_t*)(w + L.count);
  if (fresh)
    hipLaunchKernelGGL(k_pose_init, dim3((unsigned)sdg_cdiv(views, kBlock)), dim3(kBlock), 0, s, start_rows, views, dl, m, v, rows, best_loss,
                       best_step, best_rows, status, instances_needed);
  else
    hipLaunchKernelGGL(k_level_init, dim3((unsigned)sdg_cdiv(views, kBlock)), dim3(kBlock), 0, s, start_rows, views, dl, m, v, rows, best_loss,
                       best_step, best_rows);
  SDG_LAUNCH_OK();
  for (int step = 0; step <= steps; ++step) {
    const int last = step == steps;      // the last evaluation takes no gradient; the others the camera rows' alone
    int st = render_pass(S, sh_degree, rows, views, width, height, T, lambda, max_instances, L, w, last ? nullptr : (float*)(w + L.grad),
                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, last ? nullptr : d_rows, stream);
    if (st != 0) return st;
    const StepArgs A = {start_rows, loss,  last ? nullptr : d_rows, count, max_instances, views, step, last, ps::adam_at(step, lr, beta1, beta2, eps),
                        dl,         m,     v,    rows,  best_loss, best_step, best_rows, history + (size_t)step * views, status,
                        instances_needed};
    st = launch_step(A, s);
    if (st != 0) return st;
  }
  return 0;
}

// sixdgs_refine_poses_levels' workspace: the largest single level's, then the rows handed from level to level
struct LevelsLayout : SdgBump {
  size_t level, start, best;
};

LevelsLayout levels_layout(int64_t n, int views, int levels, const int32_t* h_width, const int32_t* h_height, const int64_t* h_max_instances) {
  LevelsLayout L = {};
  if (levels < 1 || levels > pyr::kMaxLevels || !h_width || !h_height || !h_max_instances) return L;
  size_t widest = 0;
  for (int l = 0; l < levels; ++l) {
    const size_t one = layout(n, views, h_width[l], h_height[l], h_max_instances[l]).total;
    if (one == 0) return L;
    widest = one > widest ? one : widest;
  }
  L.level = L.take(widest);
  L.start = L.take((size_t)views * 16 * sizeof(float));
  L.best = L.take((size_t)views * 16 * sizeof(float));
  return L;
}

}  // namespace

extern "C" {

int sixdgs_pose_compose(const float* start, const float* delta, int views, float* rows, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(views >= 0 && views <= kMaxViews);
  if (views == 0) return 0;
  SDG_CHECK_ARG(start && delta && rows && rows != start);
  SDG_CHECK_ARG(aligned4(start) && aligned4(delta) && aligned4(rows));
  hipLaunchKernelGGL(k_pose_compose, dim3((unsigned)sdg_cdiv(views, kBlock)), dim3(kBlock), 0, sdg_stream(stream), start, delta, views, rows);
  SDG_LAUNCH_OK();
  return 0;
}

int sixdgs_pose_step(const float* start, const float* loss, const float* d_rows, const int64_t* instances, int64_t max_instances, int views,
                     int step, int evaluate_only, float lr, float beta1, float beta2, float eps, float* delta, float* m, float* v, float* rows,
                     float* best_loss, int32_t* best_step, float* best_rows, float* history_row, int32_t* status, int64_t* instances_needed,
                     sixdgs_stream_t stream) {
  SDG_CHECK_ARG(views >= 0 && views <= kMaxViews);
  SDG_CHECK_ARG(step >= 0 && step < INT32_MAX && (evaluate_only == 0 || evaluate_only == 1));
  SDG_CHECK_ARG(max_instances >= 1 && max_instances < ((int64_t)1 << 31));
  SDG_CHECK_ARG(adam_ok(lr, beta1, beta2, eps));
  if (views == 0) return 0;
  SDG_CHECK_ARG(start && loss && (evaluate_only || d_rows) && delta && m && v && rows && best_loss && best_step && best_rows && history_row &&
                status && instances_needed);
  SDG_CHECK_ARG(rows != start && best_rows != rows);
  SDG_CHECK_ARG(aligned4(start) && aligned4(loss) && aligned4(d_rows) && aligned4(delta) && aligned4(m) && aligned4(v) && aligned4(rows) &&
                aligned4(best_loss) && aligned4(best_step) && aligned4(best_rows) && aligned4(history_row) && aligned4(status));
  SDG_CHECK_ARG(((uintptr_t)instances & 7) == 0 && ((uintptr_t)instances_needed & 7) == 0);
  const StepArgs A = {start, loss,      evaluate_only ? nullptr : d_rows, instances, max_instances, views,   step,  evaluate_only,
                      ps::adam_at(step, lr, beta1, beta2, eps), delta, m, v, rows, best_loss, best_step, best_rows, history_row, status,
                      instances_needed};
  return launch_step(A, sdg_stream(stream));
}

size_t sixdgs_refine_poses_workspace_bytes(int64_t n, int views, int width, int height, int64_t max_instances) {
  return layout(n, views, width, height, max_instances).total;
}

int sixdgs_refine_poses(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                        const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* start_rows, int views,
                        int width, int height, float scale_modifier, const float* background, const void* target, int target_is_u8,
                        int target_stride, float lambda, int steps, float lr, float beta1, float beta2, float eps, int64_t max_instances,
                        float* best_rows, float* best_loss, int32_t* best_step, float* history, float* delta, int32_t* status,
                        int64_t* instances_needed, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const Layout L = layout(n, views, width, height, max_instances);
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  const Target T = {target, target_is_u8, target_stride};
  SDG_CHECK_ARG(L.total != 0);
  SDG_CHECK_ARG(scene_ok(S, sh_degree) && target_ok(T));
  SDG_CHECK_ARG(loop_ok(lambda, steps) && adam_ok(lr, beta1, beta2, eps));
  if (views == 0) return 0;
  SDG_CHECK_ARG(start_rows && scene_present(S) && target_present(T));
  SDG_CHECK_ARG(best_rows && best_loss && best_step && history && status && instances_needed);
  SDG_CHECK_ARG(aligned4(start_rows) && aligned4(best_rows) && aligned4(best_loss) && aligned4(best_step) &&
                aligned4(history) && aligned4(delta) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  if (ws_bytes < L.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  return refine_loop(S, sh_degree, start_rows, views, width, height, T, lambda, steps, lr, beta1, beta2, eps, max_instances, L, (char*)ws, delta,
                     best_rows, best_loss, best_step, history, status, instances_needed, true, stream);
}

size_t sixdgs_refine_poses_levels_workspace_bytes(int64_t n, int views, int levels, const int32_t* h_width, const int32_t* h_height,
                                                  const int64_t* h_max_instances) {
  return levels_layout(n, views, levels, h_width, h_height, h_max_instances).total;
}

int sixdgs_pose_rebase(const float* rows_in, const float* intrinsics, int views, float* rows_out, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(views >= 0 && views <= kMaxViews);
  if (views == 0) return 0;
  SDG_CHECK_ARG(rows_in && intrinsics && rows_out && (const float*)rows_out != intrinsics);
  SDG_CHECK_ARG(aligned4(rows_in) && aligned4(intrinsics) && aligned4(rows_out));
  hipLaunchKernelGGL(k_pose_rebase, dim3((unsigned)sdg_cdiv(views, kBlock)), dim3(kBlock), 0, sdg_stream(stream), (const uint32_t*)rows_in,
                     (const uint32_t*)intrinsics, views, (uint32_t*)rows_out);
  SDG_LAUNCH_OK();
  return 0;
}

int sixdgs_refine_poses_levels(const float* xyz, const float* scale, int scale_is_log, const float* rot, const float* opacity, int opacity_is_logit,
                               const float* f_dc, const float* f_rest, int sh_degree, int n_coef, int64_t n, const float* start_rows, int views,
                               float scale_modifier, const float* background, float lambda, int levels, const int32_t* h_width,
                               const int32_t* h_height, const int32_t* h_steps, const float* h_lr, const float* const* h_target,
                               const float* const* h_intrinsics, const int64_t* h_max_instances, float beta1, float beta2, float eps,
                               float* out_rows, float* loss_input, int32_t* kept_input, float* best_loss, int32_t* best_step,
                               int64_t* instances_needed, float* history, int32_t* status, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  const LevelsLayout LL = levels_layout(n, views, levels, h_width, h_height, h_max_instances);
  const Scene S = {xyz, scale, rot, opacity, f_dc, f_rest, background, scale_is_log, opacity_is_logit, n_coef, n, scale_modifier};
  SDG_CHECK_ARG(LL.total != 0);
  SDG_CHECK_ARG(scene_ok(S, sh_degree) && h_steps && h_lr && h_target && h_intrinsics);
  for (int l = 0; l < levels; ++l) SDG_CHECK_ARG(loop_ok(lambda, h_steps[l]) && adam_ok(h_lr[l], beta1, beta2, eps));
  if (views == 0) return 0;
  SDG_CHECK_ARG(start_rows && scene_present(S));
  for (int l = 0; l < levels; ++l) {
    const Target T = {h_target[l], 0, 3};
    SDG_CHECK_ARG(target_present(T) && h_intrinsics[l] && aligned4(h_intrinsics[l]));
  }
  SDG_CHECK_ARG(out_rows && loss_input && kept_input && best_loss && best_step && instances_needed && history && status);
  SDG_CHECK_ARG(out_rows != start_rows);
  SDG_CHECK_ARG(aligned4(start_rows) && aligned4(out_rows) && aligned4(loss_input) && aligned4(kept_input) && aligned4(best_loss) &&
                aligned4(best_step) && aligned4(history) && aligned4(status) && ((uintptr_t)instances_needed & 7) == 0);
  if (ws_bytes < LL.total) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0);
  hipStream_t s = sdg_stream(stream);
  char* w = (char*)ws + LL.level;
  float* start = (float*)((char*)ws + LL.start);
  float* best = (float*)((char*)ws + LL.best);
  const dim3 grid((unsigned)sdg_cdiv(views, kBlock)), block(kBlock);
  hipError_t e = hipMemsetAsync(instances_needed, 0, (size_t)levels * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  // 1. the input's loss at the last level, without a gradient
  const int last = levels - 1;
  {
    const Layout L = layout(n, views, h_width[last], h_height[last], h_max_instances[last]);
    const Target T = {h_target[last], 0, 3};
    const int st = render_pass(S, sh_degree, start_rows, views, h_width[last], h_height[last], T, lambda, h_max_instances[last], L, w, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_input_record, grid, block, 0, s, (const float*)(w + L.loss), (const int64_t*)(w + L.count), h_max_instances[last], views,
                       loss_input, status, instances_needed + last);
    SDG_LAUNCH_OK();
  }
  // 2. the levels: each from the one before's best camera at its own intrinsics
  size_t row = 0;
  for (int l = 0; l < levels; ++l) {
    const Layout L = layout(n, views, h_width[l], h_height[l], h_max_instances[l]);
    const Target T = {h_target[l], 0, 3};
    int st = sixdgs_pose_rebase(l == 0 ? start_rows : best, h_intrinsics[l], views, start, stream);
    if (st != 0) return st;
    st = refine_loop(S, sh_degree, start, views, h_width[l], h_height[l], T, lambda, h_steps[l], h_lr[l], beta1, beta2, eps, h_max_instances[l], L, w,
                     nullptr, best, best_loss + (size_t)l * views, best_step + (size_t)l * views, history + row * views, status,
                     instances_needed + l, false, stream);
    if (st != 0) return st;
    row += (size_t)h_steps[l] + 1;
  }
  // 3. the last level's best camera, or the input
  hipLaunchKernelGGL(k_levels_select, grid, block, 0, s, start_rows, (const float*)best, (const float*)(best_loss + (size_t)last * views),
                     (const float*)loss_input, views, out_rows, kept_input);
  SDG_LAUNCH_OK();
  return 0;
}

}  // extern "C"
