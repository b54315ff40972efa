// hostcheck.cpp -- HOST instantiation of device_math.h (the per-thread math of the HIP kernels), of dense_layout.h (the index
// arithmetic of the ray-MLP chain's operand planes), of pose_step.h (the per-view arithmetic of pose refinement) and of adam_step.h
// (the per-entry arithmetic of fitting a scene's Gaussians) behind a tiny C ABI, so the CPU test-suite can compare the product's arithmetic with the oracle and the
// golden vectors without a GPU.  densify_rules.h (the per-entry rules of a densification round) and knn_rules.h (the pair and box rules
// of the 3-nearest-neighbour search) are instantiated here too, and pyramid_rules.h (a level schedule's geometry, target value and
// keep-the-input rule) and image_prep_rules.h (the spans, weights and launch plan of the one-pass image preparation).  Contains no kernels; never used by the product path.
#include <stdlib.h>

#include "device_math.h"
#include "sweep_plan.h"
#include "dense_layout.h"
#include "sweep_layout.h"
#include "pose_step.h"
#include "adam_step.h"
#include "densify_rules.h"
#include "knn_rules.h"
#include "pyramid_rules.h"
#include "image_prep_rules.h"

#include <algorithm>
#include <vector>
using namespace sdg;

extern "C" {

void hc_mask_degraded(const float* scale, long long n, int P, unsigned char* mask) {
  for (long long i = 0; i < n; ++i) {
    float side;
    mask[i] = total_rings(scale[3 * i], scale[3 * i + 1], scale[3 * i + 2], (float)P, &side) < (long long)P;
  }
}

long long hc_quadricell_centers(const float* scale, long long E, int P, int res, float* points, long long* eid) {
  long long C = 0;
  float* table = (float*)malloc(sizeof(float) * res);
  for (long long e = 0; e < E; ++e) {
    float a = scale[3 * e], b = scale[3 * e + 1], c = scale[3 * e + 2], side;
    long long rings = total_rings(a, b, c, (float)P, &side);
    for (long long ring = 0; ring < rings; ++ring) {
      Ring rg = ring_params(a, b, c, side, (float)rings, (float)ring);
      int npts = ring_cells(rg);
      if (!npts) continue;
      if (points) {
        double acc = 0.0;
        table[0] = 0.f;
        for (int j = 0; j < res - 1; ++j) { acc += (double)ring_table_increment(rg, j); table[j + 1] = (float)acc; }
        float last = table[res - 1];
        for (int j = 0; j < res; ++j) table[j] = kTwoPi * (table[j] / last);
        for (int j = 0; j < npts; ++j) {
          int pick = ring_table_pick(table, res, (float)j * rg.dtheta);
          V3 p = ring_point(rg, table[pick]);
          points[3 * (C + j)] = p.x; points[3 * (C + j) + 1] = p.y; points[3 * (C + j) + 2] = p.z;
          eid[C + j] = e;
        }
      }
      C += npts;
    }
  }
  free(table);
  return C;
}

long long hc_emit_rays(const float* points, const long long* eid, long long C, const float* normals, const float* centers,
                       const float* rot4, float* ori, float* dir, long long* mid) {
  long long r = 0;
  for (long long i = 0; i < C; ++i) {
    long long e = eid[i];
    float R[9];
    quat_to_rotmat(rot4 + 4 * e, R);
    V3 pw = rotate(R, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]));
    if (!hemisphere_keep(normals[3 * e], pw)) continue;
    V3 d = normalize_eps(pw);
    ori[3 * r] = pw.x + centers[3 * e]; ori[3 * r + 1] = pw.y + centers[3 * e + 1]; ori[3 * r + 2] = pw.z + centers[3 * e + 2];
    dir[3 * r] = d.x; dir[3 * r + 1] = d.y; dir[3 * r + 2] = d.z;
    mid[r++] = e;
  }
  return r;
}

void hc_sym_eig(const float* mats, long long n, float* vals, float* vecs) {
  for (long long i = 0; i < n; ++i) sym_eig_3x3(mats + 9 * i, vals + 3 * i, vecs ? vecs + 9 * i : nullptr);
}

void hc_normals_from_knn(const float* cloud, const long long* knn, long long nq, int k, float* normals) {
  float* nb = (float*)malloc(sizeof(float) * 3 * k);
  for (long long q = 0; q < nq; ++q) {
    for (int j = 0; j < k; ++j)
      for (int c = 0; c < 3; ++c) nb[3 * j + c] = cloud[3 * knn[q * k + j] + c];
    V3 n = normal_from_neighbours(nb, k);
    normals[3 * q] = n.x; normals[3 * q + 1] = n.y; normals[3 * q + 2] = n.z;
  }
  free(nb);
}

long long hc_isocell_dirs(int target, int n0, float* dirs) {
  int n = isocell_rings(target, n0);
  long long o = 0;
  for (int ring = 1; ring <= n; ++ring)
    for (int j = 0; j < n0 * (2 * ring - 1); ++j, ++o)
      if (dirs) { V3 d = isocell_dir(n, n0, ring, j); dirs[3 * o] = d.x; dirs[3 * o + 1] = d.y; dirs[3 * o + 2] = d.z; }
  return o;
}

void hc_rotate_isocell(const float* dirs, long long K, const float* normals, long long E, float* out) {
  for (long long e = 0; e < E; ++e) {
    float Rm[9];
    isocell_rotation(v3(normals[3 * e], normals[3 * e + 1], normals[3 * e + 2]), Rm);
    for (long long k = 0; k < K; ++k) {
      V3 d = isocell_apply(Rm, v3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]));
      float* o = out + 3 * (e * K + k);
      o[0] = d.x; o[1] = d.y; o[2] = d.z;
    }
  }
}

void hc_sh_color(const float* sh, int ncoef, const float* dirs, long long R, int deg, float* rgb) {
  for (long long i = 0; i < R; ++i)
    for (int ch = 0; ch < 3; ++ch)
      rgb[3 * i + ch] = sh_channel(sh + (3 * i + ch) * ncoef, 1, deg, -dirs[3 * i], -dirs[3 * i + 1], -dirs[3 * i + 2]);
}

void hc_ray_input(const float* ori, const float* dir, const float* rgb, long long R, float* x) {
  for (long long i = 0; i < R; ++i)
    for (int c = 0; c < 144; ++c) x[144 * i + c] = ray_input_element(ori + 3 * i, dir + 3 * i, rgb + 3 * i, c);
}

void hc_make_rotation_mat(const float* d, const float* up, float* Rm) { make_rotation_mat(v3(d[0], d[1], d[2]), v3(up[0], up[1], up[2]), Rm); }

int hc_solve_centre(const float* Rm, const float* q, float* c) { return solve_centre(Rm, q, c) ? 1 : 0; }

void hc_pose_errors(const float* gt, const float* pr, float* out2) { pose_errors(gt, pr, out2, out2 + 1); }

void hc_distance_target(const float* pose, const float* ori, const float* dir, long long r, float* out) {
  for (long long i = 0; i < r; ++i)
    out[i] = distance_target(pose, v3(ori[3 * i], ori[3 * i + 1], ori[3 * i + 2]), v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]));
}

// ---- dense_layout.h: the ray-MLP chain's operand planes (tests/test_dense_layout.py walks a tag through them) ----
int hc_dl_row_perm(int m) { return dl::row_perm(m); }
int hc_dl_acc_row(int lane, int r) { return dl::acc_row(lane, r); }
int hc_dl_acc_feature(int permuted, int lane, int r) { return dl::acc_feature(permuted != 0, lane, r); }
long long hc_dl_plane_offset(int chunk_major, long long ray, int nslab, int slab, int plane, int c) {
  return chunk_major ? dl::cm_offset(ray, nslab, slab, plane, c) : dl::rm_offset(ray, nslab, slab, plane, c);
}
unsigned hc_dl_lds_offset(unsigned row, unsigned plane, unsigned c) { return dl::lds_offset(row, plane, c); }
unsigned hc_dl_frag_offset(unsigned row0, unsigned lane, unsigned ks, unsigned plane) { return dl::frag_offset(row0, lane, ks, plane); }
unsigned hc_dl_load_ray(int chunk_major, unsigned tid, unsigned jp) { return dl::load_ray(chunk_major != 0, tid, jp); }
unsigned hc_dl_load_chunk8(int chunk_major, unsigned tid) { return dl::load_chunk8(chunk_major != 0, tid); }
unsigned hc_dl_cm_src_offset(unsigned ray_in_tile, unsigned chunk8, unsigned granule_stride) {
  return dl::cm_src_offset(ray_in_tile, chunk8 * (unsigned)dl::kChunkRun, granule_stride);
}
int hc_sweep_launch_images(int left, int cap) { return sdg::sweep_launch_images(left, cap); }
// sweep_pack flattened: per launch hc_sweep_pack_ints() ints = n_slots, n_images, q_img[slots][4], q_lq[slots][4], img[], img_nq[], img_q[][4]
int hc_sweep_pack_ints() { return 2 + 2 * sdg::kSweepMaxSlots * sdg::kSlotQuarters + (2 + sdg::kSlotQuarters) * sdg::kSweepMaxLaunchImages; }
int hc_sweep_max_slots() { return sdg::kSweepMaxSlots; }
int hc_sweep_pack(const int* h_n_tok, int batch, int cap, int* out, int max_launches) {
  const std::vector<sdg::SweepSlots> plan = sdg::sweep_pack(h_n_tok, batch, cap);
  const int per = hc_sweep_pack_ints();
  for (size_t l = 0; l < plan.size() && (int)l < max_launches; ++l) {
    const sdg::SweepSlots& t = plan[l];
    int* o = out + (size_t)l * per;
    *o++ = t.n_slots;
    *o++ = t.n_images;
    for (int s = 0; s < sdg::kSweepMaxSlots; ++s)
      for (int w = 0; w < sdg::kSlotQuarters; ++w) *o++ = t.q_img[s][w];
    for (int s = 0; s < sdg::kSweepMaxSlots; ++s)
      for (int w = 0; w < sdg::kSlotQuarters; ++w) *o++ = t.q_lq[s][w];
    for (int i = 0; i < sdg::kSweepMaxLaunchImages; ++i) *o++ = t.img[i];
    for (int i = 0; i < sdg::kSweepMaxLaunchImages; ++i) *o++ = t.img_nq[i];
    for (int i = 0; i < sdg::kSweepMaxLaunchImages; ++i)
      for (int w = 0; w < sdg::kSlotQuarters; ++w) *o++ = t.img_q[i][w];
  }
  return (int)plan.size();
}
// ---- sweep_layout.h: the select sweep on 16x16x32 MFMAs (tests/test_sweep_layout.py walks every lane and register through them) ----
int hc_sw_const(int which) {
  const int v[] = {sw::kTokBlocks, sw::kRayBlocks, sw::kBlockBytes, sw::kBflySteps};
  return which >= 0 && which < 4 ? v[which] : -1;
}
int hc_sw_frag_row(int lane) { return sw::frag_row(lane); }
int hc_sw_frag_chunk(int lane, int plane) { return sw::frag_chunk(lane, plane); }
unsigned hc_sw_frag_offset(int row0, int lane, int plane) { return sw::frag_offset(row0, lane, plane); }
int hc_sw_acc_token(int lane, int tb) { return sw::acc_token(lane, tb); }
int hc_sw_acc_ray(int lane, int rb, int reg) { return sw::acc_ray(lane, rb, reg); }
int hc_sw_bfly_partner(int lane, int step) { return sw::bfly_partner(lane, step); }
int hc_sw_bfly_keeps(int lane, int step, int i) { return sw::bfly_keeps(lane, step, i) ? 1 : 0; }
int hc_sw_out_index(int lane, int x) { return sw::out_index(lane, x); }
int hc_sw_out_ray(int lane, int x) { return sw::out_ray(lane, x); }
int hc_sw_part_writes(int lane) { return sw::part_writes(lane) ? 1 : 0; }
int hc_sw_part_row(int wn, int lane) { return sw::part_row(wn, lane); }
// ---- pose_step.h: the per-view arithmetic of refine.hip (tests/test_pose_step_host.py) ----
float hc_ps_series_below() { return ps::kSeriesBelow; }
void hc_ps_coeffs(const float* x, long long n, float* abc) {
  for (long long i = 0; i < n; ++i) {
    const ps::Coeffs k = ps::rot_coeffs(x[i]);
    abc[3 * i] = k.a; abc[3 * i + 1] = k.b; abc[3 * i + 2] = k.c;
  }
}
void hc_ps_compose(const float* start, const float* delta, long long views, float* rows) {
  for (long long v = 0; v < views; ++v) ps::compose(start + 16 * v, delta + 6 * v, rows + 16 * v);
}
void hc_ps_chain(const float* start, const float* delta, const float* d_rows, long long views, float* g) {
  for (long long v = 0; v < views; ++v) ps::chain(start + 16 * v, delta + 6 * v, d_rows + 16 * v, g + 6 * v);
}
// sixdgs_pose_step on the host: the same per-view function in the kernel's order (view 0 owns instances_needed)
void hc_ps_step(const float* start, const float* loss, const float* d_rows, const long long* instances, long long max_instances, int views, int step,
                int evaluate_only, float lr, float beta1, float beta2, float eps, float* delta, float* m, float* v, float* rows, float* best_loss,
                int* best_step, float* best_rows, float* history_row, int* status, long long* instances_needed) {
  const ps::Adam p = ps::adam_at(step, lr, beta1, beta2, eps);
  const long long count = instances ? *instances : 0;
  if (views > 0 && count > *instances_needed) *instances_needed = count;
  for (int i = 0; i < views; ++i)
    ps::step_view(start + 16 * i, d_rows ? d_rows + 16 * i : nullptr, loss[i], count, max_instances, step, evaluate_only != 0, p, delta + 6 * i,
                  m + 6 * i, v + 6 * i, rows + 16 * i, best_loss + i, best_step + i, best_rows + 16 * i, history_row + i, status + i);
}
// ---- adam_step.h: the per-entry arithmetic of fit.hip (tests/test_gaussian_adam_host.py) ----
// sixdgs_gaussian_adam on the host: the same per-entry function over the six groups (p[k], g[k] NULL: frozen) -> the status bits
int hc_ga_adam(long long n, int n_coef, int step, float* const* p, const float* const* g, float* m, float* v, const float* lr, float beta1,
               float beta2, float eps) {
  const ps::Adam adam = ps::adam_at(step, 0.f, beta1, beta2, eps);
  int status = 0;
  long long off = 0;
  for (int k = 0; k < ga::kGroups; ++k) {
    const long long count = n * ga::group_width(k, n_coef);
    if (g[k]) {
      const ga::Rate r = ga::rate(adam, lr[k]);
      for (long long i = 0; i < count; ++i)
        if (!ga::adam_entry(r, g[k][i], p[k][i], m[off + i], v[off + i])) status |= ga::kStatusNotFinite;
    }
    off += count;
  }
  return status;
}
void hc_ga_reset(float* opacity, long long n, int is_logit, float ceiling) {
  for (long long i = 0; i < n; ++i) opacity[i] = ga::reset_entry(opacity[i], is_logit != 0, ceiling);
}
// ---- densify_rules.h: the per-entry rules of densify.hip (tests/test_densify_host.py) ----
void hc_dn_thresholds(float grad_threshold, float percent_dense, float extent, float min_opacity, int scale_is_log, int opacity_is_logit,
                      float* out4) {
  const dn::Thresholds t = dn::thresholds(grad_threshold, percent_dense, extent, min_opacity, scale_is_log, opacity_is_logit, 0, 0);
  out4[0] = t.grad; out4[1] = t.dense; out4[2] = t.world; out4[3] = t.opacity;
}
// sixdgs_densify's classification on the host: cls [n] (0 keep, 1 clone, 2 split), avg [n], flags [4][n] (the candidate of that segment
// exists and survives the prune), child_xyz [n][2][3] and child_scale [n][3] (of every Gaussian, split or not)
void hc_dn_round(long long n, const float* xyz, const float* opacity, const float* scale, const float* rot, int scale_is_log, int opacity_is_logit,
                 const float* grad_accum, const int* denom, const int* max_radii, const float* noise, float grad_threshold, float percent_dense,
                 float extent, float min_opacity, int prune_big, int screen_size, int* cls, float* avg, int* flags, float* child_xyz,
                 float* child_scale) {
  const dn::Thresholds t = dn::thresholds(grad_threshold, percent_dense, extent, min_opacity, scale_is_log, opacity_is_logit, prune_big != 0,
                                          screen_size);
  for (long long i = 0; i < n; ++i) {
    int f[dn::kSegments];
    cls[i] = dn::candidate_flags(grad_accum[i], denom[i], scale + 3 * i, opacity[i], max_radii[i], scale_is_log != 0, t, f);
    avg[i] = dn::avg_grad(grad_accum[i], denom[i]);
    for (int g = 0; g < dn::kSegments; ++g) flags[g * n + i] = f[g];
    for (int j = 0; j < 2; ++j)
      dn::child_xyz(xyz + 3 * i, rot + 4 * i, scale + 3 * i, scale_is_log != 0, noise + (i * 2 + j) * 3, child_xyz + (i * 2 + j) * 3);
    for (int k = 0; k < 3; ++k) child_scale[3 * i + k] = dn::child_scale(scale[3 * i + k], scale_is_log != 0);
  }
}
// ---- knn_rules.h: the pair and box rules of knn.hip (tests/test_knn_host.py) ----
int hc_knn_box() { return kn::kBox; }
void hc_knn_morton(long long n, const float* xyz, const float* lo, const float* hi, unsigned* code, unsigned* cells) {
  for (long long i = 0; i < n; ++i) {
    code[i] = kn::morton(xyz + 3 * i, lo, hi);
    for (int a = 0; a < 3; ++a) cells[3 * i + a] = kn::axis_cell(xyz[3 * i + a], lo[a], hi[a]);
  }
}
// per query q[i] and box (lo[i], hi[i]): box_d2; per pair: d2 from q[i] to p[i]
void hc_knn_box_d2(long long n, const float* q, const float* lo, const float* hi, float* out) {
  for (long long i = 0; i < n; ++i) out[i] = kn::box_d2(q[3 * i], q[3 * i + 1], q[3 * i + 2], lo + 3 * i, hi + 3 * i);
}
void hc_knn_box_box_d2(long long n, const float* qlo, const float* qhi, const float* lo, const float* hi, float* out) {
  for (long long i = 0; i < n; ++i) out[i] = kn::box_box_d2(qlo + 3 * i, qhi + 3 * i, lo + 3 * i, hi + 3 * i);
}
void hc_knn_pair_d2(long long n, const float* q, const float* p, float* out) {
  for (long long i = 0; i < n; ++i) out[i] = kn::pair_d2(q[3 * i], q[3 * i + 1], q[3 * i + 2], p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
// sixdgs_knn_mean_dist2's whole scheme on the host: bounding box, Morton codes, a stable sort, boxes of `box` consecutive sorted points
// with their AABBs, and per query the own box, then the others outward, pruned with box_d2 >= best[2] -> mean_d2 [n]; visited (may be
// NULL) receives the number of boxes walked per query.  Returns 0, or -1 for n < 4.
int hc_knn_boxed(long long n, const float* xyz, int box, float* mean_d2, int* visited) {
  if (n < 4 || box < 1) return -1;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = INFINITY, hi[a] = -INFINITY;
  for (long long i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], xyz[3 * i + a]);
      hi[a] = fmaxf(hi[a], xyz[3 * i + a]);
    }
  std::vector<unsigned> code(n);
  std::vector<long long> order(n);
  for (long long i = 0; i < n; ++i) {
    code[i] = kn::morton(xyz + 3 * i, lo, hi);
    order[i] = i;
  }
  std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return code[a] < code[b]; });
  const long long nb = (n + box - 1) / box;
  std::vector<float> s(3 * n), blo(3 * nb, INFINITY), bhi(3 * nb, -INFINITY);
  for (long long k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a) {
      const float c = s[3 * k + a] = xyz[3 * order[k] + a];
      blo[3 * (k / box) + a] = fminf(blo[3 * (k / box) + a], c);
      bhi[3 * (k / box) + a] = fmaxf(bhi[3 * (k / box) + a], c);
    }
  for (long long k = 0; k < n; ++k) {
    const float qx = s[3 * k], qy = s[3 * k + 1], qz = s[3 * k + 2];
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    const long long own = k / box;
    int walked = 0;
    for (long long step = 0; step < nb; ++step)
      for (int side = 0; side < (step ? 2 : 1); ++side) {
        const long long c = side ? own + step : own - step;
        if (c < 0 || c >= nb) continue;
        if (step && kn::box_d2(qx, qy, qz, &blo[3 * c], &bhi[3 * c]) >= b2) continue;
        ++walked;
        const long long end = std::min(n, (c + 1) * box);
        for (long long j = c * box; j < end; ++j)
          if (j != k) kn::insert3(kn::pair_d2(qx, qy, qz, s[3 * j], s[3 * j + 1], s[3 * j + 2]), b0, b1, b2);
      }
    mean_d2[order[k]] = kn::mean3(b0, b1, b2);
    if (visited) visited[order[k]] = walked;
  }
  return 0;
}
// ---- pyramid_rules.h: the rules of a level schedule (tests/test_pyramid_host.py) ----
int hc_pyr_max_levels() { return pyr::kMaxLevels; }
int hc_pyr_max_downscale() { return pyr::kMaxDownscale; }
// geo4 = (w, h, ox, oy); k_out4 = the level's intrinsics of k4 = (fx, fy, cx, cy)
void hc_pyr_geometry(int W, int H, int d, const float* k4, int* geo4, float* k_out4) {
  const pyr::Level g = pyr::level_geometry(W, H, d);
  geo4[0] = g.w; geo4[1] = g.h; geo4[2] = g.ox; geo4[3] = g.oy;
  pyr::level_intrinsics(k4, d, g.ox, g.oy, k_out4);
}
// sixdgs_target_pyramid's one level on the host: images [views][H][W][C] -> out [views][h][w][3]; -1 where the entry point refuses
int hc_pyr_target(const unsigned char* images, int views, int H, int W, int C, int composite, const float* background, int d, float* out) {
  if (d < 1 || d > pyr::kMaxDownscale || (C != 3 && C != 4) || (composite && C != 4)) return -1;
  const pyr::Level g = pyr::level_geometry(W, H, d);
  if (g.w < 1 || g.h < 1) return -1;
  float bg255[3] = {0.f, 0.f, 0.f};
  if (composite)
    for (int c = 0; c < 3; ++c) bg255[c] = pyr::background_term(background[c]);
  for (int v = 0; v < views; ++v)
    for (int y = 0; y < g.h; ++y)
      for (int x = 0; x < g.w; ++x)
        for (int c = 0; c < 3; ++c) {
          unsigned S = 0u, S2 = 0u;
          for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) {
              const unsigned char* q = images + (((size_t)v * H + (size_t)(g.oy + y * d + j)) * W + (size_t)(g.ox + x * d + i)) * C;
              if (composite) {
                S += (unsigned)q[c] * (unsigned)q[3];
                S2 += 255u - (unsigned)q[3];
              } else {
                S += (unsigned)q[c];
              }
            }
          out[(((size_t)v * g.h + y) * g.w + x) * 3 + c] = composite ? pyr::value_composite(S, S2, bg255[c], d) : pyr::value_plain(S, d);
        }
  return 0;
}
void hc_pyr_keep_input(const float* best_loss_last, const float* loss_input, long long n, int* keep) {
  for (long long i = 0; i < n; ++i) keep[i] = pyr::keep_input(best_loss_last[i], loss_input[i]) ? 1 : 0;
}
// ---- image_prep_rules.h: spans, weights and the launcher's plan of sixdgs_image_prep (tests/test_image_prep_host.py) ----
// plan5 = (kt, rb, nrmax, lds_bytes, supported); scales4 (may be NULL) = (sh, sw, sup_h, sup_w); returns supported
int hc_ip_plan(int batch, int height, int width, int resized_h, int resized_w, int out_size, long long* plan5, float* scales4) {
  const ip::Plan p = ip::plan(batch, height, width, resized_h, resized_w, out_size);
  plan5[0] = p.kt; plan5[1] = p.rb; plan5[2] = p.nrmax; plan5[3] = (long long)p.lds_bytes; plan5[4] = p.supported ? 1 : 0;
  if (scales4) { scales4[0] = p.sh; scales4[1] = p.sw; scales4[2] = p.sup_h; scales4[3] = p.sup_w; }
  return p.supported ? 1 : 0;
}
// output indices i0 .. i0 + count of the resized grid along an axis of n samples: weights_out [count][kt], meta_out [count][2] = (xmin, min(xsize, kt))
void hc_ip_spans(int i0, int count, int n, float scale, float support, int kt, float* weights_out, int* meta_out) {
  for (int i = 0; i < count; ++i) ip::aa_weights(i0 + i, n, scale, support, kt, weights_out + (size_t)i * kt, meta_out + 2 * i);
}
// the same indices: xsize_out [count] = the span's size before aa_weights caps it at kt
void hc_ip_span_sizes(int i0, int count, int n, float scale, float support, int* xsize_out) {
  for (int i = 0; i < count; ++i) {
    int xmin;
    ip::aa_span(i0 + i, n, scale, support, xmin, xsize_out[i]);
  }
}
// the largest row window r1 - r0 over the bands of rb output rows of a crop of out_size rows that starts at row `top` of the resized grid
int hc_ip_max_window(int height, int top, int out_size, int rb, float sh, float sup_h, int kt) {
  int worst = 0;
  for (int oy0 = 0; oy0 < out_size; oy0 += rb) {
    int r0, r1;
    ip::band_window(top, oy0, std::min(rb, out_size - oy0), height, sh, sup_h, kt, r0, r1);
    worst = std::max(worst, r1 - r0);
  }
  return worst;
}
int hc_dl_const(int which) {
  const int v[] = {dl::kSlabB, dl::kPRow, dl::kGran, dl::kGranSlab, dl::kChunkRun};
  return which >= 0 && which < 5 ? v[which] : -1;
}

}  // extern "C"
