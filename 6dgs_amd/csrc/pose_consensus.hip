// pose_consensus.hip -- consensus pose solver over the top-k rays (include/sixdgs.h: sixdgs_solve_pose_consensus): every pair of rays
// proposes a camera centre, every ray votes on every proposal, the best supported proposal is refined by 8 reweighted least-squares
// steps and handed to the tail of k_solve_pose (watch direction, rotation, fall-backs, errors).  Two kernels:
//   k_consensus_sweep   grid (hypothesis block, image): one hypothesis per thread in registers, the image's rays walked from LDS
//                       (all lanes read the same ray: a broadcast, no bank conflicts), best (S, pair) per block to the workspace;
//   k_consensus_finish  one workgroup per image: best over the blocks, refinement, tail.
// No atomics, one owner per value, sums in a fixed order: the same input gives the same bits on every call and in every batch.
#include "common.h"
#include "device_math.h"

using namespace sdg;

namespace {

constexpr int kConsMaxK = 1024;
constexpr int kConsAllPairsK = 256;        // up to here every unordered pair is a hypothesis
constexpr int kConsHypBudget = 32768;      // beyond: floor(budget / k) rank neighbours per ray
constexpr int kSweepThreads = 256;
constexpr int kFinishThreads = 1024;       // one thread per ray
constexpr int kFinishWaves = kFinishThreads / 64;
constexpr int kRefineIters = 8;
constexpr int kNoPair = 0x7fffffff;

struct ConsArgs {
  const float* rays_ori;
  const float* rays_dir;
  const int64_t* idx;   // [B,k]
  const float* val;     // [B,k]
  const float* up;      // [B,3]
  const float* gt;      // [B,4,4] or null
  float* c2w;           // [B,4,4]
  int* status;          // [B]
  float* w_final;       // [B,k] or null
  int* n_kept;          // [B] or null
  float* centre;        // [B,3] or null
  float* errors;        // [B,2] or null
  float* support;       // [B] or null
  int* n_inliers;       // [B] or null
  float* rms;           // [B] or null
  int* winner;          // [B,2] or null
  float* ws_s;          // [B,n_blk] best support of a block
  int* ws_key;          // [B,n_blk] its pair (i << 10 | j), kNoPair when the block has no valid hypothesis
  int64_t r;
  int k, prior, n_hyp, n_blk;
  float tau, inv_tau2;
};

inline int cons_hypotheses(int k) { return k <= kConsAllPairsK ? k * (k - 1) / 2 : k * (kConsHypBudget / k); }
inline int cons_blocks(int k) { return (cons_hypotheses(k) + kSweepThreads - 1) / kSweepThreads; }
inline size_t cons_ws_bytes(int batch, int k) { return sdg_align((size_t)batch * cons_blocks(k) * sizeof(float)) * 2; }

// larger support wins; equal support: the smaller pair (keys are unique per image, so this is a total order and the result does not
// depend on the order of the comparisons)
__device__ __forceinline__ bool cons_better(float sa, int ka, float sb, int kb) { return sa > sb || (sa == sb && ka < kb); }
__device__ __forceinline__ void cons_wave_best(float& s, int& key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float so = __shfl_xor(s, o, 64);
    const int ko = __shfl_xor(key, o, 64);
    if (cons_better(so, ko, s, key)) { s = so; key = ko; }
  }
}

// midpoint of the closest approach of the lines (oi, di), (oj, dj); false when they are near parallel or the point lies behind a ray
__device__ __forceinline__ bool cons_pair_centre(const V3& oi, const V3& di, const V3& oj, const V3& dj, float* c) {
  const V3 w0 = v3(oi.x - oj.x, oi.y - oj.y, oi.z - oj.z);
  const float b = dot(di, dj), d = dot(di, w0), e = dot(dj, w0);
  const float den = 1.f - b * b;
  if (!(den > 1.0e-6f)) return false;
  const float s = (b * e - d) / den, t = (e - b * d) / den;
  if (!(s > 0.f) || !(t > 0.f)) return false;
  c[0] = 0.5f * ((oi.x + s * di.x) + (oj.x + t * dj.x));
  c[1] = 0.5f * ((oi.y + s * di.y) + (oj.y + t * dj.y));
  c[2] = 0.5f * ((oi.z + s * di.z) + (oj.z + t * dj.z));
  return true;
}

// squared distance of c to the line (o, d) from the perpendicular component itself (|v|^2 - (v.d)^2 would cancel), and the side of o that c is on
__device__ __forceinline__ float cons_residual2(const float* c, const V3& o, const V3& d, bool* front) {
  const V3 v = v3(c[0] - o.x, c[1] - o.y, c[2] - o.z);
  const float t = dot(v, d);
  const V3 p = v3(v.x - t * d.x, v.y - t * d.y, v.z - t * d.z);
  *front = t > 0.f;
  return dot(p, p);
}

// hypothesis number -> pair of top-k positions
__device__ __forceinline__ void cons_pair_of(int h, int k, int* pi, int* pj) {
  if (k <= kConsAllPairsK) {                 // row-major upper triangle: row i starts at i (2k - i - 1) / 2
    const float fk = (float)(2 * k - 1);
    int i = (int)((fk - sqrtf(fmaxf(fk * fk - 8.f * (float)h, 0.f))) * 0.5f);
    i = i < 0 ? 0 : (i > k - 2 ? k - 2 : i);
    while (i > 0 && i * (2 * k - i - 1) / 2 > h) --i;
    while (i < k - 2 && (i + 1) * (2 * k - i - 2) / 2 <= h) ++i;
    *pi = i;
    *pj = i + 1 + (h - i * (2 * k - i - 1) / 2);
  } else {
    const int m = kConsHypBudget / k;
    const int i = h / m;
    *pi = i;
    *pj = (i + 1 + (h - i * m)) % k;
  }
}

__global__ void __launch_bounds__(kSweepThreads) k_consensus_sweep(ConsArgs A) {
  __shared__ float sox[kConsMaxK], soy[kConsMaxK], soz[kConsMaxK], sdx[kConsMaxK], sdy[kConsMaxK], sdz[kConsMaxK], sp[kConsMaxK];
  __shared__ float s_s[kSweepThreads / 64];
  __shared__ int s_k[kSweepThreads / 64];
  const int b = blockIdx.y, tid = threadIdx.x, k = A.k;
  const int64_t* idx = A.idx + (int64_t)b * k;
  // the image's rays, once per workgroup; padding entries become rays that vote for nothing.  The prior is left un-normalised here:
  // a common positive factor does not change which hypothesis is best
  for (int i = tid; i < k; i += kSweepThreads) {
    const int64_t id = idx[i];
    const bool ok = id >= 0 && id < A.r;
    float raw = 0.f;
    if (ok) {
      raw = 1.f;
      if (A.prior) {
        const float v = A.val[(int64_t)b * k + i];
        raw = v > 0.f ? v : 0.f;
      }
    }
    sox[i] = ok ? A.rays_ori[3 * id] : 0.f;
    soy[i] = ok ? A.rays_ori[3 * id + 1] : 0.f;
    soz[i] = ok ? A.rays_ori[3 * id + 2] : 0.f;
    sdx[i] = ok ? A.rays_dir[3 * id] : 0.f;
    sdy[i] = ok ? A.rays_dir[3 * id + 1] : 0.f;
    sdz[i] = ok ? A.rays_dir[3 * id + 2] : 0.f;
    sp[i] = raw;
  }
  __syncthreads();
  float best = -1.f;
  int key = kNoPair;
  const int h = blockIdx.x * kSweepThreads + tid;
  if (h < A.n_hyp) {
    int i, j;
    cons_pair_of(h, k, &i, &j);
    const int64_t ii = idx[i], jj = idx[j];
    float c[3];
    if (ii >= 0 && ii < A.r && jj >= 0 && jj < A.r &&
        cons_pair_centre(v3(sox[i], soy[i], soz[i]), v3(sdx[i], sdy[i], sdz[i]), v3(sox[j], soy[j], soz[j]), v3(sdx[j], sdy[j], sdz[j]), c)) {
      float acc = 0.f;                        // index order
#pragma unroll 4
      for (int q = 0; q < k; ++q) {
        bool front;
        const float r2 = cons_residual2(c, v3(sox[q], soy[q], soz[q]), v3(sdx[q], sdy[q], sdz[q]), &front);
        const float t = sp[q] * __builtin_amdgcn_rcpf(1.f + r2 * A.inv_tau2);
        acc += front ? t : 0.f;
      }
      if (acc >= 0.f) {                       // (a NaN support never wins)
        best = acc;
        key = (i << 10) | j;
      }
    }
  }
  cons_wave_best(best, key);
  if ((tid & 63) == 0) { s_s[tid >> 6] = best; s_k[tid >> 6] = key; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSweepThreads / 64; ++w)
      if (cons_better(s_s[w], s_k[w], best, key)) { best = s_s[w]; key = s_k[w]; }
    A.ws_s[(int64_t)b * A.n_blk + blockIdx.x] = best;
    A.ws_key[(int64_t)b * A.n_blk + blockIdx.x] = key;
  }
}

// Sum of v[q] over the workgroup, every thread receives the same bits.  The fixed tree of the header: rays in groups of 64 consecutive
// positions, inside a group the butterfly of sdg_wave_sum, the 16 group sums added in group order.
template <int N>
__device__ __forceinline__ void cons_block_sum(float (&v)[N], float* s_part) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = sdg_wave_sum(v[q]);
  __syncthreads();                            // the previous sum's readers are done with s_part
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < N; ++q) s_part[(threadIdx.x >> 6) * N + q] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    float s = s_part[q];
#pragma unroll 1
    for (int w = 1; w < kFinishWaves; ++w) s += s_part[w * N + q];
    v[q] = s;
  }
}

__global__ void __launch_bounds__(kFinishThreads) k_consensus_finish(ConsArgs A) {
  __shared__ float s_part[kFinishWaves * 12];
  __shared__ float s_s[kFinishWaves];
  __shared__ int s_k[kFinishWaves];
  const int b = blockIdx.x, tid = threadIdx.x, k = A.k;
  const int64_t* idx = A.idx + (int64_t)b * k;

  // ---- this thread's ray -------------------------------------------------------------------------------------------------------
  bool ok = false;
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 0.f);
  float raw = 0.f;
  if (tid < k) {
    const int64_t id = idx[tid];
    ok = id >= 0 && id < A.r;
    if (ok) {
      o = v3(A.rays_ori[3 * id], A.rays_ori[3 * id + 1], A.rays_ori[3 * id + 2]);
      d = v3(A.rays_dir[3 * id], A.rays_dir[3 * id + 1], A.rays_dir[3 * id + 2]);
      raw = 1.f;
      if (A.prior) {
        const float v = A.val[(int64_t)b * k + tid];
        raw = v > 0.f ? v : 0.f;
      }
    }
  }
  float p;
  int n;
  {
    float t[2] = {raw, ok ? 1.f : 0.f};
    cons_block_sum(t, s_part);
    p = ok ? raw / t[0] : 0.f;
    n = (int)t[1];
  }

  // ---- best hypothesis over the sweep's blocks -----------------------------------------------------------------------------------
  float best = -1.f;
  int key = kNoPair;
  if (tid < A.n_blk) {
    best = A.ws_s[(int64_t)b * A.n_blk + tid];
    key = A.ws_key[(int64_t)b * A.n_blk + tid];
  }
  cons_wave_best(best, key);
  if ((tid & 63) == 0) { s_s[tid >> 6] = best; s_k[tid >> 6] = key; }
  __syncthreads();
  best = s_s[0];
  key = s_k[0];
  for (int w = 1; w < kFinishWaves; ++w)
    if (cons_better(s_s[w], s_k[w], best, key)) { best = s_s[w]; key = s_k[w]; }
  float c[3] = {NAN, NAN, NAN};
  bool won = false;
  int wi = -1, wj = -1;
  if (n >= 2 && key != kNoPair && best >= 0.f) {
    wi = key >> 10;
    wj = key & 1023;
    const int64_t ii = idx[wi], jj = idx[wj];      // valid: the sweep only records pairs of valid rays
    won = cons_pair_centre(v3(A.rays_ori[3 * ii], A.rays_ori[3 * ii + 1], A.rays_ori[3 * ii + 2]),
                           v3(A.rays_dir[3 * ii], A.rays_dir[3 * ii + 1], A.rays_dir[3 * ii + 2]),
                           v3(A.rays_ori[3 * jj], A.rays_ori[3 * jj + 1], A.rays_ori[3 * jj + 2]),
                           v3(A.rays_dir[3 * jj], A.rays_dir[3 * jj + 1], A.rays_dir[3 * jj + 2]), c);
  }
  if (!won) { wi = -1; wj = -1; }

  int st = 0;
  // per-ray projector I - d d^T (symmetric: 6 entries) and (I - d d^T) o
  const float P00 = 1.f - d.x * d.x, P01 = 0.f - d.x * d.y, P02 = 0.f - d.x * d.z, P11 = 1.f - d.y * d.y, P12 = 0.f - d.y * d.z,
              P22 = 1.f - d.z * d.z;
  const float q0 = (P00 * o.x + P01 * o.y) + P02 * o.z, q1 = (P01 * o.x + P11 * o.y) + P12 * o.z, q2 = (P02 * o.x + P12 * o.y) + P22 * o.z;
  if (won) {
    // ---- refinement: 8 reweighted least-squares steps with the Geman-McClure weight, tau fixed ---------------------------------
#pragma unroll 1
    for (int it = 0; it < kRefineIters; ++it) {
      bool front;
      const float r2 = cons_residual2(c, o, d, &front);
      const float den = 1.f + r2 * A.inv_tau2;
      const float w = (ok && front) ? p / (den * den) : 0.f;
      float t[10] = {w * P00, w * P01, w * P02, w * P11, w * P12, w * P22, w * q0, w * q1, w * q2, w};
      cons_block_sum(t, s_part);
      float m[9] = {t[0], t[1], t[2], t[1], t[3], t[4], t[2], t[4], t[5]};
      int piv[3];
      const float sg = lu3(m, piv);
      const float det = sg * m[0] * m[4] * m[8];
      if (!(det > 0.f) || det < 1.0e-7f * ((t[9] * t[9]) * t[9])) break;      // (the same decision on every thread)
      float x[3] = {t[6], t[7], t[8]};
      lu3_solve(m, piv, x);
      if (!(x[0] == x[0] && x[1] == x[1] && x[2] == x[2])) break;
      c[0] = x[0]; c[1] = x[1]; c[2] = x[2];
    }
  } else {
    // ---- no hypothesis: the plain unweighted least-squares centre over the valid rays -----------------------------------------
    st |= 8;
    const float u = ok ? 1.f : 0.f;
    float t[9] = {u * P00, u * P01, u * P02, u * P11, u * P12, u * P22, u * q0, u * q1, u * q2};
    cons_block_sum(t, s_part);
    const float Rm[9] = {t[0], t[1], t[2], t[1], t[3], t[4], t[2], t[4], t[5]};
    const float qv[3] = {t[6], t[7], t[8]};
    if (!solve_centre(Rm, qv, c)) st |= 4;
  }

  // ---- at the final centre: weights, support, inliers, rms, watch direction --------------------------------------------------------
  bool front;
  const float r2 = cons_residual2(c, o, d, &front);
  const bool in = ok && front;
  const float den = 1.f + r2 * A.inv_tau2;
  const float w = in ? (won ? p / (den * den) : p) : 0.f;
  float t[4] = {w, in ? w * r2 : 0.f, in ? p / den : 0.f, (in && sqrtf(r2) <= 2.f * A.tau) ? 1.f : 0.f};
  cons_block_sum(t, s_part);
  const float wn = in ? w / t[0] : 0.f;
  float wd[3] = {d.x * wn, d.y * wn, d.z * wn};
  cons_block_sum(wd, s_part);
  if (A.w_final && tid < k) A.w_final[(int64_t)b * k + tid] = wn;
  if (tid != 0) return;

  // ---- tail, as in k_solve_pose ---------------------------------------------------------------------------------------------------
  const float nrm = sqrtf((wd[0] * wd[0] + wd[1] * wd[1]) + wd[2] * wd[2]);
  const V3 neg = v3(-(wd[0] / nrm), -(wd[1] / nrm), -(wd[2] / nrm));
  const V3 upv = v3(A.up[3 * b], A.up[3 * b + 1], A.up[3 * b + 2]);
  float Rw[9];
  make_rotation_mat(neg, upv, Rw);
  if (det3(Rw) < 1.0e-7f) {
    st |= 1;
    for (int i = 0; i < 9; ++i) Rw[i] = (i % 4 == 0) ? 1.f : 0.f;
  }
  float Ri[9];
  if (!inv3(Rw, Ri))
    for (int i = 0; i < 9; ++i) Ri[i] = NAN;
  float out[16];
  for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.f : 0.f;
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) out[4 * r + cc] = Ri[3 * r + cc];
    out[4 * r + 3] = c[r];
  }
  bool nan = false;
  for (int i = 0; i < 16; ++i) nan = nan || !(out[i] == out[i]);
  if (nan) {
    st |= 2;
    for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  for (int i = 0; i < 16; ++i) A.c2w[16 * b + i] = out[i];
  A.status[b] = st;
  if (A.centre)
    for (int i = 0; i < 3; ++i) A.centre[3 * b + i] = c[i];
  if (A.n_kept) A.n_kept[b] = n;
  if (A.errors) {
    float te = NAN, ae = NAN;
    if (A.gt) pose_errors(A.gt + 16 * b, out, &te, &ae);
    A.errors[2 * b] = te;
    A.errors[2 * b + 1] = ae;
  }
  if (A.support) A.support[b] = t[2];
  if (A.n_inliers) A.n_inliers[b] = (int)t[3];
  if (A.rms) A.rms[b] = sqrtf(t[1] / t[0]);
  if (A.winner) { A.winner[2 * b] = wi; A.winner[2 * b + 1] = wj; }
}

}  // namespace

extern "C" size_t sixdgs_solve_pose_consensus_workspace_bytes(int batch, int k) {
  if (batch < 0 || k < 2 || k > kConsMaxK) return 0;
  return cons_ws_bytes(batch, k);
}

extern "C" int sixdgs_solve_pose_consensus(const float* rays_ori, const float* rays_dir, int64_t r, const int64_t* idx, const float* val,
                                           int k, const float* up, const float* gt_c2w, int batch, float tau, int prior, float* c2w,
                                           int32_t* status, float* w_final, int32_t* n_kept, float* centre, float* errors, float* support,
                                           int32_t* n_inliers, float* rms, int32_t* winner, void* ws, size_t ws_bytes,
                                           sixdgs_stream_t stream) {
  SDG_CHECK_ARG(batch >= 0 && batch <= 65535 && k >= 2 && k <= kConsMaxK && r >= 0);
  SDG_CHECK_ARG(tau > 0.f && (prior == 0 || prior == 1));
  const float inv_tau2 = 1.f / (tau * tau);
  SDG_CHECK_ARG(inv_tau2 > 0.f && inv_tau2 <= 3.0e38f);       // tau^2 must be a finite, non-zero fp32 number
  SDG_CHECK_ARG(ws_bytes >= cons_ws_bytes(batch, k));
  if (batch == 0) return 0;
  SDG_CHECK_ARG(rays_ori && rays_dir && idx && val && up && c2w && status && ws && ((uintptr_t)ws % 4) == 0);
  const int n_blk = cons_blocks(k);
  float* ws_s = (float*)ws;
  int* ws_key = (int*)((char*)ws + sdg_align((size_t)batch * n_blk * sizeof(float)));
  ConsArgs A = {rays_ori, rays_dir, idx,    val,    up,     gt_c2w, c2w, status, w_final, n_kept,          centre, errors,
                support,  n_inliers, rms,   winner, ws_s,   ws_key, r,   k,      prior,   cons_hypotheses(k), n_blk,  tau,
                inv_tau2};
  hipStream_t s = sdg_stream(stream);
  hipLaunchKernelGGL(k_consensus_sweep, dim3((unsigned)n_blk, (unsigned)batch), dim3(kSweepThreads), 0, s, A);
  hipLaunchKernelGGL(k_consensus_finish, dim3((unsigned)batch), dim3(kFinishThreads), 0, s, A);
  SDG_LAUNCH_OK();
  return 0;
}
