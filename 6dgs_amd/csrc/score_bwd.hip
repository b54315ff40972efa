// score_bwd.hip -- backward of the scorer's softmax-over-rays column sum (training: ops.ray_attention_scores, the scorer of
// IdentificationModule.forward_window).  For image b, with s[t][r] = q_t . k_r / sqrt(384), A[t][r] = softmax_r(s[t]),
// score[r] = sum_t A[t][r] and g[r] = dL/dscore[r]:
//
//   c[t]  = sum_r A[t][r] g[r]
//   dS    = A[t][r] (g[r] - c[t])
//   dq_t  = sum_r dS[t][r] k_r / sqrt(384)
//   dk_r  = sum_b sum_t dS[t][r] q_t / sqrt(384)
//
// Two kernels, neither with partial sums nor atomics (every sum has one owner and a fixed order: two calls give the same bits):
//   k_bwd_q  one workgroup = 128 tokens of one image.  Sweep 1 over all rays forms the softmax sum and c (kept in the workspace for
//            k_bwd_k), sweep 2
//            recomputes the logits, forms dS and accumulates dq = dS . K in registers.  Two sweeps rather than one sweep of
//            sum A g k and sum A k: their difference cancels where g is nearly constant over the rays that carry the mass.
//   k_bwd_k  one workgroup = 128 rays.  Walks every 128-token tile of every image, recomputes the logits, forms dS with c of
//            k_bwd_q and accumulates dk = dS^T . Q in registers.
// The logits are recomputed from q, key and the forward's row maxima on the fp32 MFMA chain (gemm_tile<kMmaF32>,
// the arithmetic the scorer's parity tests use); no [B,T,R] buffer exists.  The dS tile goes through LDS and both products run on
// v_mfma_f32_32x32x2f32 too: A spans many orders of magnitude within a row, and fp32 operands keep every one of them.
// sixdgs_score_backward_split runs k_bwd_q's two sweeps over G groups of ray tiles (k_bwd_q_part1 / k_bwd_q_part2), with fixed-order
// reductions of the groups' partial sums (k_bwd_combine, k_bwd_dq_reduce) between and after them; see the kernels below.
#include "gemm_kernel.h"

using namespace sdg;

namespace {

constexpr int kT = SIXDGS_MAX_TOKENS;
constexpr int kD = SIXDGS_D;
constexpr float kSqrtD = 19.595917942265423f;   // (float)sqrt(384), the forward's divisor
constexpr int kTile = 128;                       // tokens x rays of one logits tile (gemm_tile)
constexpr int kDsLd = kTile + 1;                 // LDS row of the dS tile (odd: the transposed stores of k_bwd_q hit distinct banks)
constexpr int kSlab = 32;                        // rows of the second operand (K or Q) staged per LDS slab
constexpr int kOpLd = kD + 32;                   // its LDS row: the two 32-lane halves of a read land on disjoint banks
constexpr int kOpBytes = kSlab * kOpLd * 4;
constexpr int kGemmBytes = TileSmem<kMmaF32>::kBytes;
constexpr int kStageBytes = kGemmBytes > kOpBytes ? kGemmBytes : kOpBytes;   // the logits' staging and the operand slab share LDS
constexpr int kNF = kD / 2 / 32;                 // 32-feature blocks per wave column (6)

struct BwdArgs {
  const float* q;       // [B,256,384]
  const int* n_tok;     // [B]
  const float* key;     // [R,384]
  const float* stats;   // [B,256,2] (max, sumexp)
  const float* g;       // [B,R]
  float* c;             // [B,256] workspace: c of k_bwd_q, read by k_bwd_k
  float* ssum;          // [B,256] workspace: sum_r exp(s - max) of k_bwd_q's logits, read by k_bwd_k
  float* dq;            // [B,256,384]
  float* dk;            // [R,384]
  int64_t r;
  int batch;
};

// (max, 1 / sumexp, c) of the tile's 128 tokens into LDS; tokens at or beyond n_tok get (0, 0, 0), which makes their A exactly 0
// (their q rows are read as zeros, so their logits are 0 and exp(0 - 0) * 0 = 0).  The max is the forward's; the sum and c are
// k_bwd_q's (with_c), formed on the logits the backward recomputes -- so that A sums to 1 on THOSE logits: with the forward's sum
// (other rounding of the logits) 1 - A of a ray that holds nearly all of a token's mass, and with it g - c, lost up to 9x the
// accuracy of PyTorch's fp32 softmax backward in the peaked regime.
__device__ __forceinline__ void load_rows(const BwdArgs& A, int b, int row0, int M, bool with_c, float* s_m, float* s_is, float* s_c) {
  const int tid = threadIdx.x;
  if (tid < kTile) {
    const int t = row0 + tid;
    const bool v = t < M;
    const int64_t i = (int64_t)b * kT + t;
    s_m[tid] = v ? A.stats[2 * i] : 0.f;
    s_is[tid] = (v && with_c) ? 1.f / A.ssum[i] : 0.f;
    s_c[tid] = (v && with_c) ? A.c[i] : 0.f;
  }
}

// dS of this thread's 2 x 2 x 16 logits (acc: rows = tokens, columns = rays), stored to LDS as [ray][token] (TRANSPOSE, for dq) or
// [token][ray] (for dk).  Rays at or beyond R get dS = 0 by a select (their A is not 0: the key rows read as zeros).  COPY: k_bwd_q_part2
// calls its own instance (1), so that k_bwd_q's stays the only caller of store_ds<true, 0> and compiles to the code it had before the split.
template <bool TRANSPOSE, int COPY = 0>
__device__ __forceinline__ void store_ds(const f32x16 (&acc)[2][2], const float* gv, const bool* cv, const float* s_m, const float* s_is,
                                         const float* s_c, float* sds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(wm, tm, i, lane);
      const float m = s_m[row], is = s_is[row], c = s_c[row];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int col = acc_col(wn, tn, lane);
        const float a = expf(acc[tm][tn][i] / kSqrtD - m) * is;
        const float ds = cv[tn] ? a * (gv[tn] - c) : 0.f;
        sds[TRANSPOSE ? col * kDsLd + row : row * kDsLd + col] = ds;
      }
    }
}

// out[i][f] += sum_k sds'[k][i] op[k][f] over the 128 k of the tile: sds' is the dS tile with k leading (k = ray for dq, token for dk),
// op[k] = row k0 + k of `src` (rows >= `rows` read as zeros), staged through LDS 32 rows at a time.  Wave (wm, wn) owns rows
// wm*64 .. +63 and features wn*192 .. +191 of the output: 2 x 6 accumulators of 32 x 32.
__device__ __forceinline__ void ds_times_operand(const float* sds, const float* __restrict__ src, int64_t k0, int64_t rows, float* sop,
                                                 f32x16 (&out)[2][kNF]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  for (int s = 0; s < kTile; s += kSlab) {
    __syncthreads();                                  // dS stored / the previous slab consumed
#pragma unroll
    for (int p = 0; p < kSlab * kD / 4 / 256; ++p) {  // 12 float4 per thread
      const int e = (p * 256 + tid) * 4, k = e / kD, f = e % kD;
      const int64_t row = k0 + s + k;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < rows) v = *reinterpret_cast<const float4*>(src + row * kD + f);
      *reinterpret_cast<float4*>(sop + k * kOpLd + f) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kSlab; kk += 2) {
      const int k = kk + kh;
      const float a0 = sds[(s + k) * kDsLd + wm * 64 + l31];
      const float a1 = sds[(s + k) * kDsLd + wm * 64 + 32 + l31];
#pragma unroll
      for (int j = 0; j < kNF; ++j) {
        const float bv = sop[k * kOpLd + wn * (kD / 2) + j * 32 + l31];
        out[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, out[0][j], 0, 0, 0);
        out[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, out[1][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                    // before the next logits tile restages the shared LDS
}

__device__ __forceinline__ void zero_out(f32x16 (&out)[2][kNF]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < kNF; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) out[t][j][i] = 0.f;
}

// out / sqrt(384) -> dst rows base_row + (wave rows), features of the wave; rows at or beyond `rows` are not written
__device__ __forceinline__ void write_out(const f32x16 (&out)[2][kNF], float* __restrict__ dst, int base_row, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t row = (int64_t)base_row + acc_row(wm, t, i, lane);
      if (row >= rows) continue;
#pragma unroll
      for (int j = 0; j < kNF; ++j) dst[row * kD + wn * (kD / 2) + j * 32 + (lane & 31)] = out[t][j][i] / kSqrtD;
    }
}

__global__ void __launch_bounds__(256, 1) k_bwd_q(BwdArgs A) {
  __shared__ __attribute__((aligned(16))) char stage[kStageBytes];
  __shared__ float sds[kTile * kDsLd];
  __shared__ float s_m[kTile], s_is[kTile], s_c[kTile], s_red[2][kTile], s_sum[2][kTile];
  const int b = blockIdx.y, row0 = blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int M = min(max(A.n_tok[b], 0), kT);
  float* dq = A.dq + ((int64_t)b * kT + row0) * kD;
  if (row0 >= M) {                                    // no token of this tile: dq rows and c are 0
    for (int e = tid * 4; e < kTile * kD; e += 256 * 4) *reinterpret_cast<float4*>(dq + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < kTile) {
      A.c[(int64_t)b * kT + row0 + tid] = 0.f;
      A.ssum[(int64_t)b * kT + row0 + tid] = 1.f;
    }
    return;
  }
  load_rows(A, b, row0, M, false, s_m, s_is, s_c);
  __syncthreads();
  const GemmOperands go = {A.q + (int64_t)b * kT * kD, nullptr, A.key, kD, 0, kD, M, A.r, kD, kD, nullptr, nullptr, nullptr};
  const float* g = A.g + (int64_t)b * A.r;
  const int n_tiles = (int)((A.r + kTile - 1) / kTile);
  char* smem = stage;
  // ---- sweep 1: S[t] = sum_r exp(s - max_t) and c[t] = sum_r exp(s - max_t) g[r] / S[t]; each thread sums its two columns per tile,
  // the row owner folds lanes and waves at the end
  float cp[2][16], sp[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) cp[t][i] = sp[t][i] = 0.f;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int64_t col0 = (int64_t)tile * kTile;
    f32x16 acc[2][2];
    gemm_tile<kMmaF32>(go, row0, col0, smem, acc);
    float gv[2];
    bool cv[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = col0 + acc_col(wn, tn, lane);
      cv[tn] = col < A.r;
      gv[tn] = cv[tn] ? g[col] : 0.f;
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float m = s_m[acc_row(wm, tm, i, lane)];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float e = cv[tn] ? expf(acc[tm][tn][i] / kSqrtD - m) : 0.f;
          sp[tm][i] += e;
          cp[tm][i] += e * gv[tn];
        }
      }
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = cp[tm][i], w = sp[tm][i];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {                            // the 32 columns of the half-wave (same row)
        v += __shfl_xor(v, o, 64);
        w += __shfl_xor(w, o, 64);
      }
      if ((lane & 31) == 0) {
        s_red[wn][acc_row(wm, tm, i, lane)] = v;
        s_sum[wn][acc_row(wm, tm, i, lane)] = w;
      }
    }
  __syncthreads();
  if (tid < kTile) {
    const bool v = row0 + tid < M;
    const float sum = v ? s_sum[0][tid] + s_sum[1][tid] : 1.f;
    const float c = v ? (s_red[0][tid] + s_red[1][tid]) / sum : 0.f;
    s_c[tid] = c;
    s_is[tid] = v ? 1.f / sum : 0.f;                                 // as load_rows forms it in k_bwd_k
    A.c[(int64_t)b * kT + row0 + tid] = c;
    A.ssum[(int64_t)b * kT + row0 + tid] = sum;
  }
  __syncthreads();
  // ---- sweep 2: dS, then dq += dS . K
  f32x16 out[2][kNF];
  zero_out(out);
  float* sop = reinterpret_cast<float*>(stage);
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int64_t col0 = (int64_t)tile * kTile;
    f32x16 acc[2][2];
    gemm_tile<kMmaF32>(go, row0, col0, smem, acc);
    float gv[2];
    bool cv[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = col0 + acc_col(wn, tn, lane);
      cv[tn] = col < A.r;
      gv[tn] = cv[tn] ? g[col] : 0.f;
    }
    store_ds<true>(acc, gv, cv, s_m, s_is, s_c, sds);
    ds_times_operand(sds, A.key, col0, A.r, sop, out);
  }
  write_out(out, dq, 0, kTile);                         // rows >= M hold dS = 0: zeros
}

__global__ void __launch_bounds__(256, 1) k_bwd_k(BwdArgs A) {
  __shared__ __attribute__((aligned(16))) char stage[kStageBytes];
  __shared__ float sds[kTile * kDsLd];
  __shared__ float s_m[kTile], s_is[kTile], s_c[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wn = wave & 1;
  const int64_t col0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * kTile;
  float* sop = reinterpret_cast<float*>(stage);
  f32x16 out[2][kNF];
  zero_out(out);
  float gv[2];
  bool cv[2];
  for (int b = 0; b < A.batch; ++b) {
    const int M = min(max(A.n_tok[b], 0), kT);
    const GemmOperands go = {A.q + (int64_t)b * kT * kD, nullptr, A.key, kD, 0, kD, M, A.r, kD, kD, nullptr, nullptr, nullptr};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = col0 + acc_col(wn, tn, lane);
      cv[tn] = col < A.r;
      gv[tn] = cv[tn] ? A.g[(int64_t)b * A.r + col] : 0.f;
    }
    for (int row0 = 0; row0 < M; row0 += kTile) {
      load_rows(A, b, row0, M, true, s_m, s_is, s_c);   // (the previous tile's readers passed ds_times_operand's last barrier)
      f32x16 acc[2][2];
      gemm_tile<kMmaF32>(go, row0, col0, stage, acc);    // its barriers publish s_m / s_is / s_c
      store_ds<false>(acc, gv, cv, s_m, s_is, s_c, sds);
      ds_times_operand(sds, A.q + (int64_t)b * kT * kD, row0, M, sop, out);
    }
  }
  write_out(out, A.dk, (int)col0, A.r);
}

// ---- the ray-split form of k_bwd_q (sixdgs_score_backward_split): the 128-ray tiles are cut into G contiguous groups, one workgroup per
// (token tile, image, group).  k_bwd_q_part1 writes each group's partial (sum_r exp(s - max), sum_r exp(s - max) g) per token,
// k_bwd_combine sums them over g = 0 .. G-1 into ssum and c, k_bwd_q_part2 writes each group's partial dq, k_bwd_dq_reduce sums those over
// g in the same order.  Every sum has one owner and a fixed order: the same inputs and G give the same bits; no atomics.
constexpr int kMaxRayGroups = 1024;

struct SplitArgs {
  BwdArgs a;
  float* part;          // [G][B][256][2] workspace: each group's (sum exp, sum exp g) per token
  float* dqp;           // [G][B][256][384] workspace: each group's dq (already / sqrt(384))
  int groups;
  int n_tiles;          // 128-ray tiles of R
};

__device__ __forceinline__ void group_tiles(const SplitArgs& S, int grp, int& t0, int& t1) {
  const int base = S.n_tiles / S.groups, rem = S.n_tiles % S.groups;
  t0 = grp * base + min(grp, rem);
  t1 = t0 + base + (grp < rem ? 1 : 0);
}

__global__ void __launch_bounds__(256, 1) k_bwd_q_part1(SplitArgs S) {
  __shared__ __attribute__((aligned(16))) char stage[kGemmBytes];
  __shared__ float s_m[kTile], s_is[kTile], s_c[kTile], s_red[2][kTile], s_sum[2][kTile];
  const BwdArgs& A = S.a;
  const int b = blockIdx.y, row0 = blockIdx.x * kTile, grp = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int M = min(max(A.n_tok[b], 0), kT);
  if (row0 >= M) return;                              // k_bwd_combine reads no partial of a token at or beyond n_tok
  load_rows(A, b, row0, M, false, s_m, s_is, s_c);
  __syncthreads();
  const GemmOperands go = {A.q + (int64_t)b * kT * kD, nullptr, A.key, kD, 0, kD, M, A.r, kD, kD, nullptr, nullptr, nullptr};
  const float* g = A.g + (int64_t)b * A.r;
  int t0, t1;
  group_tiles(S, grp, t0, t1);
  float cp[2][16], sp[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) cp[t][i] = sp[t][i] = 0.f;
  for (int tile = t0; tile < t1; ++tile) {
    const int64_t col0 = (int64_t)tile * kTile;
    f32x16 acc[2][2];
    gemm_tile<kMmaF32>(go, row0, col0, stage, acc);
    float gv[2];
    bool cv[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = col0 + acc_col(wn, tn, lane);
      cv[tn] = col < A.r;
      gv[tn] = cv[tn] ? g[col] : 0.f;
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float m = s_m[acc_row(wm, tm, i, lane)];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float e = cv[tn] ? expf(acc[tm][tn][i] / kSqrtD - m) : 0.f;
          sp[tm][i] += e;
          cp[tm][i] += e * gv[tn];
        }
      }
  }
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = cp[tm][i], w = sp[tm][i];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        v += __shfl_xor(v, o, 64);
        w += __shfl_xor(w, o, 64);
      }
      if ((lane & 31) == 0) {
        s_red[wn][acc_row(wm, tm, i, lane)] = v;
        s_sum[wn][acc_row(wm, tm, i, lane)] = w;
      }
    }
  __syncthreads();
  if (tid < kTile) {
    const int64_t i = ((int64_t)grp * A.batch + b) * kT + row0 + tid;
    *reinterpret_cast<float2*>(S.part + 2 * i) = make_float2(s_sum[0][tid] + s_sum[1][tid], s_red[0][tid] + s_red[1][tid]);
  }
}

// one thread per (image, token): ssum and c over the groups in order; tokens at or beyond n_tok get c = 0 (and ssum = 1, as k_bwd_q)
__global__ void __launch_bounds__(256) k_bwd_combine(SplitArgs S) {
  const BwdArgs& A = S.a;
  const int b = blockIdx.x, t = threadIdx.x;
  const int M = min(max(A.n_tok[b], 0), kT);
  const int64_t i = (int64_t)b * kT + t;
  float sum = 1.f, c = 0.f;
  if (t < M) {
    float s = 0.f, cg = 0.f;
    for (int grp = 0; grp < S.groups; ++grp) {
      const float2 p = *reinterpret_cast<const float2*>(S.part + 2 * (((int64_t)grp * A.batch) * kT + i));
      s += p.x;
      cg += p.y;
    }
    sum = s;
    c = cg / s;
  }
  A.c[i] = c;
  A.ssum[i] = sum;
}

__global__ void __launch_bounds__(256, 1) k_bwd_q_part2(SplitArgs S) {
  __shared__ __attribute__((aligned(16))) char stage[kStageBytes];
  __shared__ float sds[kTile * kDsLd];
  __shared__ float s_m[kTile], s_is[kTile], s_c[kTile];
  const BwdArgs& A = S.a;
  const int b = blockIdx.y, row0 = blockIdx.x * kTile, grp = blockIdx.z;
  const int lane = threadIdx.x & 63, wn = (threadIdx.x >> 6) & 1;
  const int M = min(max(A.n_tok[b], 0), kT);
  if (row0 >= M) return;                              // k_bwd_dq_reduce writes those rows as zeros without reading a partial
  load_rows(A, b, row0, M, true, s_m, s_is, s_c);       // the combined ssum and c
  __syncthreads();
  const GemmOperands go = {A.q + (int64_t)b * kT * kD, nullptr, A.key, kD, 0, kD, M, A.r, kD, kD, nullptr, nullptr, nullptr};
  const float* g = A.g + (int64_t)b * A.r;
  int t0, t1;
  group_tiles(S, grp, t0, t1);
  f32x16 out[2][kNF];
  zero_out(out);
  float* sop = reinterpret_cast<float*>(stage);
  for (int tile = t0; tile < t1; ++tile) {
    const int64_t col0 = (int64_t)tile * kTile;
    f32x16 acc[2][2];
    gemm_tile<kMmaF32>(go, row0, col0, stage, acc);
    float gv[2];
    bool cv[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int64_t col = col0 + acc_col(wn, tn, lane);
      cv[tn] = col < A.r;
      gv[tn] = cv[tn] ? g[col] : 0.f;
    }
    store_ds<true, 1>(acc, gv, cv, s_m, s_is, s_c, sds);
    ds_times_operand(sds, A.key, col0, A.r, sop, out);
  }
  write_out(out, S.dqp + (((int64_t)grp * A.batch + b) * kT + row0) * kD, 0, kTile);
}

// one thread per 4 features of one dq row: the sum of the groups' partial dq in order; rows at or beyond n_tok are written as zeros
__global__ void __launch_bounds__(256) k_bwd_dq_reduce(SplitArgs S) {
  const BwdArgs& A = S.a;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;          // float4 index into dq [B,256,384]
  if (e >= (int64_t)A.batch * kT * (kD / 4)) return;
  const int64_t row = e / (kD / 4);
  const int b = (int)(row / kT), t = (int)(row % kT);
  const int M = min(max(A.n_tok[b], 0), kT);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < M) {
    const int64_t stride = (int64_t)A.batch * kT * kD;                 // one group's partial dq
    for (int grp = 0; grp < S.groups; ++grp) {
      const float4 p = *reinterpret_cast<const float4*>(S.dqp + grp * stride + 4 * e);
      s.x += p.x;
      s.y += p.y;
      s.z += p.z;
      s.w += p.w;
    }
  }
  *reinterpret_cast<float4*>(A.dq + 4 * e) = s;
}

// G of sixdgs_score_backward_split: ray_groups > 0 as given, 0 = enough groups that the 2 x B x G workgroups of the two partial kernels
// cover every compute unit once (one workgroup per CU: 143 KB of LDS); either way at most one group per 128-ray tile and kMaxRayGroups
int resolve_ray_groups(int batch, int64_t r, int ray_groups) {
  const int64_t tiles = sdg_cdiv(r > 0 ? r : 0, kTile);
  int64_t g = ray_groups;
  if (ray_groups == 0) {
    static int cus = 0;
    if (cus == 0) {
      int dev = 0;
      hipDeviceProp_t prop;
      cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    const int64_t wgs = 2 * (int64_t)(batch > 0 ? batch : 1);
    g = sdg_cdiv(cus, wgs);
  }
  if (g > tiles) g = tiles;
  if (g > kMaxRayGroups) g = kMaxRayGroups;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

extern "C" {

size_t sixdgs_score_backward_workspace_bytes(int batch) { return 2 * sdg_align((size_t)(batch > 0 ? batch : 0) * kT * sizeof(float)); }

int sixdgs_score_backward(const float* q, const int32_t* d_n_tok, int batch, const float* key, int64_t r, const float* row_stats,
                          const float* g, float* dq, float* dk, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(batch >= 0 && r >= 0);
  if (ws_bytes < sixdgs_score_backward_workspace_bytes(batch)) return SIXDGS_E_WORKSPACE;
  hipStream_t s = sdg_stream(stream);
  if (r > 0 && dk == nullptr) return SIXDGS_E_BADARG;
  if (batch == 0 || r == 0) {                         // nothing to contract: zero gradients
    if (batch > 0) {
      SDG_CHECK_ARG(dq != nullptr);
      hipError_t e = hipMemsetAsync(dq, 0, (size_t)batch * kT * kD * sizeof(float), s);
      if (e != hipSuccess) return (int)e;
    }
    if (r > 0) {
      hipError_t e = hipMemsetAsync(dk, 0, (size_t)r * kD * sizeof(float), s);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  SDG_CHECK_ARG(q && d_n_tok && key && row_stats && g && dq && ws);
  SDG_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)key % 16) == 0 && ((uintptr_t)dq % 16) == 0 && ((uintptr_t)dk % 16) == 0);
  SDG_CHECK_ARG(batch <= 65535 && r <= (int64_t)kTile * 0x7fffffff);
  float* c = (float*)ws;
  float* ssum = (float*)((char*)ws + sdg_align((size_t)batch * kT * sizeof(float)));
  BwdArgs A = {q, d_n_tok, key, row_stats, g, c, ssum, dq, dk, r, batch};
  hipLaunchKernelGGL(k_bwd_q, dim3(kT / kTile, (unsigned)batch), dim3(256), 0, s, A);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_bwd_k, dim3((unsigned)sdg_cdiv(r, kTile)), dim3(256), 0, s, A);
  SDG_LAUNCH_OK();
  return 0;
}

size_t sixdgs_score_backward_split_workspace_bytes(int batch, int64_t r, int ray_groups) {
  if (ray_groups < 0) return 0;
  const int g = resolve_ray_groups(batch, r, ray_groups);
  const size_t base = sixdgs_score_backward_workspace_bytes(batch);
  if (g == 1) return base;
  const size_t rows = (size_t)g * (size_t)(batch > 0 ? batch : 0) * kT;
  return base + sdg_align(rows * 2 * sizeof(float)) + sdg_align(rows * kD * sizeof(float));
}

int sixdgs_score_backward_split(const float* q, const int32_t* d_n_tok, int batch, const float* key, int64_t r, const float* row_stats,
                                const float* g, float* dq, float* dk, int ray_groups, void* ws, size_t ws_bytes, sixdgs_stream_t stream) {
  SDG_CHECK_ARG(ray_groups >= 0 && batch >= 0 && r >= 0);
  const int groups = resolve_ray_groups(batch, r, ray_groups);
  if (groups == 1 || batch == 0 || r == 0)            // one group: k_bwd_q and k_bwd_k as sixdgs_score_backward runs them
    return sixdgs_score_backward(q, d_n_tok, batch, key, r, row_stats, g, dq, dk, ws, ws_bytes, stream);
  if (ws_bytes < sixdgs_score_backward_split_workspace_bytes(batch, r, ray_groups)) return SIXDGS_E_WORKSPACE;
  SDG_CHECK_ARG(q && d_n_tok && key && row_stats && g && dq && dk && ws);
  SDG_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)key % 16) == 0 && ((uintptr_t)dq % 16) == 0 && ((uintptr_t)dk % 16) == 0 &&
                ((uintptr_t)ws % 16) == 0);
  SDG_CHECK_ARG(batch <= 65535 && r <= (int64_t)kTile * 0x7fffffff);
  hipStream_t s = sdg_stream(stream);
  const size_t cbytes = sdg_align((size_t)batch * kT * sizeof(float));
  const size_t rows = (size_t)groups * batch * kT;
  char* w = (char*)ws;
  float* c = (float*)w;
  float* ssum = (float*)(w + cbytes);
  float* part = (float*)(w + 2 * cbytes);
  float* dqp = (float*)(w + 2 * cbytes + sdg_align(rows * 2 * sizeof(float)));
  SplitArgs S = {{q, d_n_tok, key, row_stats, g, c, ssum, dq, dk, r, batch}, part, dqp, groups, (int)sdg_cdiv(r, kTile)};
  const dim3 grid(kT / kTile, (unsigned)batch, (unsigned)groups);
  hipLaunchKernelGGL(k_bwd_q_part1, grid, dim3(256), 0, s, S);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_bwd_combine, dim3((unsigned)batch), dim3(kT), 0, s, S);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_bwd_q_part2, grid, dim3(256), 0, s, S);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_bwd_dq_reduce, dim3((unsigned)sdg_cdiv((int64_t)batch * kT * (kD / 4), 256)), dim3(256), 0, s, S);
  SDG_LAUNCH_OK();
  hipLaunchKernelGGL(k_bwd_k, dim3((unsigned)sdg_cdiv(r, kTile)), dim3(256), 0, s, S.a);
  SDG_LAUNCH_OK();
  return 0;
}

}  // extern "C"
