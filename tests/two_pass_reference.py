"""fp64 reference, error bound, top-k rule and case table of the two-pass scorer's edge tests (test_gpu_two_pass_edges.py on the GPU,
test_two_pass_reference_host.py on the CPU).  Plain torch: the same code runs in fp64 on the CPU for the host tests and on the GPU for
the large cases.  Importing it needs no GPU.

Reference.  Per image b with T = n_tok[b] tokens
    logit[t][r] = q[b][t] . key[r] / sqrt(384),   p[t][r] = softmax over r,   s[r] = sum_{t < T} p[t][r],
with the row statistics (max_r logit, sum_r exp(logit - max)).  The operands are the fp32 values as given; in the plane modes the key is
the one DECODED from the scaled fp16 planes (decode()), which is what those kernels multiply.  dtype = float32 gives the fp32 restatement
whose own distance from fp64 is the yardstick e32.

Bound, per ray (never relative to the largest score):
    |s_kernel[r] - s64[r]| <= eps_b s64[r] + A[r] (1 + eps_b) + T_b 2^-125
    eps_b = 4 e32_b + 8e-7 B_b + 2^-24 sqrt(R) + (2^-20 in MMA_F16X3 only)
  e32_b     largest per-ray relative error of the fp32 restatement of the case against fp64; the factor 4 is the suite's (training-path and
            train-window tests).  The restatement gets the same absolute allowance T_b 2^-125 as the kernel before its error is divided by
            s64[r]: a ray whose score lies below fp32's normal range has no relative accuracy in ANY fp32 evaluation, and without the
            allowance one such ray would set e32 = 1 and empty the bound of every other ray (this only ever tightens the bound);
  B_b       max_{t,r} sum_k |q_tk| |key_rk| / sqrt(384).  The suite asserts 4e-7 B per logit (test_f16x3_tile_scaling_edge_cases,
            test_linear_mfma_vs_fp64); a term of the sum sees that error twice, in its own logit and in the row maximum it is taken against;
  2^-24 sqrt(R)   the floor of the sum over rays those same tests use;
  2^-20     the header's figure for the 24-bit grid of MMA_F16X3;
  T_b 2^-125      v_exp_f32 results below fp32's normal range are flushed: once in the exponential, once in the product with 1/Z;
  A[r]      the clamp allowance, MMA_F16X3 only: that mode stores a logit more than 32 below the largest of its lane's 64 rays of the 128-ray
            tile as that maximum minus 32, so a ray's term can be too large by e^-32 of that maximum's term.  A[r] = e^-32 sum_t max_{r' in
            the 128-ray tile of r} p64[t][r'], from the fp64 probabilities.  Layout-free: the lane's 64 rays are a subset of the tile, so this
            is never tighter than what the kernel does.

Top-k rule.  idx / val are exactly the kernel's own scores under (value desc, index asc); every fp64 top-k ray must be returned whose fp64
score exceeds the (k+1)-th by more than the sum of the two rays' bounds (must_set())."""
import math
from collections import namedtuple

import torch

D = 384
MAX_TOKENS = 256
TILE = 128                       # rays per scale tile of the key planes = the tile of the clamp allowance
TOPK = 100
SQRT_D = math.sqrt(384.0)
FLUSH = 2.0 ** -125              # per token: two flushes of at most 2^-126
L24_GRID = 2.0 ** -20            # include/sixdgs.h at SIXDGS_MMA_F16X3
CLAMP = 32.0                     # the 24-bit grid ends 32 below the lane's maximum
LOGIT_ERR = 4e-7                 # per logit, relative to sum |q||key| / sqrt(384)

MODES = ("MMA_F32", "MMA_BF16X6", "MMA_F16X3", "MMA_F16X3_L32")
PLANE_MODES = ("MMA_F16X3", "MMA_F16X3_L32")
FP32_KEY_MODES = ("MMA_F32", "MMA_BF16X6")
L24_MODE = "MMA_F16X3"

Ref = namedtuple("Ref", "scores rowmax sumexp allow bmax")


def decode(planes, scale, r):
    """fp64 [r,384] keys from the scaled fp16 planes (uint8 [r,1536]: [12 slabs][h, l][32]) and the reciprocal scale of every 128-row tile."""
    pl = planes.view(torch.float16).view(r, 12, 2, 32).double()
    return (pl[:, :, 0] + pl[:, :, 1]).reshape(r, D) * scale.double().repeat_interleave(TILE)[:r, None]


def reference(q, n_tok, key, dtype=torch.float64, chunk=32768):
    """Ref(scores [B,R], rowmax [B,256], sumexp [B,256], allow [B,R], bmax [B]) in `dtype`, on the device of q.  Rows of rowmax / sumexp at or
    beyond the token count are (-inf, 0); an image without tokens has all-zero scores.  Chunked over the rays (whole 128-ray tiles per chunk):
    never more than [T, chunk] at once."""
    assert chunk % TILE == 0
    n_tok = [int(t) for t in n_tok]
    r, dev = key.shape[0], q.device
    scores = torch.zeros(len(n_tok), r, dtype=dtype, device=dev)
    allow = torch.zeros(len(n_tok), r, dtype=dtype, device=dev)
    rowmax = torch.full((len(n_tok), MAX_TOKENS), -math.inf, dtype=dtype, device=dev)
    sumexp = torch.zeros(len(n_tok), MAX_TOKENS, dtype=dtype, device=dev)
    bmax = []
    for b, t in enumerate(n_tok):
        if t == 0 or r == 0:
            bmax.append(0.0)
            continue
        qb = q[b, :t].to(dtype)
        mx = torch.full((t,), -math.inf, dtype=dtype, device=dev)
        se = torch.zeros(t, dtype=dtype, device=dev)
        bm = 0.0
        for r0 in range(0, r, chunk):
            kc = key[r0:r0 + chunk].to(dtype)
            lg = (qb @ kc.T) / SQRT_D
            mn = torch.maximum(mx, lg.amax(1))
            se = se * torch.exp(mx - mn) + torch.exp(lg - mn[:, None]).sum(1)
            mx = mn
            bm = max(bm, float((qb.abs() @ kc.abs().T).max()) / SQRT_D)
        for r0 in range(0, r, chunk):
            kc = key[r0:r0 + chunk].to(dtype)
            p = torch.exp((qb @ kc.T) / SQRT_D - mx[:, None]) / se[:, None]
            n = p.shape[1]
            scores[b, r0:r0 + n] = p.sum(0)
            pad = (-n) % TILE
            pp = torch.nn.functional.pad(p, (0, pad)) if pad else p              # p >= 0: zeros do not raise a tile's maximum
            tile_max = pp.view(t, -1, TILE).amax(2).sum(0)                       # [tiles]: sum_t max_{r' in tile} p[t][r']
            allow[b, r0:r0 + n] = math.exp(-CLAMP) * tile_max.repeat_interleave(TILE)[:n]
        rowmax[b, :t], sumexp[b, :t] = mx, se
        bmax.append(bm)
    return Ref(scores, rowmax, sumexp, allow, bmax)


def e32_of(s32, s64, t):
    """Largest per-ray relative error of the fp32 restatement, after the absolute allowance every fp32 evaluation gets (module docstring)."""
    if t == 0 or s64.numel() == 0:
        return 0.0
    return float((((s32.double() - s64).abs() - t * FLUSH).clamp_min(0.0) / s64).max())


def eps_of(e32, bmax, r, mode):
    return 4.0 * e32 + 2.0 * LOGIT_ERR * bmax + 2.0 ** -24 * math.sqrt(r) + (L24_GRID if mode == L24_MODE else 0.0)


def score_bound(s64, allow, eps, t, mode):
    """The per-ray bound [R] (fp64) on |s_kernel - s64|."""
    a = allow if mode == L24_MODE else torch.zeros_like(allow)
    return eps * s64 + a * (1.0 + eps) + t * FLUSH


def order_of(s, k=TOPK):
    """Indices of the k largest under (value desc, index asc)."""
    return torch.sort(s, descending=True, stable=True).indices[:k]


def must_set(s64, bound, k=TOPK):
    """(fp64 top-k in order, those of them every correct scorer must return).  With no more than k rays every ray is returned by construction."""
    order = order_of(s64, k + 1)
    if s64.numel() <= k:
        return order, order
    top, nxt = order[:k], order[k]
    return top, top[(s64[top] - s64[nxt]) > (bound[top] + bound[nxt])]


def clamped_rays(q_row, key):
    """bool [R] (fp64 logits of ONE token): rays more than 32 below the largest logit of their 128-ray tile.  (The kernel clamps against the
    maximum of the lane's 64 rays, which is no larger: every ray the kernel clamps is among these.)"""
    lg = (key.double() @ q_row.double()) / SQRT_D
    r = lg.numel()
    pad = (-r) % TILE
    lp = torch.nn.functional.pad(lg, (0, pad), value=-math.inf)
    tmax = lp.view(-1, TILE).amax(1).repeat_interleave(TILE)[:r]
    return (tmax - lg) > CLAMP


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
# Keys N(0, 0.07^2); q N(0, qs^2): qs = 0.7 / 45 / 170 give a logit sigma of about 0.05 / 3.2 / 12 (flat, mid, peaked).
QS = (0.7, 45.0, 170.0)
TOKEN_EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
RAY_EDGES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 513)


def _case(name, r, n_tok, qs, seed, modes=MODES, parity=True, undecided_modes=()):
    """parity: the case is held to the per-ray bound and the top-k rule.  undecided_modes: modes in which the rule need not decide MIN_MUST rays."""
    return dict(name=name, r=r, n_tok=tuple(n_tok), qs=qs, seed=seed, modes=tuple(modes), parity=parity, undecided_modes=tuple(undecided_modes))


# (seed 14, not 13: with 13 the single-token image of the peaked case has 7 of its top 100 within the clamp allowance of the 101st in MMA_F16X3)
TOKEN_CASES = [_case(f"tokens_qs{qs:g}", 300, TOKEN_EDGES, qs, seed) for qs, seed in zip(QS, (11, 12, 14))]
RAY_CASES = [_case(f"rays_{r}", r, (200, 3), QS[i % 3], 100 + r) for i, r in enumerate(RAY_EDGES)]
GROUP_CASES = [
    _case("f16_groups_15", 256 * 15, (200, 3), 45.0, 31),                 # k_merge_stats: 15 of its 16 lanes hold a group (fp16 path)
    _case("f16_groups_17", 256 * 16 + 1, (200, 3), 170.0, 32),            # 17 groups, an odd number of 128-ray tiles (33)
    _case("f32_groups_15", 128 * 15, (200, 3), 170.0, 33),                # the same around 16 groups of k_logits
    _case("f32_groups_17", 128 * 16 + 1, (200, 3), 0.7, 34),              # = 2049 rays
    _case("f16_257_tiles", 65537, (129, 3), 45.0, 35),                    # 257 256-ray tiles over 256 groups: unequal runs, groups without a tile
]
LARGE_CASE = _case("beyond_2048_tiles", 262144 + 129, (129, 3), 45.0, 36, modes=FP32_KEY_MODES)   # 2050 tiles: 2 per group, 1025 groups
ROUTES_CASE = _case("routes", 1189, (256, 137, 1, 200, 0), 45.0, 37, parity=False)
IGNORED_CASE = _case("ignored_rows", 300, (1, 100, 129), 45.0, 38, parity=False)
CLAMP_CASE = _case("clamp", 300, (1,), 290.0, 5, undecided_modes=(L24_MODE,))      # the allowance A[r] is what that mode's rays differ by
CASES = TOKEN_CASES + RAY_CASES + GROUP_CASES + [LARGE_CASE, ROUTES_CASE, IGNORED_CASE, CLAMP_CASE]
MIN_MUST = 95                    # of the 100 fp64 top rays of a parity image, at least this many are decided by the rule
MIN_CLAMPED = 50                 # of the clamp case's fp64 top 100, at least this many lie beyond the 24-bit grid
MAX_EPS = 1e-3                   # no case may come with a bound that is slack for another reason (an fp32 restatement that lost a ray)
IGNORED_FILLS = ("zeros", "noise", "huge", "nan", "inf")


def make_inputs(case):
    """(key [R,384], q [B,256,384] with zero rows at or beyond the token count) on the CPU, from the case's seed."""
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    key = torch.randn(case["r"], D, generator=g) * 0.07
    q = torch.randn(len(case["n_tok"]), MAX_TOKENS, D, generator=g) * case["qs"]
    for b, t in enumerate(case["n_tok"]):
        q[b, t:] = 0.0
    return key, q


def fill_ignored(q, n_tok, fill, qs, seed=0):
    """A copy of q whose rows at or beyond the token counts hold: zeros; noise of the real rows' scale; finite values 2^30 times that scale;
    NaN; +-Inf (alternating)."""
    q = q.clone()
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    for b, t in enumerate(n_tok):
        n = MAX_TOKENS - t
        if fill == "zeros":
            q[b, t:] = 0.0
        elif fill == "noise":
            q[b, t:] = torch.randn(n, D, generator=g) * qs
        elif fill == "huge":
            q[b, t:] = torch.randn(n, D, generator=g) * (qs * 2.0 ** 30)
        elif fill == "nan":
            q[b, t:] = math.nan
        elif fill == "inf":
            sign = torch.where((torch.arange(n * D) % 2 == 0), 1.0, -1.0).view(n, D)
            q[b, t:] = sign * math.inf
        else:
            raise ValueError(fill)
    return q


def image_figures(ref64, ref32, b, t, r, mode):
    """(e32, eps, bound [R]) of image b of a case from its fp64 reference and fp32 restatement."""
    e32 = e32_of(ref32.scores[b], ref64.scores[b], t)
    eps = eps_of(e32, ref64.bmax[b], r, mode)
    return e32, eps, score_bound(ref64.scores[b], ref64.allow[b], eps, t, mode)
