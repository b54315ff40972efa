"""The select sweep on 16x16x32 MFMAs (the default) against the 32x32x16 form (SIXDGS_SWEEP_MFMA=32) and against fp64, at the edges the new
shape adds: 16-row token blocks, 16-ray blocks with 4 lane groups, a 4-step butterfly and a 4-group token merge.

Reference.  As tests/test_gpu_select_contract.py: the keys DECODED from the scaled fp16 planes, q in fp64.  With the sweep's own exponent
offsets c_t (SelectStream.ctok after begin(): -ref_t log2e - log2(f Z~_t), -inf beyond the token count)
    e[t][r] = 2^(logit[t][r] log2e + c_t),    U[r] = sum_t e[t][r],    g_t = sum_r e[t][r]
in fp64 on the GPU, chunked over the rays.

Bound.  k_sel_bounds' own eps = 1.4e-4 x + 1.3e-5 with x = max_t |q_t| max_r |k_r| / sqrt(384) (csrc/score.hip: kEpsPerX, kEpsConst; derived
there for 1152 products in any order, so it does not depend on the MFMA shape) bounds every e[t][r] and therefore U[r], relative.  The eps
covers token sums of depth <= 10; g_t sums up to R rays, each addition adding at most u = 2^-24 relative to the (positive) running sum, and the
additions one g_t goes through are the contract test's count D = 255 (a tile) + tiles of a run + 80 (the merge) + 1; plus q's plane split
against the fp32 q of the reference (2^-21 x, as in the contract test's eps_r).  So
    |U - U_ref| <= (eps + 2^-21 x) U_ref,   |g - g_ref| <= (eps + 2^-21 x + D u) g_ref,   and the two shapes within twice that of each other.
Every figure is printed before it is asserted."""
import importlib
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U24 = 2.0 ** -24
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = importlib.import_module("6dgs_amd.ops")
    o.set_mma_mode(o.MMA_DEFAULT)
    return o


@pytest.fixture
def shape_env():
    """Sets the sweep's developer switches for one call and restores them (the library reads them at every launch, the sibling mode once
    per process -- that one is chosen by the slot count instead: a launch of one slot always takes the one-shot grid)."""
    saved = {k: os.environ.get(k) for k in ("SIXDGS_SWEEP_MFMA",)}

    def use(shape):
        if shape == 32:
            os.environ["SIXDGS_SWEEP_MFMA"] = "32"
        else:
            os.environ.pop("SIXDGS_SWEEP_MFMA", None)
    yield use
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def decode(planes, scale, r):
    pl = planes.view(torch.float16).view(r, 12, 2, 32).double()
    return (pl[:, :, 0] + pl[:, :, 1]).reshape(r, 384) * scale.double().repeat_interleave(128)[:r, None]


def reference(q, n_tok, keyd, ctok, chunk=65536):
    """fp64 (U [B,R], g [B,256], x [B]) for the sweep's own offsets ctok."""
    r = keyd.shape[0]
    kmax = float(keyd.norm(dim=1).max())
    inv = 1.0 / math.sqrt(384.0)
    us, gs, xs = [], [], []
    for b, t in enumerate(n_tok):
        u = torch.zeros(r, dtype=torch.float64, device=keyd.device)
        g = torch.zeros(256, dtype=torch.float64, device=keyd.device)
        x = 0.0
        if t > 0:
            qb = q[b, :t].double()
            cb = ctok[b, :t].double()
            for r0 in range(0, r, chunk):
                e = torch.exp2((qb @ keyd[r0:r0 + chunk].T) * (inv * LOG2E) + cb[:, None])
                u[r0:r0 + chunk] = e.sum(0)
                g[:t] += e.sum(1)
            x = float(qb.norm(dim=1).max()) * kmax * inv
        us.append(u), gs.append(g), xs.append(x)
    return torch.stack(us), torch.stack(gs), xs


def make_case(ops, r, seed, q_scale, n_tok):
    g = torch.Generator(device="cpu").manual_seed(seed)
    key = torch.randn(r, 384, generator=g) * 0.07
    q = torch.randn(len(n_tok), 256, 384, generator=g) * q_scale
    for b, t in enumerate(n_tok):
        q[b, t:] = 0.0
    key, q = key.cuda(), q.cuda()
    nt = torch.tensor(n_tok, dtype=torch.int32, device="cuda")
    planes, scale = ops.split_planes_f16(key)
    si = ops.select_sample_indices(r, "cuda") if r >= ops.SELECT_SAMPLE_STRIDE else torch.tensor([r // 2], device="cuda")
    s_planes, s_scale = ops.split_planes_f16(key[si].contiguous())
    return dict(r=r, q=q, nt=nt, n_tok=list(n_tok), planes=planes, scale=scale, s_planes=s_planes, s_scale=s_scale)


def sweep(ops, c, use, shape):
    use(shape)
    ss = ops.SelectStream(c["q"], c["nt"], c["r"], 100, 4096, c["n_tok"])
    ss.begin(c["s_planes"], c["s_scale"])
    ss.sweep(c["planes"], c["scale"], 0)
    torch.cuda.synchronize()
    return ss.u[:, :c["r"]].clone(), ss.gsum.clone(), ss.ctok.clone()


def check_case(ops, c, use, tag):
    u16, g16, ctok = sweep(ops, c, use, 16)
    u32, g32, ctok32 = sweep(ops, c, use, 32)
    assert torch.equal(torch.nan_to_num(ctok, neginf=-1e30), torch.nan_to_num(ctok32, neginf=-1e30)), f"{tag}: the pre-pass must not depend on the sweep's shape"
    u_ref, g_ref, xs = reference(c["q"], c["n_tok"], decode(c["planes"], c["scale"], c["r"]), ctok)
    d = 255 + math.ceil(c["r"] / 65536) + 1 + 80 + 1
    worst = 0.0
    for b, t in enumerate(c["n_tok"]):
        if t == 0:                                    # no tokens: nothing is summed (the contract test covers what such an image returns)
            continue
        eps = 1.4e-4 * xs[b] + 1.3e-5 + 2.0 ** -21 * xs[b]
        eps_g = eps + d * U24
        assert bool((g16[b, t:] == 0).all()) and bool((g32[b, t:] == 0).all()), f"{tag} image {b}: g_t beyond the token count"
        fig = []
        for name, u, g in (("16x16x32", u16, g16), ("32x32x16", u32, g32)):
            eu = float(((u[b].double() - u_ref[b]).abs() / u_ref[b]).max()) / eps
            eg = float(((g[b, :t].double() - g_ref[b, :t]).abs() / g_ref[b, :t]).max()) / eps_g
            fig.append((name, eu, eg))
        du = float(((u16[b].double() - u32[b].double()).abs() / u_ref[b]).max()) / (2 * eps)
        dg = float(((g16[b, :t].double() - g32[b, :t].double()).abs() / g_ref[b, :t]).max()) / (2 * eps_g)
        print(f"[sweep shape] {tag} image {b} ({t} tokens, x = {xs[b]:.3g}): " +
              ", ".join(f"{n}: U {eu:.3f} g {eg:.3f} of the bound" for n, eu, eg in fig) + f"; between the shapes: U {du:.3f} g {dg:.3f} of 2 eps")
        for n, eu, eg in fig:
            assert eu <= 1.0 and eg <= 1.0, f"{tag} image {b} {n}: U {eu:.3f}, g {eg:.3f} of the bound"
        assert du <= 1.0 and dg <= 1.0, f"{tag} image {b}: the shapes differ by U {du:.3f}, g {dg:.3f} of 2 eps"
        worst = max(worst, *(max(eu, eg) for _, eu, eg in fig))
    return worst


TOKEN_COUNTS = (1, 15, 16, 17, 31, 64, 65, 137, 256)


@pytest.mark.parametrize("t", TOKEN_COUNTS)
def test_token_counts_at_the_16_row_block_edges(ops, shape_env, t):
    """One image of t tokens (one slot: the one-shot grid) and the same image eight times (eight images, packed by their token counts: the
    persistent grid), R = 4096 + 37."""
    check_case(ops, make_case(ops, 4096 + 37, 11 + t, 6.0, (t,)), shape_env, f"t={t} one image")
    check_case(ops, make_case(ops, 4096 + 37, 12 + t, 6.0, (t,) * 8), shape_env, f"t={t} eight images")


def test_packed_batch_of_mixed_token_counts(ops, shape_env):
    check_case(ops, make_case(ops, 70_001, 5, 6.0, (256, 1, 137, 0, 64, 200, 31, 16, 17, 15, 65)), shape_env, "mixed batch")


@pytest.mark.parametrize("r", [1, 255, 256, 257, 65_536 + 3])
def test_ray_counts_at_the_tile_edges(ops, shape_env, r):
    """Ragged last tiles under the new (lane, register) -> ray map; one slot (one-shot grid) and several (persistent grid)."""
    check_case(ops, make_case(ops, r, 100 + r % 89, 6.0, (200,)), shape_env, f"R={r} one slot")
    check_case(ops, make_case(ops, r, 101 + r % 89, 6.0, (256, 37, 0, 1, 256, 129)), shape_env, f"R={r} packed")


@pytest.mark.parametrize("slots", [1, 4, 8, 12])
def test_slot_counts(ops, shape_env, slots):
    """`slots` images of 256 tokens are `slots` slots of one launch (12: the last launch of a batch takes up to 1.5 x the cap of 8)."""
    check_case(ops, make_case(ops, 40_000 + 3, 40 + slots, 6.0, (256,) * slots), shape_env, f"{slots} slots")


@pytest.mark.parametrize("q_scale", [0.02, 45.0])
def test_score_select_returns_the_old_shapes_top_100(ops, shape_env, q_scale):
    """sixdgs_score_select end to end: the same top-100 in the same order as the 32x32x16 sweep wherever that one's adjacent values differ by
    more than the contract's rho; values within 2 beta (both are within beta of the fp64 score)."""
    c = make_case(ops, 300_001, 7, q_scale, (256, 137, 1, 0, 64))
    out = {}
    for shape in (16, 32):
        shape_env(shape)
        out[shape] = ops.score_select(c["q"], c["nt"], c["planes"], c["scale"], c["s_planes"], c["s_scale"], 100, max_candidates=4096, n_tok_host=c["n_tok"])
        torch.cuda.synchronize()
    (i16, v16, s16), (i32, v32, s32) = out[16], out[32]
    # status = the candidate count (it may move by a few with the rounding of U), or -1: more candidates than the list holds -- in both or in neither
    assert [v < 0 for v in s16.tolist()] == [v < 0 for v in s32.tolist()], (s16.tolist(), s32.tolist())
    keyd = decode(c["planes"], c["scale"], c["r"])
    kmax = float(keyd.norm(dim=1).max())
    for b, t in enumerate(c["n_tok"]):
        if int(s32[b]) < 0:                                   # refused by both (flat scores: the bounds admit more than 4096 candidates): no partial answer
            assert bool((i16[b] == -1).all()) and bool((i32[b] == -1).all()), f"image {b}: a refusal with a partial answer"
            print(f"[sweep shape] select q_scale={q_scale} image {b}: refused by both shapes")
            continue
        if t == 0:
            assert torch.equal(i16[b], i32[b])
            continue
        x = float(c["q"][b, :t].double().norm(dim=1).max()) * kmax / math.sqrt(384.0)
        eps_r = (2.0 ** -21 + 5 * U24) * x + 128 * U24 * math.log(2.0) + 12 * U24
        dd = 255 + math.ceil(c["r"] / 65536) + 1 + 80 + 1
        beta = 1.01 * (eps_r + 1.4e-4 * x + 1.3e-5 + (eps_r - 10 * U24) + dd * U24)
        rho = (1.0 + beta) / (1.0 - beta)
        a, v = i32[b].cpu(), v32[b].double().cpu()
        real = bool((v[:-1] > rho * v[1:]).all())
        dv = float(((v16[b].double().cpu() - v).abs() / v).max()) / (2 * beta) if torch.equal(i16[b].cpu(), a) else float("nan")
        print(f"[sweep shape] select q_scale={q_scale} image {b}: every gap real: {real}, same rays in order: {torch.equal(i16[b].cpu(), a)}, values {dv:.3g} of 2 beta")
        assert set(i16[b].tolist()) == set(a.tolist()) or not real, f"image {b}: other rays than the old shape"
        got = i16[b].cpu()
        for j in range(100):                                   # position j must agree unless it sits in a run of near-ties of the old shape
            tie = (j > 0 and v[j - 1] <= rho * v[j]) or (j < 99 and v[j] <= rho * v[j + 1])
            assert tie or int(got[j]) == int(a[j]), f"image {b} rank {j}: {int(got[j])} != {int(a[j])} across a real gap"
        if torch.equal(got, a):
            assert dv <= 1.0, f"image {b}: values differ by {dv:.3f} of 2 beta"
