"""CPU checks of tests/two_pass_reference.py, the yardstick of test_gpu_two_pass_edges.py: the reference against the oracle and the g5_scorer
fixtures, every term of the bound on cases worked by hand, and the conditions on the case table that keep any GPU test from hiding a failure
behind a slack bound or an undecided top-k.  Also what the library says about the scorer's workspace, without a GPU."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import two_pass_reference as R    # noqa: E402


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle(oracle):
    rng = np.random.default_rng(3)
    key = (rng.standard_normal((300, 384)) * 0.07).astype(np.float32)
    q = np.zeros((2, 256, 384), np.float32)
    q[0, :37] = rng.standard_normal((37, 384)).astype(np.float32) * 45.0
    q[1, :200] = rng.standard_normal((200, 384)).astype(np.float32) * 0.7
    for chunk in (32768, 128):      # one chunk, and three with a ragged last one
        ref = R.reference(torch.from_numpy(q), (37, 200), torch.from_numpy(key), torch.float64, chunk=chunk)
        for b, t in enumerate((37, 200)):
            s, mx, sm = oracle.attention_scores(q[b, :t], key, return_stats=True)
            assert rel_err(ref.scores[b].numpy(), s) < 1e-5
            assert np.abs(ref.rowmax[b, :t].numpy() - mx).max() < 1e-4 and rel_err(ref.sumexp[b, :t].numpy(), sm) < 1e-5
            assert abs(float(ref.scores[b].sum()) - t) < 1e-9 * t
            assert bool(torch.isinf(ref.rowmax[b, t:]).all()) and bool((ref.sumexp[b, t:] == 0).all())
    one = R.reference(torch.from_numpy(q), (37, 200), torch.from_numpy(key), torch.float64)
    assert torch.allclose(one.scores, ref.scores, rtol=1e-12, atol=0) and torch.allclose(one.allow, ref.allow, rtol=1e-12, atol=0)
    assert one.bmax == pytest.approx(ref.bmax, rel=1e-12)


@pytest.mark.parametrize("tag,T,scale", [("flat256", 256, 1.0), ("peaky256", 256, 40.0), ("peaky137", 137, 40.0), ("mid1", 1, 10.0)])
def test_reference_agrees_with_the_scores64_fixtures(oracle, golden, syn, tag, T, scale):
    g = golden("g5_scorer")
    sd = syn.make_scorer_state_dict(0)
    rays = syn.make_rays(4096, 0)
    _, key = oracle.ray_features(rays["ori"], rays["dir"], rays["rgb"], sd)
    q = np.zeros((1, 256, 384), np.float32)
    q[0, :T] = oracle.q_proj(syn.make_tokens(T, 1, scale), sd)
    ref = R.reference(torch.from_numpy(q), (T,), torch.from_numpy(key), torch.float64)
    assert rel_err(ref.scores[0].numpy(), g[f"{tag}_scores64"]) < 1e-5
    assert np.abs(ref.rowmax[0, :T].numpy() - g[f"{tag}_rowmax"]).max() < 1e-4


def test_reference_and_every_bound_term_by_hand():
    # two tokens, two rays: token 0 has logits (a, 0), token 1 (0, 0)
    a = 3.0
    q = torch.zeros(1, 256, 384, dtype=torch.float64)
    key = torch.zeros(2, 384, dtype=torch.float64)
    q[0, 0, 0] = math.sqrt(384.0) * 2.0
    key[0, 0] = a / 2.0
    ref = R.reference(q, (2,), key, torch.float64)
    p0 = 1.0 / (1.0 + math.exp(-a))
    assert ref.scores[0].tolist() == pytest.approx([p0 + 0.5, 1.0 - p0 + 0.5], rel=1e-12)
    assert ref.rowmax[0, :2].tolist() == pytest.approx([a, 0.0], abs=1e-12) and ref.sumexp[0, :2].tolist() == pytest.approx([1.0 + math.exp(-a), 2.0], rel=1e-12)
    assert ref.bmax[0] == pytest.approx(a, rel=1e-12)
    assert ref.allow[0].tolist() == pytest.approx([math.exp(-32.0) * (p0 + 0.5)] * 2, rel=1e-12)      # one tile: the larger probability of each token
    # eps: 4 e32 + 8e-7 B + 2^-24 sqrt(R), + 2^-20 on the 24-bit grid only
    want = 4 * 1e-7 + 8e-7 * 2.0 + 2.0 ** -24 * 16.0
    for mode in R.MODES:
        assert R.eps_of(1e-7, 2.0, 256, mode) == pytest.approx(want + (2.0 ** -20 if mode == "MMA_F16X3" else 0.0), rel=1e-12)
    # e32: per ray, relative, after T 2^-125 absolute -- the second ray is below fp32's range and was flushed by the restatement
    s64 = torch.tensor([1.0, 1e-40, 0.25], dtype=torch.float64)
    s32 = torch.tensor([1.0 + 2.0 ** -20, 0.0, 0.25 * (1 - 2.0 ** -19)], dtype=torch.float64)
    assert R.e32_of(s32, s64, 1) == pytest.approx(2.0 ** -19, rel=1e-9)
    assert R.e32_of(s32, s64, 0) == 0.0
    # the bound: eps s + A (1 + eps) + T 2^-125, A on the 24-bit grid only
    al = torch.tensor([1e-3, 0.0, 2e-3], dtype=torch.float64)
    b24 = R.score_bound(s64, al, 1e-5, 3, "MMA_F16X3")
    assert b24.tolist() == pytest.approx([1e-5 + 1e-3 * (1 + 1e-5) + 3 * 2.0 ** -125, 1e-45 + 3 * 2.0 ** -125, 0.25e-5 + 2e-3 * (1 + 1e-5) + 3 * 2.0 ** -125], rel=1e-12)
    for mode in ("MMA_F32", "MMA_BF16X6", "MMA_F16X3_L32"):
        assert R.score_bound(s64, al, 1e-5, 3, mode).tolist() == pytest.approx([1e-5 + 3 * 2.0 ** -125, 1e-45 + 3 * 2.0 ** -125, 0.25e-5 + 3 * 2.0 ** -125], rel=1e-12)
    # the top-k rule, k = 2 of 4: ray 0 clears the third by more than both bounds, ray 3 does not; ties go to the lower index
    s = torch.tensor([1.0, 0.1, 0.5, 0.6], dtype=torch.float64)
    top, must = R.must_set(s, torch.full((4,), 0.06, dtype=torch.float64), 2)
    assert top.tolist() == [0, 3] and must.tolist() == [0]
    top, must = R.must_set(s, torch.full((4,), 0.04, dtype=torch.float64), 2)
    assert must.tolist() == [0, 3]
    assert R.order_of(torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0]), 4).tolist() == [1, 2, 4, 3]
    top, must = R.must_set(s, torch.ones(4, dtype=torch.float64), 4)      # no more rays than k: every ray is returned whatever its bound
    assert sorted(must.tolist()) == [0, 1, 2, 3]


def test_clamp_allowance_on_two_tiles_of_which_one_clamps():
    """One token, 256 rays.  Tile 0: one ray at logit 0, the others 40 below (beyond the grid's 32); tile 1: all rays at -10 (nothing to clamp)."""
    q = torch.zeros(1, 256, 384, dtype=torch.float64)
    key = torch.zeros(256, 384, dtype=torch.float64)
    q[0, 0, 0] = math.sqrt(384.0)
    key[1:128, 0] = -40.0
    key[128:, 0] = -10.0
    ref = R.reference(q, (1,), key, torch.float64)
    z = 1.0 + 127 * math.exp(-40.0) + 128 * math.exp(-10.0)
    assert ref.sumexp[0, 0].item() == pytest.approx(z, rel=1e-12)
    assert ref.allow[0, :128].tolist() == pytest.approx([math.exp(-32.0) / z] * 128, rel=1e-13)
    assert ref.allow[0, 128:].tolist() == pytest.approx([math.exp(-42.0) / z] * 128, rel=1e-13)
    deep = R.clamped_rays(q[0, 0], key)
    assert deep.tolist() == [False] + [True] * 127 + [False] * 128            # exactly tile 0 clamps
    # what a scorer on the clamped logits reports: too large in tile 0 by less than A, unchanged in tile 1
    lg = key[:, 0].double()
    tmax = torch.cat([lg[:128].max().expand(128), lg[128:].max().expand(128)])
    s_cl = torch.exp(torch.maximum(lg, tmax - 32.0)) / z
    over = s_cl - ref.scores[0]
    ulp = 1e-14 * ref.scores[0]                                                 # fp64 rounding of this very check
    assert bool((over >= -ulp).all()) and bool((over <= ref.allow[0] + ulp).all()) and bool((over[128:].abs() <= ulp[128:]).all())
    assert float(over[1:128].min()) > 0.99 * math.exp(-32.0) / z                # ... and by nearly all of A: the allowance is not slack
    b24 = R.score_bound(ref.scores[0], ref.allow[0], 1e-6, 1, "MMA_F16X3")
    b32 = R.score_bound(ref.scores[0], ref.allow[0], 1e-6, 1, "MMA_F16X3_L32")
    assert bool((over <= b24).all()) and not bool((over[1:128] <= b32[1:128]).any())     # without A the clamp is a failure


# ---- conditions on the case table --------------------------------------------------------------------------------------------------------
HOST_CASES = [c for c in R.CASES if c["parity"] and c["r"] <= 70000]      # the 262 273-ray case asserts the same conditions where it runs, on the GPU


def test_case_table_is_the_one_the_issue_asks_for():
    names = [c["name"] for c in R.CASES]
    assert len(set(names)) == len(names)
    assert all(c["n_tok"] == R.TOKEN_EDGES and c["r"] == 300 for c in R.TOKEN_CASES) and sorted(c["qs"] for c in R.TOKEN_CASES) == [0.7, 45.0, 170.0]
    assert R.TOKEN_EDGES == (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
    assert tuple(c["r"] for c in R.RAY_CASES) == (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 513)
    assert all(c["n_tok"] == (200, 3) for c in R.RAY_CASES) and {c["qs"] for c in R.RAY_CASES} == {0.7, 45.0, 170.0}
    assert {c["r"] for c in R.GROUP_CASES} == {256 * 15, 256 * 16 + 1, 128 * 15, 128 * 16 + 1, 2049, 65537}
    assert all(c["modes"] == R.MODES for c in R.TOKEN_CASES + R.RAY_CASES + R.GROUP_CASES + [R.ROUTES_CASE, R.IGNORED_CASE, R.CLAMP_CASE])
    assert [c for c in R.GROUP_CASES if c["r"] == 65537][0]["n_tok"] == (129, 3)
    assert R.LARGE_CASE["r"] == 262144 + 129 and R.LARGE_CASE["n_tok"] == (129, 3) and R.LARGE_CASE["modes"] == ("MMA_F32", "MMA_BF16X6")
    assert R.ROUTES_CASE["r"] == 1189 and len(R.ROUTES_CASE["n_tok"]) == 5
    assert R.IGNORED_CASE["r"] == 300 and R.IGNORED_CASE["n_tok"] == (1, 100, 129)
    assert (R.CLAMP_CASE["r"], R.CLAMP_CASE["n_tok"], R.CLAMP_CASE["qs"]) == (300, (1,), 290.0)
    assert R.MIN_MUST == 95 and R.MIN_CLAMPED == 50 and R.TOPK == 100
    assert all(c["undecided_modes"] == () for c in R.CASES if c is not R.CLAMP_CASE) and R.CLAMP_CASE["undecided_modes"] == ("MMA_F16X3",)


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["name"])
def test_no_case_can_hide_a_failure(case):
    """In every image of every parity case, in every mode: eps stays below MAX_EPS (the fp32 restatement lost no ray) and at least 95 of the 100 fp64
    top rays are in the must-set (all of them where there are no more rays than k).  On the fp32 keys: the plane modes' decoded keys differ from
    them by 2^-22 of a tile's largest, which moves no count here by more than a ray -- the GPU tests assert both conditions again on their own operands."""
    key, q = R.make_inputs(case)
    ref64 = R.reference(q, case["n_tok"], key, torch.float64)
    ref32 = R.reference(q, case["n_tok"], key, torch.float32)
    for b, t in enumerate(case["n_tok"]):
        if t == 0:
            assert bool((ref64.scores[b] == 0).all())
            continue
        for mode in case["modes"]:
            e32, eps, bound = R.image_figures(ref64, ref32, b, t, case["r"], mode)
            top, must = R.must_set(ref64.scores[b], bound, R.TOPK)
            assert eps <= R.MAX_EPS, (case["name"], b, mode, e32, eps)
            if mode not in case["undecided_modes"]:
                assert must.numel() >= min(R.MIN_MUST, top.numel()), (case["name"], b, mode, must.numel())


def test_clamp_case_reaches_beyond_the_grid():
    case = R.CLAMP_CASE
    key, q = R.make_inputs(case)
    ref64 = R.reference(q, case["n_tok"], key, torch.float64)
    top = R.order_of(ref64.scores[0], R.TOPK)
    deep = R.clamped_rays(q[0, 0], key)
    lg = (key.double() @ q[0, 0].double()) / R.SQRT_D
    print(f"clamp case: {int(deep[top].sum())} of the fp64 top 100 more than 32 below their tile's maximum; logits span {float(lg.max() - lg.min()):.1f}, "
          f"the 100th is {float(lg.max() - lg[top[-1]]):.1f} below the largest")
    assert int(deep[top].sum()) >= R.MIN_CLAMPED
    assert float(lg.max() - lg[top[-1]]) > 40.0          # the unclamped modes have to order scores far below e^-32 of the largest


def test_ignored_fills_leave_the_real_rows_alone():
    case = R.IGNORED_CASE
    _, q = R.make_inputs(case)
    for fill in R.IGNORED_FILLS:
        f = R.fill_ignored(q, case["n_tok"], fill, case["qs"])
        for b, t in enumerate(case["n_tok"]):
            assert torch.equal(f[b, :t], q[b, :t])
            tail = f[b, t:]
            if fill == "zeros":
                assert bool((tail == 0).all())
            elif fill == "noise":
                assert 0.9 * case["qs"] < float(tail.std()) < 1.1 * case["qs"]
            elif fill == "huge":
                assert bool(torch.isfinite(tail).all()) and 0.9 < float(tail.std()) / (case["qs"] * 2.0 ** 30) < 1.1
            elif fill == "nan":
                assert bool(torch.isnan(tail).all())
            else:
                assert bool(torch.isinf(tail).all()) and bool((tail > 0).any()) and bool((tail < 0).any())


# ---- what the library says without a GPU -------------------------------------------------------------------------------------------------
def test_workspace_sizes_of_the_table():
    lib = importlib.import_module("6dgs_amd._lib").load()
    ops = importlib.import_module("6dgs_amd.ops")
    for r in sorted({c["r"] for c in R.CASES}):
        plain = [lib.sixdgs_score_topk_workspace_bytes(r, b, R.TOPK) for b in range(1, 18)]
        l24 = [lib.sixdgs_score_topk_workspace_bytes_ex(r, b, R.TOPK, ops.MMA_F16X3, 1) for b in range(1, 18)]
        l32 = [lib.sixdgs_score_topk_workspace_bytes_ex(r, b, R.TOPK, ops.MMA_F16X3_L32, 1) for b in range(1, 18)]
        for sizes in (plain, l24, l32):
            assert all(x < y for x, y in zip(sizes, sizes[1:])), (r, sizes)          # monotone in the batch
        assert all(a < b for a, b in zip(l24, l32)), r                               # the 24-bit figure is the smaller one
        assert l32 == plain                                                          # "enough for every mode" is the fp32 figure
        assert lib.sixdgs_score_topk_workspace_bytes_ex(r, 1, R.TOPK, ops.MMA_DEFAULT, 1) == l24[0]
        assert lib.sixdgs_score_topk_workspace_bytes_ex(r, 1, R.TOPK, ops.MMA_F16X3, 0) == plain[0]      # no planes: fp32 logits
