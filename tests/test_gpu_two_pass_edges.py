"""The two-pass scorer (sixdgs_score_topk[_ex], sixdgs_score_pass1 / 2: k_logits<MMA>, k_logits_f16x<kAllTerms, kOutL24 | kOutF32>, the q split,
k_merge_stats, k_score_reduce / _blocked / _blocked24) against fp64 at its token, ray and group edges, in the four modes MMA_F32, MMA_BF16X6,
MMA_F16X3 and MMA_F16X3_L32.  Reference, per-ray bound, top-k rule and the case table: tests/two_pass_reference.py (its docstring derives the
bound); test_two_pass_reference_host.py checks on the CPU that no case of the table comes with a bound slack enough to hide a failure.
Every measured figure is printed as a ratio to its bound before it is asserted.  Everything runs inside this process; the modes are chosen
with ops.set_mma_mode and restored."""
import importlib
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import two_pass_reference as R    # noqa: E402

K = R.TOPK


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = importlib.import_module("6dgs_amd.ops")
    o.set_mma_mode(o.MMA_DEFAULT)
    return o


_inputs, _refs = {}, {}


def inputs(ops, case):
    """The case's operands on the GPU, with the key planes and the key decoded from them.  One entry at a time for the large cases."""
    name = case["name"]
    if name not in _inputs:
        if case["r"] > 10000:
            for k in [k for k in _inputs if _inputs[k]["r"] > 10000]:
                del _inputs[k]
        key, q = R.make_inputs(case)
        key, q = key.cuda(), q.cuda()
        planes, scale = ops.split_planes_f16(key)
        _inputs[name] = dict(r=case["r"], key=key, q=q, nt=torch.tensor(case["n_tok"], dtype=torch.int32, device="cuda"), planes=planes, scale=scale)
    return _inputs[name]


def refs(ops, case, mode):
    """(fp64 reference, fp32 restatement) of the case for the operands the mode multiplies, computed once on the GPU and left unchanged."""
    planes = mode in R.PLANE_MODES
    if (case["name"], planes) not in _refs:
        c = inputs(ops, case)
        key = R.decode(c["planes"], c["scale"], case["r"]) if planes else c["key"]
        _refs[(case["name"], planes)] = (R.reference(c["q"], case["n_tok"], key, torch.float64), R.reference(c["q"], case["n_tok"], key.float(), torch.float32))
    return _refs[(case["name"], planes)]


def run(ops, mode, q, nt, c, **kw):
    """ops.score_topk in `mode` on the case's keys (planes in the plane modes)."""
    planes = mode in R.PLANE_MODES
    ops.set_mma_mode(getattr(ops, mode))
    try:
        out = ops.score_topk(q, nt, c["key"], K, key_planes=c["planes"] if planes else None, key_scale=c["scale"] if planes else None, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_mma_mode(ops.MMA_DEFAULT)
    return out


def check_topk_is_own_order(idx, val, sc, r, tag):
    n = min(r, K)
    order = R.order_of(sc, n)
    assert torch.equal(idx[:n], order), f"{tag}: idx is not the kernel's own scores under (value desc, index asc)"
    assert torch.equal(val[:n], sc[order]), f"{tag}: val is not the score at idx"
    assert bool((idx[n:] == -1).all()) and bool(torch.isnan(val[n:]).all()), f"{tag}: padding beyond min(R, k) must be (-1, NaN)"


def check_image(case, mode, b, ref64, ref32, idx, val, sc, stats, worst):
    """Scores, row statistics and top-k of image b against fp64."""
    t, r = case["n_tok"][b], case["r"]
    tag = f"{case['name']} {mode} image {b} ({t} tokens, {r} rays)"
    check_topk_is_own_order(idx, val, sc, r, tag)
    if t == 0:      # no tokens: an empty sum for every ray, all ties -> the lowest indices (test_score_topk_batched_and_grouped)
        n = min(r, K)
        assert bool((sc == 0).all()) and torch.equal(idx[:n], torch.arange(n, device=idx.device)) and bool((val[:n] == 0).all()), tag
        return
    s64 = ref64.scores[b]
    e32, eps, bound = R.image_figures(ref64, ref32, b, t, r, mode)
    bmax = ref64.bmax[b]
    err = (sc.double() - s64).abs()
    ratio = float((err / bound).max())
    ratio_no_grid = float((err / R.score_bound(s64, ref64.allow[b], eps - R.L24_GRID, t, mode)).max()) if mode == R.L24_MODE else float("nan")
    dmax = float((stats[:t, 0].double() - ref64.rowmax[b, :t]).abs().max()) / (R.LOGIT_ERR * bmax)
    se_k = stats[:t, 1].double() * torch.exp(stats[:t, 0].double() - ref64.rowmax[b, :t])
    dse = float(((se_k - ref64.sumexp[b, :t]).abs() / ref64.sumexp[b, :t]).max()) / eps
    top, must = R.must_set(s64, bound, K)
    missing = [int(i) for i in must.tolist() if i not in set(idx.tolist())]
    print(f"[two-pass edges] {tag}: score err / bound {ratio:.4f} (without the 2^-20 term {ratio_no_grid:.4f}), row max err / (4e-7 B) {dmax:.3f}, "
          f"sumexp err / eps {dse:.3f}; e32 {e32:.3g}, B {bmax:.4g}, eps {eps:.3g}; must-set {must.numel()} of {top.numel()}, missing {len(missing)}")
    worst.append((ratio, ratio_no_grid, dmax, dse, e32, bmax, tag))
    assert eps <= R.MAX_EPS, f"{tag}: eps {eps:.3g}: the case's own bound is slack"
    assert mode in case["undecided_modes"] or must.numel() >= min(R.MIN_MUST, top.numel()), f"{tag}: only {must.numel()} of the fp64 top rays are decided"
    assert ratio <= 1.0, f"{tag}: a score is {ratio:.3f} x its bound from fp64"
    assert dmax <= 1.0, f"{tag}: a row maximum is {dmax:.3f} x 4e-7 B from fp64"
    assert dse <= 1.0, f"{tag}: a row's sumexp is {dse:.3f} x eps from fp64"
    assert not missing, f"{tag}: fp64 top-k rays beyond the bound's reach were not returned: {missing[:5]}"


def check_case(ops, case, mode):
    c = inputs(ops, case)
    ref64, ref32 = refs(ops, case, mode)
    idx, val, sc, stats = run(ops, mode, c["q"], c["nt"], c, want_stats=True)
    worst = []
    for b in range(len(case["n_tok"])):
        check_image(case, mode, b, ref64, ref32, idx[b], val[b], sc[b], stats[b], worst)
    if worst:
        w = max(worst)
        print(f"[two-pass edges] worst of {case['name']} {mode}: score {w[0]:.4f} (no grid term {w[1]:.4f}), e32 {w[4]:.3g}, B {w[5]:.4g} at {w[6]}; "
              f"row max {max(x[2] for x in worst):.3f}, sumexp {max(x[3] for x in worst):.3f}")
    return idx, val, sc, stats


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.TOKEN_CASES, ids=lambda c: c["name"])
def test_token_edges(ops, case, mode):
    """16 images of 0 .. 256 tokens in one call: every 32-token group of the blocked reduce kernels and every 64- / 128-token split of the logits
    kernels, one token either side.  Images of 1, 129 and 256 tokens scored alone give the bits they get inside the batch."""
    c = inputs(ops, case)
    idx, val, sc, stats = check_case(ops, case, mode)
    for t in (1, 129, 256):
        b = case["n_tok"].index(t)
        i1, v1, s1, st1 = run(ops, mode, c["q"][b:b + 1].contiguous(), c["nt"][b:b + 1].contiguous(), c, want_stats=True)
        assert torch.equal(i1[0], idx[b]) and torch.equal(v1[0], val[b]) and torch.equal(s1[0], sc[b]) and torch.equal(st1[0, :t], stats[b, :t]), \
            f"{case['name']} {mode}: the image of {t} tokens scores to other bits alone than in the batch"


@pytest.mark.parametrize("mode", R.MODES)
def test_ray_edges(ops, mode):
    """1 .. 513 rays around every 64 / 128 / 256-ray edge, batch of (200, 3) tokens: the second image's score row starts unaligned whenever
    R % 4 != 0; k = 100 > R pads with (-1, NaN)."""
    for case in R.RAY_CASES:
        check_case(ops, case, mode)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.GROUP_CASES, ids=lambda c: c["name"])
def test_group_structure(ops, case, mode):
    """k_merge_stats around its 16 lanes in both logits paths; 257 tiles over 256 groups in the fp16 path (unequal runs, groups without a tile,
    an empty second half of the last 256-ray tile)."""
    check_case(ops, case, mode)


@pytest.mark.parametrize("mode", R.LARGE_CASE["modes"])
def test_beyond_2048_tiles(ops, mode):
    """2050 128-ray tiles: k_logits walks two tiles per group and k_merge_stats folds 1025 groups.  The fp64 reference runs on the GPU, chunked."""
    check_case(ops, R.LARGE_CASE, mode)
    if mode == R.LARGE_CASE["modes"][-1]:
        _inputs.pop(R.LARGE_CASE["name"], None)      # 0.8 GB of keys and planes: not kept for the rest of the session


@pytest.mark.parametrize("mode", R.MODES)
def test_same_bits_by_other_routes(ops, mode):
    """want_scores=False (scores kept only in the workspace), images_in_flight 1 / 2 / 3 for five images, and score_pass1 + score_pass2 on the
    local statistics all give the bits of the resident fused call."""
    case = R.ROUTES_CASE
    c = inputs(ops, case)
    b, r = len(case["n_tok"]), case["r"]
    idx, val, sc, stats = run(ops, mode, c["q"], c["nt"], c, want_stats=True)
    for i in range(b):
        check_topk_is_own_order(idx[i], val[i], sc[i], r, f"routes {mode} image {i}")
    i0, v0, s0, _ = run(ops, mode, c["q"], c["nt"], c, want_scores=False)
    assert s0 is None and torch.equal(i0, idx) and torch.equal(v0, val), f"{mode}: want_scores=False"
    for n in (1, 2, 3):
        i1, v1, s1, st1 = run(ops, mode, c["q"], c["nt"], c, want_stats=True, images_in_flight=n)
        assert torch.equal(i1, idx) and torch.equal(v1, val) and torch.equal(s1, sc), f"{mode}: images_in_flight={n}"
        for i, t in enumerate(case["n_tok"]):
            assert torch.equal(st1[i, :t], stats[i, :t]), f"{mode}: images_in_flight={n}, statistics of image {i}"
    planes = mode in R.PLANE_MODES
    ops.set_mma_mode(getattr(ops, mode))
    try:
        ws = torch.empty(ops.score_topk_workspace_bytes(r, b, K, planes=planes), dtype=torch.uint8, device="cuda")
        st = ops.score_pass1(c["q"], c["nt"], c["key"], ws, K, key_planes=c["planes"] if planes else None, key_scale=c["scale"] if planes else None)
        i2, v2, s2 = ops.score_pass2(st, c["nt"], r, ws, K, used_planes=planes)
        torch.cuda.synchronize()
    finally:
        ops.set_mma_mode(ops.MMA_DEFAULT)
    for i, t in enumerate(case["n_tok"]):
        assert torch.equal(st[i, :t], stats[i, :t]), f"{mode}: pass 1 statistics of image {i}"
    assert torch.equal(i2, idx) and torch.equal(v2, val) and torch.equal(s2, sc), f"{mode}: score_pass1 + score_pass2"


@pytest.mark.parametrize("mode", R.MODES)
def test_ignored_rows(ops, mode):
    """q rows at or beyond n_tok are not read: whatever they hold -- noise, values 2^30 times the real rows' scale, NaN, +-Inf -- idx, val, scores
    and the statistics of the rows below the token count are those of zero rows, bit for bit, through ops.score_topk and
    ops.ray_attention_scores.  (Before the q split took n_tok, the fp16 x 3 modes chose the scale of a 128-token half from all its rows:
    profiles/two_pass_scorer_edges.md has what that did.)"""
    case = R.IGNORED_CASE
    c = inputs(ops, case)
    q0 = c["q"].cpu()
    want = want_train = None
    bad = []
    for fill in R.IGNORED_FILLS:
        q = R.fill_ignored(q0, case["n_tok"], fill, case["qs"]).cuda()
        idx, val, sc, stats = run(ops, mode, q, c["nt"], c, want_stats=True)
        ops.set_mma_mode(getattr(ops, mode))
        try:
            train = ops.ray_attention_scores(q, c["nt"], c["key"])
            torch.cuda.synchronize()
        finally:
            ops.set_mma_mode(ops.MMA_DEFAULT)
        if fill == "zeros":
            want, want_train = (idx, val, sc, stats), train
            assert torch.equal(train, sc), f"{mode}: ray_attention_scores and score_topk disagree on zero rows"
            continue
        for b, t in enumerate(case["n_tok"]):
            same = dict(idx=torch.equal(idx[b], want[0][b]), val=torch.equal(val[b], want[1][b]), scores=torch.equal(sc[b], want[2][b]),
                        stats=torch.equal(stats[b, :t], want[3][b, :t]), train=torch.equal(train[b], want_train[b]))
            rel = float(((sc[b].double() - want[2][b].double()).abs() / want[2][b].double()).max())
            print(f"[two-pass edges] ignored rows {mode} fill {fill} image {b} ({t} tokens): " + ", ".join(f"{k} {'same' if v else 'DIFFER'}" for k, v in same.items()) +
                  f"; largest relative change of a score {rel:.3g}")
            bad += [f"{fill} image {b}: {k}" for k, v in same.items() if not v]
    assert not bad, f"{mode}: results depend on q rows at or beyond n_tok: {bad}"


@pytest.mark.parametrize("mode", R.MODES)
def test_clamp(ops, mode):
    """One token, logits spread over ~118: most of the fp64 top 100 lie more than 32 below their tile's largest logit.  All modes: the per-ray
    bound and the top-k rule -- in the three unclamped modes the must-set is nearly all 100, so they order scores down to e^-55 of the largest.
    MMA_F16X3 stores such logits as (the lane's maximum - 32): its scores there are too LARGE, never too small, within the allowance A[r]."""
    case = R.CLAMP_CASE
    c = inputs(ops, case)
    ref64, ref32 = refs(ops, case, mode)
    idx, val, sc, stats = check_case(ops, case, mode)
    s64 = ref64.scores[0]
    e32, eps, bound = R.image_figures(ref64, ref32, 0, 1, case["r"], mode)
    top, must = R.must_set(s64, bound, K)
    keyd = R.decode(c["planes"], c["scale"], case["r"]) if mode in R.PLANE_MODES else c["key"]
    deep = R.clamped_rays(c["q"][0, 0], keyd)
    n_deep = int(deep[top].sum())
    low = float(((s64 - sc[0].double() - R.FLUSH) / (eps * s64)).max())
    over = float(((sc[0].double() - s64) / bound)[deep].max())
    print(f"[two-pass edges] clamp {mode}: {n_deep} of the fp64 top {top.numel()} beyond the grid, must-set {must.numel()}, "
          f"(s64 - s) / (eps s64) {low:.3f}, (s - s64) / bound among the clamped rays {over:.3f}")
    assert n_deep >= R.MIN_CLAMPED
    assert low <= 1.0, f"{mode}: a score is below s64 (1 - eps)"
    if mode != R.L24_MODE:
        assert must.numel() >= R.MIN_MUST
