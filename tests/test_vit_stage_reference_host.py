"""CPU checks of tests/vit_stage_reference.py, the yardstick of test_gpu_vit_stage_edges.py: the references against the module's own code
(_Block of 6dgs_amd/backbone.py and F.scaled_dot_product_attention in fp64), every term of the bounds on a 2 x 384 example worked by hand, the
two launch-plan restatements at 256 compute units against values worked out from csrc/vit.hip, and the conditions on the case tables that keep
a GPU test from hiding a failure: torch's own fp32 CPU evaluation of EVERY case lies within the case's bound (starting constants), every
element compared, and the tables hold every row and token count the kernels change path at."""
import importlib
import math
import os
import sys

import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch.nn.functional as F    # noqa: E402
import vit_stage_reference as R    # noqa: E402

START = dict(c_ln=R.C_LN_START, e_erf=R.E_ERF_START)


# ---- the references against the module's own code --------------------------------------------------------------------------------------
def test_references_chain_to_the_modules_block_in_fp64():
    bb = importlib.import_module("6dgs_amd.backbone")
    torch.manual_seed(2)
    blk = bb._Block(384, 6).double().eval()
    with torch.no_grad():
        blk.ls1.gamma.copy_(torch.rand(384) * 0.5 + 0.1)
        blk.ls2.gamma.copy_(torch.randn(384) * 0.5)
        blk.norm1.weight.copy_(torch.rand(384) + 0.5)
        blk.norm1.bias.copy_(torch.randn(384) * 0.1)
        images, tokens = 2, 37
        x = torch.randn(images, tokens, 384, dtype=torch.float64)
        want = blk(x)
        a, p, n1, n2, mlp = blk.attn, blk.attn.proj, blk.norm1, blk.norm2, blk.mlp
        t = x.reshape(-1, 384)
        qkv = R.ref_linear(t, a.qkv.weight, a.qkv.bias, ln=(n1.weight, n1.bias, n1.eps))                                          # (a)
        y = R.ref_attention(qkv, images, tokens, 6)
        t = R.ref_linear(y, p.weight, p.bias, epilogue=R.EPI_RESID, residual=t, gamma=blk.ls1.gamma)                              # (b)
        hid = R.ref_linear(t, mlp.fc1.weight, mlp.fc1.bias, ln=(n2.weight, n2.bias, n2.eps), epilogue=R.EPI_GELU)                 # (c)
        t = R.ref_linear(hid, mlp.fc2.weight, mlp.fc2.bias, epilogue=R.EPI_RESID, residual=t, gamma=blk.ls2.gamma)                # (d)
    assert float((t.view_as(want) - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_reference_attention_is_sdpa_in_fp64_and_by_hand():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(3 * 41, 3 * 128, generator=g)
    q, k, v = qkv.double().view(3, 41, 3, 2, 64).permute(2, 0, 3, 1, 4).unbind(0)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(123, 128)
    assert torch.equal(R.ref_attention(qkv, 3, 41, 2), want)
    # by hand: image 1, head 1, query 5
    lg = (q[1, 1, 5] @ k[1, 1].T) / 8.0
    p = torch.exp(lg - lg.max())
    p = p / p.sum()
    assert torch.allclose(want[41 + 5, 64:], p @ v[1, 1], rtol=1e-12, atol=0)
    lam, s = R.attention_terms(qkv, 3, 41, 2)
    assert float(lam[1, 1, 5]) == pytest.approx(float((q[1, 1, 5].abs() * k[1, 1].abs()).sum(1).max()) / 8.0, rel=1e-12)
    assert float(s[1, 1, 5]) == pytest.approx(float((p * v[1, 1].abs().amax(1)).sum()), rel=1e-12)
    b = R.attention_bound(qkv, 3, 41, 2, c0=2e-6)
    assert float(b.e[41 + 5, 64 + 7]) == pytest.approx((8e-7 * float(lam[1, 1, 5]) + 2e-6) * float(s[1, 1, 5]), rel=1e-12)
    assert float(b.e[41 + 5, 7]) == pytest.approx((8e-7 * float(lam[1, 0, 5]) + 2e-6) * float(s[1, 0, 5]), rel=1e-12)


# ---- every term of the linear bound by hand -----------------------------------------------------------------------------------------------
def test_every_linear_bound_term_by_hand():
    assert R.LOGIT_ERR == 4e-7 and R.U == 2.0 ** -23
    # 2 x 384: row 0 = (3, -1, 0, ...), row 1 = (1, 1, 0, ...); w row 0 = (2, 4, 0, ...), row 1 = (-1, 0, ...); two more zero rows up to n = 4
    x = torch.zeros(2, 384, dtype=torch.float64)
    w = torch.zeros(4, 384, dtype=torch.float64)
    x[0, :2] = torch.tensor([3.0, -1.0], dtype=torch.float64)
    x[1, :2] = 1.0
    w[0, :2] = torch.tensor([2.0, 4.0], dtype=torch.float64)
    w[1, 0] = -1.0
    b = torch.tensor([0.5, -0.25, 0.0, 1.0], dtype=torch.float64)
    fl = lambda s: 2.0 ** -125 * (s + 1.0)      # noqa: E731
    # plain + bias: v = [[2.5, -3.25, 0, 1], [6.5, -1.25, 0, 1]], A = [[10.5, 3.25, 0, 1], [6.5, 1.25, 0, 1]]
    bd = R.linear_bound(x, w, b)
    assert bd.ref.tolist() == [[2.5, -3.25, 0.0, 1.0], [6.5, -1.25, 0.0, 1.0]]
    a = [[10.5, 3.25, 0.0, 1.0], [6.5, 1.25, 0.0, 1.0]]
    for i in range(2):
        for j in range(4):
            want = 4e-7 * a[i][j] + 2.0 ** -23 * abs(bd.ref[i][j].item()) + fl(float(w[j].abs().sum()))
            assert float(bd.e[i, j]) == pytest.approx(want, rel=1e-12)
    # residual + gamma
    res = torch.tensor([[1.0, 2.0, 3.0, 4.0], [-1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    gam = torch.tensor([0.5, -2.0, 1.0, 0.0], dtype=torch.float64)
    br = R.linear_bound(x, w, b, epilogue=R.EPI_RESID, residual=res, gamma=gam)
    assert br.ref[0].tolist() == [1.0 + 0.5 * 2.5, 2.0 + 2.0 * 3.25, 3.0, 4.0]
    assert float(br.e[0, 1]) == pytest.approx(2.0 * float(bd.e[0, 1]) + 2.0 ** -23 * (2.0 + 6.5), rel=1e-12)
    assert float(br.e[0, 3]) == pytest.approx(2.0 ** -23 * 4.0, rel=1e-12)                       # gamma 0: nothing but the residual's rounding
    # GELU
    bg = R.linear_bound(x, w, b, epilogue=R.EPI_GELU, e_erf=1.5e-7)
    y01 = 0.5 * -3.25 * (1.0 + math.erf(-3.25 / math.sqrt(2.0)))
    assert float(bg.ref[0, 1]) == pytest.approx(y01, rel=1e-12)
    assert float(bg.e[0, 1]) == pytest.approx(1.13 * float(bd.e[0, 1]) + 0.5 * 3.25 * 1.5e-7 + 2.0 ** -23 * abs(y01), rel=1e-12)
    # LayerNorm: row 0 has mean 2 / 384, kappa = 3 / sigma
    g = torch.full((384,), 2.0, dtype=torch.float64)
    lb = torch.full((384,), 0.25, dtype=torch.float64)
    bl = R.linear_bound(x, w, b, ln=(g, lb, 1e-6), c_ln=4.0)
    mean = 2.0 / 384
    var = (9.0 + 1.0) / 384 - mean * mean
    sig = math.sqrt(var + 1e-6)
    assert float(R.kappa(x)[0]) == pytest.approx(3.0 / sig, rel=1e-12)
    xh = [(3.0 - mean) / sig * 2.0 + 0.25, (-1.0 - mean) / sig * 2.0 + 0.25]
    assert float(bl.ref[0, 0]) == pytest.approx(2.0 * xh[0] + 4.0 * xh[1] + 0.5, rel=1e-12)
    want = (4e-7 * (2.0 * abs(xh[0]) + 4.0 * abs(xh[1]) + 0.5) + 2.0 ** -23 * abs(float(bl.ref[0, 0])) + fl(6.0)
            + 4.0 * 2.0 ** -23 * (1.0 + 3.0 / sig) * (2.0 * 6.0))
    assert float(bl.e[0, 0]) == pytest.approx(want, rel=1e-12)
    # the shares add up to the bound, in every form
    for bnd in (bd, br, bg, bl):
        assert torch.allclose(sum(t.expand_as(bnd.e) for t in bnd.terms.values()), bnd.e, rtol=1e-12, atol=0)
    # worst / needed
    y = bd.ref.clone()
    y[1, 0] += 0.5 * float(bd.e[1, 0])
    ratio, name = R.worst(y, bd)
    assert ratio == pytest.approx(0.5, rel=1e-9) and name == "product"
    y[0, 2] = 1e-30                                                                               # where the bound is the floor alone
    assert R.worst(y, bd)[0] == pytest.approx(1e-30 / fl(0.0), rel=1e-9)
    y[0, 2] = math.nan
    assert R.worst(y, bd)[0] == math.inf


# ---- the launch plans against csrc/vit.hip, by hand at 256 compute units --------------------------------------------------------------------
def test_plan_restatements_at_256_compute_units():
    # tok_ft_per_wg: per = ceil(ceil(m / 64) * ceil(n / 256) / 256), clamped to [1, tiles]; 1 whenever K > 384
    for (m, n, k), want in {(4112, 1536, 384): 2, (4112, 1152, 384): 2, (4112, 384, 384): 1, (257, 1152, 384): 1, (3264, 1152, 384): 1, (3265, 1152, 384): 2,
                            (6528, 1152, 384): 2, (6529, 1152, 384): 3, (2688, 1536, 384): 1, (2689, 1536, 384): 2, (5440, 1536, 384): 2, (5441, 1536, 384): 3,
                            (4112, 384, 1536): 1, (100000, 384, 1536): 1, (100000, 384, 384): 2, (100000, 128, 384): 1, (65, 640, 768): 1}.items():
        assert R.planned_ft_per_wg(m, n, k, 256) == want, (m, n, k)
    assert R.planned_walk(3265, 1152, 384) == [2, 2, 1] and R.planned_walk(6529, 1152, 384) == [3, 2] and R.planned_walk(5441, 1536, 384) == [3, 3]
    assert R.planned_walk(3265, 1280, 384) == [2, 2, 1] and R.planned_walk(257, 1152, 384) == [1] * 5
    assert [c["m"] for c in R.WALK_CASES] == [3265, 2689, 3265, 6529, 5441, 6529]
    assert all(R.planned_ft_per_wg(m, 384, 1536, cus) == 1 for m in (1, 4112, 10 ** 6) for cus in (1, 64, 256, 304))       # form (d) never walks
    # sixdgs_tok_attention: groups = ceil(tokens / 128), one fewer while images * heads * groups > 256
    for (im, h, t), want in {(1, 6, 257): 3, (14, 6, 257): 3, (15, 6, 257): 2, (16, 6, 257): 2, (21, 6, 288): 2, (22, 6, 288): 1, (22, 6, 257): 1,
                             (1, 1, 1): 1, (3, 6, 128): 1, (3, 6, 129): 2, (3, 6, 256): 2, (43, 6, 129): 1, (300, 1, 288): 1, (128, 1, 200): 2}.items():
        assert R.planned_groups(im, h, t, 256) == want, (im, h, t)
    assert [(c["images"], c["expect_groups"]) for c in R.GROUP_CASES] == [(14, 3), (16, 2), (22, 1)] * 2
    assert all(c["expect_groups"] == R.planned_groups(c["images"], c["heads"], c["tokens"], 256) for c in R.ATTENTION_CASES)
    assert all(c["expect_ft"] == R.planned_ft_per_wg(c["m"], R.FORMS[c["form"]]["n"], R.FORMS[c["form"]]["k"], 256) for c in R.LINEAR_CASES)


def test_weight_cursor_restated_and_its_mutations():
    """The ring of weight fragments (restated from k_tok_gemm): every wave multiplies exactly the sets of its own feature blocks, slab by slab, over
    chunks and walked tiles; waves beyond the layer in a half-full tile read block 0; every load lies inside the packed planes.  The two mutations
    of the cursor that the GPU suite cannot see, and why: `<=` in the stop rule changes only loads that are never consumed (and stays inside the
    planes); an unclamped blk_of changes only what inactive waves load -- beyond the planes, so it is never to be run."""
    for n, k in ((128, 384), (384, 384), (640, 768), (1152, 384), (1280, 384), (1536, 384), (384, 1536), (640, 1536)):
        n_fb, n_ft, ks = n // 32, R.cdiv(n, R.FT), k // 32
        for per in range(1, n_ft + 1):
            for ft0 in range(0, n_ft, per):
                for wave in range(8):
                    ft1 = min(ft0 + per, n_ft)
                    want = [((ft * 8 + wave) if ft * 8 + wave < n_fb else 0, gs) for ft in range(ft0, ft1) for gs in range(ks)]
                    consumed, issued = R.weight_cursor(n, k, ft0, per, wave)
                    assert consumed == want and len(issued) == len(want) + 4 and issued[-4:] == [want[-1]] * 4          # stops on the wave's last set
                    assert all(0 <= b < n_fb and 0 <= g < ks for b, g in issued)
                    c2, i2 = R.weight_cursor(n, k, ft0, per, wave, stop="<=")
                    assert c2 == want and all(0 <= b < n_fb and 0 <= g < ks for b, g in i2)                          # same products, loads in bounds
                    c3, i3 = R.weight_cursor(n, k, ft0, per, wave, clamp=False)
                    active = [(ft * 8 + wave) < n_fb for ft in range(ft0, ft1) for _ in range(ks)]
                    assert [c for c, a in zip(c3, active) if a] == [w for w, a in zip(want, active) if a]                # stored outputs unchanged
    # the half-full last tile of LN + QKV (n = 1152: 36 blocks, tile 4 holds blocks 32 .. 35): waves 4 .. 7 would load blocks 36 .. 39
    _, issued = R.weight_cursor(1152, 384, 4, 1, 5, clamp=False)
    assert max(b for b, _ in issued) == 37 >= 1152 // 32
    _, issued = R.weight_cursor(1152, 384, 3, 2, 5, stop="<=")
    assert issued[-4:] != issued[-5:-4] * 4 and R.weight_cursor(1152, 384, 3, 2, 5)[0] == R.weight_cursor(1152, 384, 3, 2, 5, stop="<=")[0]


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
def test_tables_hold_every_edge():
    assert {c["m"] for c in R.ROW_CASES} == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257}
    assert {(c["m"], c["form"]) for c in R.ROW_CASES} == {(m, f) for m in R.ROW_EDGES for f in ("a", "b", "c", "d", "e768", "e128")}
    assert {(c["form"], c["expect_ft"]) for c in R.WALK_CASES} == {(f, n) for f in ("a", "c", "r1280") for n in (2, 3)}
    assert all(c["m"] % 64 == 1 for c in R.WALK_CASES)
    assert {c["tokens"] for c in R.TOKEN_CASES} == {1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 161, 255, 256, 257, 287, 288}
    assert {(c["tokens"], c["heads"], c["images"], c["mags"]) for c in R.TOKEN_CASES} == {(t, h, i, m) for t in R.TOKEN_EDGES for h in (1, 6) for i in (1, 3)
                                                                                        for m in ((1.0, 1.0, 1.0), (6.0, 3.0, 0.01), (0.05, 0.05, 30.0))}
    assert {(c["tokens"], c["expect_groups"]) for c in R.GROUP_CASES} == {(t, g) for t in (257, 288) for g in (1, 2, 3)}
    assert {c["kind"] for c in R.STRUCTURE_CASES} == {"zero_k", "zero_v", "zero_q_row", "big_key", "big_value"}
    names = [c["name"] for c in R.LINEAR_CASES + R.ATTENTION_CASES]
    seeds = [c["seed"] for c in R.LINEAR_CASES] + [c["seed"] for c in R.ATTENTION_CASES]
    assert len(set(names)) == len(names) and len(set(seeds)) == len(seeds)
    x = R.erf_sweep()
    assert x.shape == (66, 384) and float(x.abs().amax(1).min()) == 40.0 and bool((x * 1024 == (x * 1024).round()).all())
    v = x.flatten()
    assert float(v.min()) == -40.0 and int(((v >= -12) & (v < 12)).sum()) >= 24 * 1024 and len(set(v[(v >= -12) & (v < 12)].tolist())) == 24 * 1024


def torch_fp32_linear(i):
    x = i["x"]
    xh = F.layer_norm(x, (x.shape[1],), i["ln"][0], i["ln"][1], i["ln"][2]) if i["ln"] is not None else x
    v = F.linear(xh, i["w"], i["b"])
    if i["epilogue"] == R.EPI_GELU:
        return F.gelu(v)
    if i["epilogue"] == R.EPI_RESID:
        return i["residual"] + i["gamma"] * v
    return v


@pytest.mark.parametrize("table", ["rows", "walk", "numerics"])
def test_torch_fp32_lies_within_every_linear_bound(table):
    """No case may come with a bound that torch's own fp32 kernels miss (the kernel under test is held to be no worse than an fp32 evaluation),
    with the STARTING constants; every element is compared.  The plain product stays below 2.7e-7 A where nothing but the product is summed."""
    worst = {}
    for case in dict(rows=R.ROW_CASES, walk=R.WALK_CASES, numerics=R.NUMERIC_CASES)[table]:
        i = R.make_linear_inputs(case)
        assert i["x"].shape == (case["m"], R.FORMS[case["form"]]["k"])
        bd = R.linear_bound(i["x"], i["w"], i["b"], i["ln"], i["epilogue"], i["residual"], i["gamma"], **START)
        y = torch_fp32_linear(i)
        assert y.shape == bd.e.shape == bd.ref.shape and bool(torch.isfinite(bd.e).all()) and bool((bd.e > 0).all())
        worst[case["name"]] = R.worst(y, bd)
        if case["form"] in ("p384", "p1536"):
            prod = float(((y.double() - bd.ref).abs() / (bd.terms["product"] / R.LOGIT_ERR + bd.terms["floor"] / 2.7e-7)).max())
            assert prod < 2.7e-7, (case["name"], prod)
    print(f"[vit stage host] torch fp32 / bound, {table}:", {k: (round(r, 3), n) for k, (r, n) in worst.items()})
    assert all(r <= 1.0 for r, _ in worst.values()), {k: v for k, v in worst.items() if v[0] > 1.0}


def test_numeric_cases_are_what_they_claim():
    i = R.make_linear_inputs(next(c for c in R.NUMERIC_CASES if c["name"] == "magnitudes_p384"))
    mx = i["x"].abs().amax(1)
    assert float(mx.min()) < 1e-29 and float(mx.max()) > 1e29
    i = R.make_linear_inputs(next(c for c in R.NUMERIC_CASES if c["name"] == "weight_rows_b"))
    wm = i["w"].abs().amax(1)
    assert float(wm.min()) < 1e-6 and float(wm.max()) > 1e4
    i = R.make_linear_inputs(next(c for c in R.NUMERIC_CASES if c["name"] == "offsets_a"))
    k = R.kappa(i["x"])
    assert float(k.min()) > 250.0                                                                  # offsets 300 x the spread
    i = R.make_linear_inputs(next(c for c in R.NUMERIC_CASES if c["name"] == "special_a"))
    x, w = i["x"], i["w"]
    assert all(bool((x[r] == 0).all()) for r in R.SPECIAL_ROWS["zero"]) and all(float(x[r].var()) == 0.0 and float(x[r].abs().max()) > 0 for r in R.SPECIAL_ROWS["constant"])
    assert all(0 < float(x[r].abs().max()) < 2.0 ** -126 for r in R.SPECIAL_ROWS["subnormal"])
    assert all(bool((w[j] == 0).all()) for j in R.ZERO_W_ROWS)
    ref = R.ref_linear(x, w, i["b"], i["ln"])
    want = F.linear(i["ln"][1].double(), w.double(), i["b"].double())                              # LN(0) = the LayerNorm's bias
    assert torch.allclose(ref[0], want, rtol=1e-12, atol=1e-15) and torch.equal(ref[:, 37], i["b"][37].double().expand(x.shape[0]))
    assert float(R.kappa(x)[5]) == pytest.approx(3.0 / 1e-3, rel=1e-9)                             # a constant row: sigma = sqrt(eps)


@pytest.mark.parametrize("table", ["tokens", "groups", "structure"])
def test_torch_fp32_lies_within_every_attention_bound(table):
    """torch's fp32 CPU attention within every case's bound with the starting c0; in the peaked set it stays below 1.4e-5 s_q."""
    worst, peaked = {}, 0.0
    for case in dict(tokens=R.TOKEN_CASES, groups=R.GROUP_CASES, structure=R.STRUCTURE_CASES)[table]:
        qkv = R.make_attention_inputs(case)
        im, t, h = case["images"], case["tokens"], case["heads"]
        assert qkv.shape == (im * t, 3 * h * 64)
        bd = R.attention_bound(qkv, im, t, h, c0=R.C0_START)
        q, k, v = R._heads(qkv, im, t, h)
        y = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(im * t, h * 64)
        assert y.shape == bd.e.shape and bool(torch.isfinite(bd.e).all())
        worst[case["name"]] = R.worst(y, bd)[0]
        if case["mags"] == R.MAGNITUDES[1] and case["kind"] == "random":
            s = bd.terms["c0"] / R.C0_START
            peaked = max(peaked, float(((y.double() - bd.ref).abs() / s)[s > 0].max()))
            lam = float((bd.terms["logits"] / s)[s > 0].max()) / (2 * R.LOGIT_ERR)
            assert t < 31 or 20.0 < lam < 400.0, (case["name"], lam)                                  # a bound of ~1e-4 s_q: peaked, not slack
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"[vit stage host] torch fp32 attention / bound, {table}: worst {top}; peaked set: {peaked:.3g} s_q")
    assert all(r <= 1.0 for r in worst.values()), {k: v for k, v in worst.items() if v > 1.0}
    assert peaked < 1.4e-5


def test_structure_cases_by_hand():
    case = next(c for c in R.STRUCTURE_CASES if c["name"] == "zero_k_33")
    qkv = R.make_attention_inputs(case)
    ref = R.ref_attention(qkv, 2, 33, 2)
    assert torch.allclose(ref, torch.full_like(ref, 16.0), rtol=1e-14, atol=0)                      # the mean of 0 .. 32
    bd = R.attention_bound(qkv, 2, 33, 2, c0=2e-6)
    assert torch.allclose(bd.e, torch.full_like(bd.e, 2e-6 * 16.0), rtol=1e-12, atol=0)            # Lambda = 0: c0 s_q alone
    case = next(c for c in R.STRUCTURE_CASES if c["name"] == "zero_v_257")
    bd = R.attention_bound(R.make_attention_inputs(case), 2, 257, 2)
    assert bool((bd.ref == 0).all()) and bool((bd.e == 0).all())                                    # exactly 0 is asked
    case = next(c for c in R.STRUCTURE_CASES if c["name"] == "big_key_64")
    qkv = R.make_attention_inputs(case)
    kmax = qkv[:, 128:256].abs().amax(1)
    assert float(kmax[32]) > 1e3 * float(kmax[:32].max())
