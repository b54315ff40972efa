"""The ViT stage kernels (sixdgs_tok_linear = k_tok_pack + k_tok_gemm, sixdgs_tok_attention = k_tok_attn) against fp64 at their row, tile, walk,
token and group edges.  References, per-element bounds, the launch-plan restatements and the case tables: tests/vit_stage_reference.py (its
docstring derives the bounds); test_vit_stage_reference_host.py checks on the CPU that torch's own fp32 evaluation of every case lies within
the same bounds.  Every element of every output is compared; every measured figure is printed as a ratio to its bound before it is asserted.
Beyond the bounds: guard values around strided outputs, bit-for-bit invariances (an output depends on its own row / image / head, the weights
and a fixed order), isolation of NaN / Inf rows, images and heads, the module at 16 images, and the argument errors.  Everything runs inside
this process; the walked launches are reached by the row count, from the device's compute-unit count."""
import importlib
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vit_stage_reference as R    # noqa: E402

SENTINEL = 0x7FC5A5A5              # a NaN's bit pattern: a sentinel taken for data would also show as a non-finite output


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def cus(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


_consts = {}


def on_gpu(i):
    """The case's operands on the GPU; constants (weights above all: the pack cache is keyed on the tensor object) are moved once and kept."""
    out = {}
    for k, v in i.items():
        if k == "ln" and v is not None:
            out[k] = (on_gpu(dict(t=v[0]))["t"], on_gpu(dict(t=v[1]))["t"], v[2])
        elif torch.is_tensor(v) and k in ("w", "b", "gamma", "t"):
            if id(v) not in _consts:
                _consts[id(v)] = (v, v.cuda())
            out[k] = _consts[id(v)][1]
        else:
            out[k] = v.cuda() if torch.is_tensor(v) else v
    return out


def linear(ops, i, x=None, residual=None, out=None):
    y = ops.tok_linear(i["x"] if x is None else x, i["w"], i["b"], ln=i["ln"], epilogue=i["epilogue"], residual=i["residual"] if residual is None else residual,
                       gamma=i["gamma"], out=out)
    torch.cuda.synchronize()
    return y


def bound_of(i, **kw):
    return R.linear_bound(i["x"], i["w"], i["b"], i["ln"], i["epilogue"], i["residual"], i["gamma"], **kw)


def check_linear(ops, case, cus):
    f = R.FORMS[case["form"]]
    assert R.planned_ft_per_wg(case["m"], f["n"], f["k"], cus) == case["expect_ft"], f"{case['name']}: a device of {cus} compute units plans another walk"
    i = on_gpu(R.make_linear_inputs(case))
    y = linear(ops, i)
    bd = bound_of(i)
    ratio, term = R.worst(y, bd)
    extra = ""
    if i["ln"] is not None:
        extra += f", c_ln needed {R.needed(y, bd, 'layernorm', bd.terms['layernorm'] / R.C_LN):.3f}"
    if i["epilogue"] == R.EPI_GELU:
        extra += f", E_erf needed {R.needed(y, bd, 'erf', bd.terms['erf'] / R.E_ERF):.3g}"
    shares = {k: float((((y.double() - bd.ref).abs()) / t.expand_as(bd.e).clamp_min(1e-300)).max()) for k, t in bd.terms.items()}
    print(f"[vit stage edges] linear {case['name']} (m {case['m']}, walk {R.planned_walk(case['m'], f['n'], f['k'], cus)}): err / E {ratio:.4f} (largest term there: "
          f"{term}){extra}; err / each term alone " + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))
    assert y.shape == bd.e.shape and bool(torch.isfinite(y).all()), case["name"]
    assert ratio <= 1.0, f"{case['name']}: an element is {ratio:.3f} x its bound from fp64"
    return i, y, bd


# ---- bounds: the linear tables --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.ROW_EDGES)
def test_linear_rows_against_fp64(ops, cus, m):
    cases = [c for c in R.ROW_CASES if c["m"] == m]
    assert len(cases) == len(R.PRODUCTION_FORMS)
    for case in cases:
        check_linear(ops, case, cus)


@pytest.mark.parametrize("case", R.WALK_CASES, ids=lambda c: c["name"])
def test_linear_walked_tiles_against_fp64(ops, cus, case):
    """ft_per_wg == 2 and 3 (asserted from the device's compute units): the ragged walks 2+2+1 and 3+2 over a half-full last tile (a), the walks
    of LN + FC1 + GELU (c) and of five full tiles under the residual epilogue; the last token tile holds ONE row."""
    i, y, _ = check_linear(ops, case, cus)
    # rows of the walked launch equal the same rows run alone (ft_per_wg == 1), bit for bit: first tile, a ragged middle, the last tiles with the one-row tile
    m, f = case["m"], R.FORMS[case["form"]]
    for i0, r in ((0, 64), (1000, 129), (m - 65, 65), (m - 1, 1)):
        assert R.planned_ft_per_wg(r, f["n"], f["k"], cus) == 1
        alone = linear(ops, i, x=i["x"][i0:i0 + r], residual=None if i["residual"] is None else i["residual"][i0:i0 + r])
        assert torch.equal(alone, y[i0:i0 + r]), f"{case['name']}: rows {i0}:{i0 + r} of the walked launch differ from the same rows alone"


@pytest.mark.parametrize("case", R.NUMERIC_CASES, ids=lambda c: c["name"])
def test_linear_numerics_against_fp64(ops, cus, case):
    i, y, bd = check_linear(ops, case, cus)
    f = R.FORMS[case["form"]]
    if case["rows"] == "special":
        for j in R.ZERO_W_ROWS:      # an all-zero weight row: exactly the bias through the epilogue
            if j < f["n"] and i["epilogue"] == R.EPI_BIAS:
                want = i["b"][j] if i["b"] is not None else torch.zeros((), device="cuda")
                assert bool((y[:, j] == want).all()), f"{case['name']}: output column {j} of an all-zero weight row is not exactly the bias"
        if i["ln"] is None and i["epilogue"] == R.EPI_BIAS:
            want = i["b"] if i["b"] is not None else torch.zeros(f["n"], device="cuda")
            for r in R.SPECIAL_ROWS["zero"]:      # an all-zero row through the plain prologue: exactly the bias
                assert torch.equal(y[r], want), f"{case['name']}: the output of all-zero row {r} is not exactly the bias"
        if i["ln"] is not None:                     # LN(0) = the LayerNorm's bias: the row's output is that of the bias vector
            lnb = i["ln"][1][None, :].repeat(2, 1)
            one = ops.tok_linear(lnb, i["w"], i["b"])
            for r in R.SPECIAL_ROWS["zero"]:
                assert float((y[r] - one[0]).abs().max()) <= float((2 * bd.e[r]).max()), case["name"]


def test_gelu_erf_sweep_against_fp64(ops):
    """The epilogue's erf alone: identity weight, no bias, plain prologue, every multiple of 2^-10 in [-12, 12) and +-40.  The planes hold these
    entries exactly (erf_sweep), so the pre-activation is the entry itself -- checked bit for bit through the bias epilogue first."""
    x = R.erf_sweep().cuda()
    p = on_gpu(R.make_params("g384"))
    assert torch.equal(ops.tok_linear(x, p["w"]), x), "the product with the identity is not exact: the sweep does not isolate the erf"
    y = ops.tok_linear(x, p["w"], epilogue=ops.TOK_EPI_GELU)
    torch.cuda.synchronize()
    v = x.double()
    ref = torch.nn.functional.gelu(v)
    err = (y.double() - ref).abs()
    nz = v != 0
    e_erf = float(((err - R.U * ref.abs()).clamp_min(0.0)[nz] / (0.5 * v.abs()[nz])).max())
    at = float(v[nz][((err - R.U * ref.abs()).clamp_min(0.0)[nz] / (0.5 * v.abs()[nz])).argmax()])
    bd = R.linear_bound(x, p["w"], epilogue=R.EPI_GELU)
    ratio, term = R.worst(y, bd)
    print(f"[vit stage edges] erf sweep: measured erf error {e_erf:.4g} at v = {at:.6g} (the rational form's own 1.5e-7; E_ERF {R.E_ERF:.3g}); err / E {ratio:.4f} ({term}); "
          f"gelu(-40) = {float(y[0, 383])!r}, gelu(40) = {float(y[0, 382])!r}, gelu(0) max |.| = {float(y[~nz].abs().max()) if bool((~nz).any()) else 0.0!r}")
    assert bool(torch.isfinite(y).all())
    assert bool((y[:, 383].abs() <= 1e-30).all()) and bool((y[:, 382] == 40.0).all())              # v = -40: finite, magnitude <= 1e-30, no NaN
    assert bool((y[~nz] == 0).all())
    assert e_erf <= R.E_ERF, f"the erf is off by {e_erf:.4g}, beyond E_ERF = {R.E_ERF:.3g}"
    assert ratio <= 1.0


# ---- bounds: the attention tables -------------------------------------------------------------------------------------------------------------
def check_attention(ops, case, cus):
    im, t, h = case["images"], case["tokens"], case["heads"]
    assert R.planned_groups(im, h, t, cus) == case["expect_groups"], f"{case['name']}: a device of {cus} compute units plans other groups"
    qkv = R.make_attention_inputs(case).cuda()
    y = ops.tok_attention(qkv, im, t, h)
    torch.cuda.synchronize()
    bd = R.attention_bound(qkv, im, t, h)
    ratio, term = R.worst(y, bd)
    unit = bd.terms["c0"] / R.C0
    c0 = R.needed(y, bd, "c0", unit)
    flat = float((((y.double() - bd.ref).abs())[unit > 0] / unit[unit > 0]).max()) if bool((unit > 0).any()) else 0.0
    print(f"[vit stage edges] attention {case['name']} (groups {case['expect_groups']}): err / E {ratio:.4f} ({term}), c0 needed {c0:.3g}, err / s_q {flat:.3g}, "
          f"largest 8e-7 Lambda {float((bd.terms['logits'][unit > 0] / unit[unit > 0]).max()) if bool((unit > 0).any()) else 0.0:.3g}")
    assert y.shape == bd.e.shape and bool(torch.isfinite(y).all()), case["name"]
    assert ratio <= 1.0, f"{case['name']}: an element is {ratio:.3f} x its bound from fp64"
    return qkv, y


@pytest.mark.parametrize("tokens", R.TOKEN_EDGES)
def test_attention_tokens_against_fp64(ops, cus, tokens):
    cases = [c for c in R.TOKEN_CASES if c["tokens"] == tokens]
    assert len(cases) == 12
    for case in cases:
        check_attention(ops, case, cus)


@pytest.mark.parametrize("case", R.GROUP_CASES, ids=lambda c: c["name"])
def test_attention_lowered_groups_against_fp64(ops, cus, case):
    """groups 3, 2 and 1 at 257 and 288 tokens (a wave walks one, two, three query tiles); image i inside the batch equals the single-image call
    (3 groups), bit for bit."""
    qkv, y = check_attention(ops, case, cus)
    t, h = case["tokens"], case["heads"]
    assert R.planned_groups(1, h, t, cus) == 3
    for i in (0, case["images"] // 2, case["images"] - 1):
        one = ops.tok_attention(qkv[i * t:(i + 1) * t], 1, t, h)
        assert torch.equal(one, y[i * t:(i + 1) * t]), f"{case['name']}: image {i} inside the batch differs from the single-image call"


@pytest.mark.parametrize("kind", ["zero_k", "zero_v", "zero_q_row", "big_key", "big_value"])
def test_attention_structure_against_fp64(ops, cus, kind):
    for case in [c for c in R.STRUCTURE_CASES if c["kind"] == kind]:
        qkv, y = check_attention(ops, case, cus)
        if kind == "zero_v":
            assert bool((y == 0).all()), f"{case['name']}: V = 0 must give exactly 0"


# ---- guards -----------------------------------------------------------------------------------------------------------------------------------
def sentinel_buffer(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int32, device="cuda")


def check_sentinels(buf, r0, m, c0, n, tag):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[r0:r0 + m, c0:c0 + n] = False
    assert bool((buf[keep] == SENTINEL).all()), f"{tag}: a guard value around the output was overwritten"
    assert bool(torch.isfinite(buf.view(torch.float32)[r0:r0 + m, c0:c0 + n]).all()), f"{tag}: a non-finite output (a guard or a NaN neighbour taken for data)"


@pytest.mark.parametrize("m", [1, 65, 257])
def test_linear_guards_and_strides(ops, cus, m):
    """out = a view with ldy > n cut from a sentinel buffer with m + 3 rows of slack behind it; the residual a view with ldr > n; x a column slice
    (ldx > k) of a buffer whose other columns and trailing rows are NaN.  Every sentinel intact, every output finite and bit-identical to the
    contiguous call; in place on the residual equals out of place."""
    for case in [c for c in R.ROW_CASES if c["m"] == m]:
        f = R.FORMS[case["form"]]
        i = on_gpu(R.make_linear_inputs(case))
        n, k = f["n"], f["k"]
        want = linear(ops, i)
        xb = torch.full((2 * m + 3, k + 8), math.nan, device="cuda")
        xb[:m, 4:4 + k] = i["x"]
        res = None
        if i["residual"] is not None:
            rb = torch.full((2 * m + 3, n + 12), math.nan, device="cuda")
            rb[:m, 8:8 + n] = i["residual"]
            res = rb[:m, 8:8 + n]
        buf = sentinel_buffer(2 + 2 * m + 3, n + 20)
        view = buf.view(torch.float32)[2:2 + m, 4:4 + n]
        assert view.stride(0) > n and view.data_ptr() % 16 == 0
        got = linear(ops, i, x=xb[:m, 4:4 + k], residual=res, out=view)
        assert got.data_ptr() == view.data_ptr()
        check_sentinels(buf, 2, m, 4, n, case["name"])
        assert torch.equal(view, want), f"{case['name']}: strided input / residual / output differ from the contiguous call"
        if res is not None:
            assert bool(torch.isnan(rb[m:]).all()) and bool(torch.isnan(rb[:, :8]).all()) and torch.equal(res, i["residual"])      # the residual is only read
            inplace = res                           # ... and in place on that view (out is residual) equals out of place
            got = linear(ops, i, x=xb[:m, 4:4 + k], residual=inplace, out=inplace)
            assert torch.equal(inplace, want), f"{case['name']}: in place on the residual differs from out of place"
            assert bool(torch.isnan(rb[m:]).all()) and bool(torch.isnan(rb[:, :8]).all()) and bool(torch.isnan(rb[:, 8 + n:]).all())


@pytest.mark.parametrize("tokens,heads,images", [(1, 6, 3), (33, 1, 3), (129, 6, 2), (257, 6, 3), (288, 2, 3)])
def test_attention_guards_and_strides(ops, tokens, heads, images):
    """qkv a column slice (ldq > 3 c) of a NaN buffer with NaN trailing rows; out a view with ldy > c cut from a sentinel buffer."""
    case = dict(name=f"guards_{tokens}", images=images, tokens=tokens, heads=heads, mags=(1.0, 2.0, 1.0), seed=9000 + tokens, kind="random")
    qkv = R.make_attention_inputs(case).cuda()
    m, c = images * tokens, heads * 64
    want = ops.tok_attention(qkv, images, tokens, heads)
    qb = torch.full((m + tokens + 3, 3 * c + 8), math.nan, device="cuda")
    qb[:m, 4:4 + 3 * c] = qkv
    buf = sentinel_buffer(2 + 2 * m + 3, c + 20)
    view = buf.view(torch.float32)[2:2 + m, 8:8 + c]
    got = ops.tok_attention(qb[:m, 4:4 + 3 * c], images, tokens, heads, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr() and view.stride(0) > c
    check_sentinels(buf, 2, m, 8, c, case["name"])
    assert torch.equal(view, want), f"{case['name']}: strided qkv / output differ from the contiguous call"


# ---- isolation: bad VALUES in one row / image / head, never a fault ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_linear_rows_do_not_mix(ops, cus, bad):
    """A NaN or Inf row of x makes its own output row non-finite and leaves every other row bit-identical -- in every production form, with bad
    rows first in a tile, in the middle and last of all (the row that the tiles' padding repeats), and in a walked launch."""
    cases = [c for c in R.ROW_CASES if c["m"] == 129] + [c for c in R.WALK_CASES if c["name"] in ("walk2_a", "walk2_r1280")]
    for case in cases:
        i = on_gpu(R.make_linear_inputs(case))
        m = case["m"]
        clean = linear(ops, i)
        rows = sorted({0, 37, 64, m - 1})
        x = i["x"].clone()
        x[rows] = bad
        got = linear(ops, i, x=x)
        good = torch.ones(m, dtype=torch.bool, device="cuda")
        good[rows] = False
        assert torch.equal(got[good], clean[good]), f"{case['name']}: a {bad} row of x changed another row's output"
        assert bool((~torch.isfinite(got[~good])).any(1).all()), f"{case['name']}: a {bad} row of x gave a finite output row"


def test_attention_images_and_heads_do_not_mix(ops, cus):
    for images, tokens, heads in ((3, 257, 6), (16, 257, 6), (22, 288, 6), (3, 33, 2)):
        case = dict(name="isolation", images=images, tokens=tokens, heads=heads, mags=(1.0, 1.0, 1.0), seed=9500 + images, kind="random")
        qkv = R.make_attention_inputs(case).cuda()
        c = heads * 64
        clean = ops.tok_attention(qkv, images, tokens, heads)
        bad_image = images // 2
        q2 = qkv.clone()
        q2[bad_image * tokens:(bad_image + 1) * tokens] = math.nan
        got = ops.tok_attention(q2, images, tokens, heads)
        keep = torch.ones(images * tokens, dtype=torch.bool, device="cuda")
        keep[bad_image * tokens:(bad_image + 1) * tokens] = False
        assert torch.equal(got[keep], clean[keep]), f"{images} x {tokens}: a NaN image changed another image"
        assert bool(torch.isnan(got[~keep]).all())
        bad_head = heads - 1
        for part in range(3):      # NaN in q, then k, then v of one head
            q3 = qkv.clone()
            q3[:, part * c + bad_head * 64: part * c + (bad_head + 1) * 64] = math.nan
            got = ops.tok_attention(q3, images, tokens, heads)
            cols = torch.ones(c, dtype=torch.bool, device="cuda")
            cols[bad_head * 64:(bad_head + 1) * 64] = False
            assert torch.equal(got[:, cols], clean[:, cols]), f"{images} x {tokens}: NaN in part {part} of head {bad_head} changed another head"
            assert bool(torch.isnan(got[:, ~cols]).all())
    torch.cuda.synchronize()


# ---- the module at 16 images: all five stages on their walked forms -----------------------------------------------------------------------------
def test_fused_vit_blocks_at_16_images_equal_the_unfused_module(cus, monkeypatch):
    bb = importlib.import_module("6dgs_amd.backbone")
    m = 16 * 257
    assert all(m >= v for v in bb.FUSED_MIN_ROWS.values())                                           # every stage is the library's at this size
    assert R.planned_ft_per_wg(m, 1152, 384, cus) == 2 and R.planned_ft_per_wg(m, 1536, 384, cus) == 2 and R.planned_groups(16, 6, 257, cus) == 2
    torch.manual_seed(3)
    vit = bb.ViTS14().eval()
    with torch.no_grad():
        for blk in vit.blocks:
            blk.ls1.gamma.copy_(torch.rand(384) * 0.5 + 0.1)
            blk.ls2.gamma.copy_(torch.rand(384) * 0.5 + 0.1)
            blk.norm1.weight.copy_(torch.rand(384) + 0.5)
            blk.norm1.bias.copy_(torch.randn(384) * 0.1)
            blk.norm2.weight.copy_(torch.rand(384) + 0.5)
            blk.norm2.bias.copy_(torch.randn(384) * 0.1)
        x = torch.randn(16, 3, 224, 224).cuda()
        vg = vit.to("cuda")
        monkeypatch.setenv("SIXDGS_VIT_FUSED", "1")
        fused = vg.forward_features(x)["x_norm_patchtokens"]
        monkeypatch.setenv("SIXDGS_VIT_FUSED", "0")
        plain = vg.forward_features(x)["x_norm_patchtokens"]
        monkeypatch.delenv("SIXDGS_VIT_FUSED")
    scale = float(plain.abs().max())
    d = float((fused - plain).abs().max()) / scale
    print(f"[vit stage edges] module at 16 images: fused vs unfused {d:.3g} of the largest token")
    assert fused.shape == (16, 256, 384) and d < 1e-5


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    with pytest.raises(RuntimeError):
        ops.tok_attention(z(289, 192), 1, 289, 1)                                           # one more token than a wave holds logits for: unsupported
    ops.tok_attention(z(288, 192), 1, 288, 1)
    with pytest.raises(RuntimeError):
        ops.tok_attention(z(40, 194)[:, :192], 1, 40, 1)                                    # ldq % 4 != 0
    with pytest.raises(RuntimeError):
        ops.tok_attention(z(40, 192), 1, 40, 1, out=z(41, 60).as_strided((40, 64), (60, 1)))   # ldy < heads * 64
    w = torch.randn(128, 384, device="cuda")
    with pytest.raises(RuntimeError):
        ops.tok_linear(z(10, 384), w, out=z(11, 124).as_strided((10, 128), (124, 1)))        # ldy < n
    with pytest.raises(RuntimeError):
        ops.tok_linear(z(10, 384), w, epilogue=ops.TOK_EPI_RESID, residual=z(11, 124).as_strided((10, 128), (124, 1)))      # ldr < n
    with pytest.raises(RuntimeError):
        ops.tok_linear(z(10, 384), w, out=z(10, 130)[:, :128])                               # ldy % 4 != 0
    torch.cuda.synchronize()
