"""fp64 references, per-element error bounds, launch-plan restatements and case tables of the ViT stage kernels' edge tests (sixdgs_tok_linear =
k_tok_pack + k_tok_gemm, sixdgs_tok_attention = k_tok_attn; test_gpu_vit_stage_edges.py on the GPU, test_vit_stage_reference_host.py on the CPU).
Plain torch: the same code runs in fp64 on the CPU for the host tests and on the GPU for the GPU tests.  Importing it needs no GPU.

References.  ref_linear: F.layer_norm, F.linear, F.gelu (erf form) and res + gamma * (.), all in double, on the fp32 values as given.
ref_attention: F.scaled_dot_product_attention in double on the permuted views the module uses.

Bounds, per ELEMENT (never relative to the largest output).  u = 2^-23 (one fp32 rounding, relative), LOGIT_ERR = 4e-7 is the figure the suite
already asserts per product of this arithmetic (two scaled fp16 planes, three cross terms, fp32 accumulation: two_pass_reference.LOGIT_ERR).
  linear     v = prologue(x) . w^T + b:      E_v = 4e-7 A + u |v| + floor
               A_ij = sum_k |xh_ik| |w_jk| + |b_j|, xh = x (plain) or LN64(x) (LayerNorm prologue).  K = 1536 has the same form: every
               384-chunk has its own row scale.
               floor_j = 2^-125 (sum_k |w_jk| + 1): the power-of-two row scale is clamped to 2^+-100 (f3_shift), so a row whose largest
               magnitude lies below 2^-113 keeps an absolute grid of 2^-25 2^-100 per element instead of a relative one, and results below
               fp32's normal range may be flushed.  Zero for every row of ordinary size.
  LayerNorm  + c_ln u (1 + kappa_i) sum_k |g_k| |w_jk|,  kappa_i = max_k |x_ik| / sigma_i,  sigma_i = sqrt(var_i + eps): the mean, the
               subtraction, rstd and the scale each round once (c_ln starts at 4); a rounding of the mean or of x - mean is u max|x| in x
               units = u kappa in units of xh / g.  The ill-conditioned rows (offsets 300 x the spread, constant rows) are held by kappa.
  GELU       y = gelu(v):  E = 1.13 E_v + 0.5 |v| E_erf + u |y|   (|gelu'| <= 1.13; the erf enters as 0.5 v (1 + erf))
  residual   y = res + gamma v:  E = |gamma| E_v + u (|res| + |gamma v|)
  attention  per (image, head, query): E_q = (8e-7 Lambda_q + c0) s_q
               Lambda_q = max_key sum_d |q_d| |k_d| / 8: a logit error delta <= 4e-7 Lambda moves every probability by at most e^(+-2 delta)
               (its own logit and the row maximum / sum it is taken against);  s_q = sum_key p_key max_d |v_key,d| in fp64;
               c0 covers the P . V product, exp2 and the final rounding.
The three measured constants (C_LN, E_ERF, C0) are what the GPU tests assert with: 2 x the largest ratio measured on the MI355X against fp64
over the tables, rounded up to one digit, never above the starting values (profiles/vit_stage_edges.md has the ratio of every case).  The host
test holds torch's fp32 CPU evaluation of every case to the same bound with the STARTING constants: a case whose bound were slack enough to
hide a wrong kernel would show there first."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from two_pass_reference import LOGIT_ERR

U = 2.0 ** -23
FLOOR = 2.0 ** -125
GELU_SLOPE = 1.13
C_LN_START, E_ERF_START, C0_START = 4.0, 1.5e-7, 2e-6
# measured on the MI355X (profiles/vit_stage_edges.md): 2 x the largest ratio seen, rounded up to one digit
C_LN, E_ERF, C0 = 0.5, 4.1e-7, 4e-7
CUS = 256                        # compute units of the MI355X: the walk and group tables are built for it and the GPU test asserts the plan
LN_EPS = 1e-6
TT, FT, CK = 64, 256, 384        # token rows / features per workgroup tile, columns per staged chunk
MAX_TOKENS = 288
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2


# ---- references --------------------------------------------------------------------------------------------------------------------------
def _d(t):
    return None if t is None else t.double()


def layer_norm64(x, ln):
    return F.layer_norm(x.double(), (x.shape[1],), ln[0].double(), ln[1].double(), float(ln[2]))


def pre_activation(x, w, b, ln):
    """(xh, v) in fp64: the prologue's rows and the product + bias."""
    xh = layer_norm64(x, ln) if ln is not None else x.double()
    return xh, F.linear(xh, w.double(), _d(b))


def ref_linear(x, w, b=None, ln=None, epilogue=EPI_BIAS, residual=None, gamma=None):
    v = pre_activation(x, w, b, ln)[1]
    if epilogue == EPI_GELU:
        return F.gelu(v)
    if epilogue == EPI_RESID:
        return residual.double() + (gamma.double() * v if gamma is not None else v)
    return v


def _heads(qkv, images, tokens, heads):
    return qkv.view(images, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)          # q, k, v: [images, heads, tokens, 64]


def ref_attention(qkv, images, tokens, heads):
    q, k, v = _heads(qkv.double(), images, tokens, heads)
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(images * tokens, heads * 64)


# ---- the launch plans, restated (pure integer functions) -----------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def planned_ft_per_wg(m, n, k, cus=CUS):
    """tok_ft_per_wg of csrc/vit.hip: feature tiles a workgroup walks.  K beyond one chunk re-stages per chunk: always 1."""
    n_ft = cdiv(n, FT)
    if k != CK:
        return 1
    per = cdiv(cdiv(m, TT) * n_ft, cus)
    return max(1, min(n_ft, per))


def planned_walk(m, n, k, cus=CUS):
    """The feature tiles of each workgroup along y: e.g. [2, 2, 1] for 5 tiles walked in twos."""
    n_ft, per = cdiv(n, FT), planned_ft_per_wg(m, n, k, cus)
    return [min(per, n_ft - f0) for f0 in range(0, n_ft, per)]


def planned_groups(images, heads, tokens, cus=CUS):
    """The loop in sixdgs_tok_attention: groups of 4 query tiles per (image, head); one fewer while the grid exceeds the compute units."""
    groups = cdiv(tokens, 128)
    while groups > 1 and images * heads * groups > cus:
        groups -= 1
    return groups


def smallest_m(n, k, want, cus=CUS):
    """The smallest row count with planned_ft_per_wg == want: one row in its last token tile (m = 64 t + 1)."""
    for t in range(0, 1 << 14):
        if planned_ft_per_wg(TT * t + 1, n, k, cus) == want:
            return TT * t + 1
    raise ValueError((n, k, want, cus))


def weight_cursor(n, k, ft0, ft_per_wg, wave, pfw=4, stop="<", clamp=True):
    """k_tok_gemm's ring of weight fragments for one wave, restated: (consumed, issued) lists of (32-feature block, k-slab) sets -- what the slab
    loop multiplies, in order, and every set the cursor loads (the last `pfw` loads are never consumed).  stop / clamp are the kernel's
    `pf_ft + 1 < ft1` and the `b < n_fb ? b : 0` of blk_of; the other values are the mutations the host test reasons about."""
    n_fb, n_ft, ks = n // 32, cdiv(n, FT), k // 32
    ft1 = min(ft0 + ft_per_wg, n_ft)

    def blk_of(ft):
        b = ft * 8 + wave
        return b if b < n_fb or not clamp else 0

    cur = dict(gs=0, ft=ft0, blk=blk_of(ft0))
    issued = []

    def issue():
        got = (cur["blk"], cur["gs"])
        issued.append(got)
        if cur["gs"] + 1 < ks:
            cur["gs"] += 1
        elif (cur["ft"] + 1 < ft1) if stop == "<" else (cur["ft"] + 1 <= ft1):
            cur["ft"] += 1
            cur["gs"] = 0
            cur["blk"] = blk_of(cur["ft"])
        return got

    ring = [issue() for _ in range(pfw)]
    consumed = []
    for _ft in range(ft0, ft1):
        for _c in range(k // CK):
            for sl in range(CK // 32):
                consumed.append(ring[sl % pfw])
                ring[sl % pfw] = issue()
    return consumed, issued


# ---- the bound's terms -------------------------------------------------------------------------------------------------------------------
def product_term(xh, w, b):
    a = xh.abs() @ w.double().abs().T
    return LOGIT_ERR * (a + b.double().abs() if b is not None else a)


def rounding_term(y):
    return U * y.abs()


def floor_term(w):
    return FLOOR * (w.double().abs().sum(1) + 1.0)


def kappa(x, eps=LN_EPS):
    xd = x.double()
    return xd.abs().amax(1) / torch.sqrt(xd.var(1, unbiased=False) + eps)


def layernorm_term(x, ln, w, c_ln):
    gw = w.double().abs() @ ln[0].double().abs()                                  # [n]: sum_k |g_k| |w_jk|
    return c_ln * U * (1.0 + kappa(x, float(ln[2])))[:, None] * gw[None, :]


def gelu_term(v, e_v, y, e_erf):
    return GELU_SLOPE * e_v + 0.5 * v.abs() * e_erf + U * y.abs()


def residual_term(res, gv):
    return U * (res.double().abs() + gv.abs())


Bound = namedtuple("Bound", "ref e terms v")


def linear_bound(x, w, b=None, ln=None, epilogue=EPI_BIAS, residual=None, gamma=None, c_ln=None, e_erf=None):
    """Bound(ref [m,n], e [m,n], terms {name: [m,n] share of e}, v) in fp64 on the device of x."""
    c_ln = C_LN if c_ln is None else c_ln
    e_erf = E_ERF if e_erf is None else e_erf
    xh, v = pre_activation(x, w, b, ln)
    terms = {"product": product_term(xh, w, b), "rounding_v": rounding_term(v), "floor": floor_term(w)[None, :].expand_as(v)}
    if ln is not None:
        terms["layernorm"] = layernorm_term(x, ln, w, c_ln)
    e_v = sum(terms.values())
    if epilogue == EPI_GELU:
        y = F.gelu(v)
        e = gelu_term(v, e_v, y, e_erf)
        terms = {k: GELU_SLOPE * t for k, t in terms.items()}
        terms.update(erf=0.5 * v.abs() * e_erf, rounding_y=rounding_term(y))
    elif epilogue == EPI_RESID:
        g = gamma.double()[None, :] if gamma is not None else torch.ones_like(v[:1])
        y = residual.double() + g * v
        e = g.abs() * e_v + residual_term(residual, g * v)
        terms = {k: g.abs() * t for k, t in terms.items()}
        terms["residual"] = residual_term(residual, g * v)
    else:
        y, e = v, e_v
    return Bound(y, e, terms, v)      # (terms: the shares of e, for the reports)


def attention_terms(qkv, images, tokens, heads):
    """(Lambda [images, heads, tokens], s [images, heads, tokens]) in fp64."""
    q, k, v = _heads(qkv.double(), images, tokens, heads)
    lam = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) / 8.0
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    s = p @ v.abs().amax(-1, keepdim=True)
    return lam, s[..., 0]


def attention_bound(qkv, images, tokens, heads, c0=None):
    """Bound(ref [m, heads*64], e [m, heads*64] (one value per query and head), terms, None)."""
    c0 = C0 if c0 is None else c0
    lam, s = attention_terms(qkv, images, tokens, heads)
    spread = lambda t: t.permute(0, 2, 1).reshape(images * tokens, heads).repeat_interleave(64, 1)      # noqa: E731
    terms = {"logits": spread(2.0 * LOGIT_ERR * lam * s), "c0": spread(c0 * s)}
    return Bound(ref_attention(qkv, images, tokens, heads), sum(terms.values()), terms, None)


def worst(y, bound):
    """(largest |y - ref| / e, the term that holds the largest share of e there).  Elements with e == 0 must be exact."""
    err = (y.double() - bound.ref).abs()
    ratio = torch.where(bound.e > 0, err / bound.e, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    i = int(ratio.argmax())
    name = max(bound.terms, key=lambda k: float(bound.terms[k].expand_as(ratio).reshape(-1)[i]))
    return float(ratio.reshape(-1)[i]), name


def needed(y, bound, name, unit):
    """What the constant of term `name` would have to be for the bound to hold with the other terms as they are: max (err - others) / unit."""
    err = (y.double() - bound.ref).abs()
    others = bound.e - bound.terms[name]
    r = ((err - others).clamp_min(0.0) / unit)
    return float(r[unit > 0].max()) if bool((unit > 0).any()) else 0.0


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
# The five production stage forms ((e) in its two shapes: 2.5 feature tiles over two chunks, and half a tile).
FORMS = {
    "a": dict(k=384, n=1152, ln=True, epilogue=EPI_BIAS, bias=True, gamma=False),          # LayerNorm + QKV
    "b": dict(k=384, n=384, ln=False, epilogue=EPI_RESID, bias=True, gamma=True),          # proj + LayerScale + residual
    "c": dict(k=384, n=1536, ln=True, epilogue=EPI_GELU, bias=True, gamma=False),          # LayerNorm + FC1 + GELU
    "d": dict(k=1536, n=384, ln=False, epilogue=EPI_RESID, bias=True, gamma=True),         # FC2 + LayerScale + residual
    "e768": dict(k=768, n=640, ln=False, epilogue=EPI_BIAS, bias=True, gamma=False),
    "e128": dict(k=384, n=128, ln=False, epilogue=EPI_BIAS, bias=True, gamma=False),
    "r1280": dict(k=384, n=1280, ln=False, epilogue=EPI_RESID, bias=True, gamma=True),      # five FULL feature tiles, residual epilogue (walk table)
    "p384": dict(k=384, n=384, ln=False, epilogue=EPI_BIAS, bias=False, gamma=False),       # numerics: nothing but the product
    "p1536": dict(k=1536, n=384, ln=False, epilogue=EPI_BIAS, bias=False, gamma=False),
    "g384": dict(k=384, n=384, ln=False, epilogue=EPI_GELU, bias=False, gamma=False),       # the erf sweep (identity weight)
}
PRODUCTION_FORMS = ("a", "b", "c", "d", "e768", "e128")
ROW_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
_FORM_SEED = {f: 500 + i for i, f in enumerate(FORMS)}


def _lcase(name, form, m, seed, rows="normal", expect_ft=1):
    return dict(name=name, form=form, m=m, seed=seed, rows=rows, expect_ft=expect_ft)


ROW_CASES = [_lcase(f"rows_{m}_{f}", f, m, 1000 + 10 * i + j) for i, m in enumerate(ROW_EDGES) for j, f in enumerate(PRODUCTION_FORMS)]
# the walked launches: form (d) (K = 1536) re-stages per chunk and always has ft_per_wg == 1 (planned_ft_per_wg), so it has no walk case
WALK_CASES = [_lcase(f"walk{want}_{f}", f, smallest_m(FORMS[f]["n"], FORMS[f]["k"], want), 2000 + 10 * want + j, expect_ft=want)
              for want in (2, 3) for j, f in enumerate(("a", "c", "r1280"))]
NUMERIC_CASES = [
    _lcase("magnitudes_p384", "p384", 61, 3001, rows="logspace30"),           # row magnitudes 1e-30 .. 1e30, one scale per row
    _lcase("magnitudes_p1536", "p1536", 61, 3002, rows="logspace30"),         # ... and per chunk
    # under LayerNorm the squares of a 1e30 row overflow fp32 in ANY fp32 evaluation (torch's included): the sweep ends at 1e15 there
    _lcase("magnitudes_a", "a", 61, 3003, rows="logspace15"),
    _lcase("weight_rows_b", "b", 70, 3004, rows="normal"),                    # weight rows 1e-6 .. 1e6 (make_params: form seed + "wlog")
    _lcase("offsets_a", "a", 70, 3005, rows="offset300"),                     # offsets 300 x the spread: kappa ~ 300
    _lcase("offsets_c", "c", 70, 3006, rows="offset300"),
    _lcase("special_a", "a", 70, 3007, rows="special"),                       # zero row, constant rows, one subnormal row
    _lcase("special_b", "b", 70, 3008, rows="special"),
    _lcase("special_e128", "e128", 70, 3009, rows="special"),
    _lcase("special_p1536", "p1536", 70, 3010, rows="special"),
]
WLOG_CASES = ("weight_rows_b",)
ZERO_W_ROWS = (0, 37, 383)                                                     # all-zero weight rows of the "special" cases (where n allows)
SPECIAL_ROWS = dict(zero=(0, 33), constant=(5, 64), subnormal=(9,))
LINEAR_CASES = ROW_CASES + WALK_CASES + NUMERIC_CASES

TOKEN_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 161, 255, 256, 257, 287, 288)
MAGNITUDES = ((1.0, 1.0, 1.0), (6.0, 3.0, 0.01), (0.05, 0.05, 30.0))          # (q, k, v): mid, peaked, flat


def _acase(name, images, tokens, heads, mags, seed, kind="random", expect_groups=None):
    return dict(name=name, images=images, tokens=tokens, heads=heads, mags=mags, seed=seed, kind=kind,
                expect_groups=planned_groups(images, heads, tokens) if expect_groups is None else expect_groups)


TOKEN_CASES = [_acase(f"tokens_{t}_h{h}_i{im}_m{mi}", im, t, h, mags, 4000 + 100 * ti + 10 * mi + 2 * (h == 6) + (im == 3))
               for ti, t in enumerate(TOKEN_EDGES) for h in (1, 6) for im in (1, 3) for mi, mags in enumerate(MAGNITUDES)]
# images chosen so that the launcher lowers the groups of 128 queries from 3 to 2 and 1 (a wave then walks two or three query tiles)
GROUP_IMAGES = {3: 14, 2: 16, 1: 22}
GROUP_CASES = [_acase(f"groups{g}_{t}", GROUP_IMAGES[g], t, 6, MAGNITUDES[(g + t) % 3], 7000 + 10 * g + (t == 288), expect_groups=g)
               for t in (257, 288) for g in (3, 2, 1)]
STRUCTURE_TOKENS = (1, 33, 64, 257, 287, 288)
STRUCTURE_CASES = [_acase(f"{kind}_{t}", 2, t, 2, (1.0, 1.0, 1.0), 8000 + 10 * ki + ti, kind=kind)
                   for ki, kind in enumerate(("zero_k", "zero_v", "zero_q_row", "big_key", "big_value")) for ti, t in enumerate(STRUCTURE_TOKENS)]
ATTENTION_CASES = TOKEN_CASES + GROUP_CASES + STRUCTURE_CASES
BIG = 1e4

_params = {}


def make_params(form, wlog=False):
    """The form's constants on the CPU (one set per form, shared by its cases: the GPU test packs each weight once)."""
    key = (form, wlog)
    if key not in _params:
        f = FORMS[form]
        g = torch.Generator(device="cpu").manual_seed(_FORM_SEED[form] + (50 if wlog else 0))
        r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale      # noqa: E731
        if form == "g384":
            w = torch.eye(384)
        else:
            w = r(f["n"], f["k"], scale=0.05)
        if wlog:
            w = w * torch.logspace(-6, 6, f["n"])[torch.randperm(f["n"], generator=g)][:, None]
        p = dict(w=w, b=r(f["n"], scale=0.5) if f["bias"] else None,
                 ln=(r(384) * 0.3 + 1.0, r(384, scale=0.1), LN_EPS) if f["ln"] else None,
                 gamma=r(f["n"], scale=0.5) if f["gamma"] else None)
        _params[key] = p
    return _params[key]


def make_linear_inputs(case):
    """dict(x, w, b, ln, gamma, residual, epilogue) on the CPU from the case's seed.  "special" cases carry their own weight (zero rows)."""
    f = FORMS[case["form"]]
    p = dict(make_params(case["form"], wlog=case["name"] in WLOG_CASES))
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    m, k = case["m"], f["k"]
    x = torch.randn(m, k, generator=g)
    rows = case["rows"]
    if rows == "normal":
        if f["ln"]:      # rows of different spread and offset: per-row statistics
            x = x * torch.exp(torch.randn(m, 1, generator=g)) + torch.randn(m, 1, generator=g) * 2.0
    elif rows == "logspace30":
        x = x * torch.logspace(-30, 30, m)[:, None]
    elif rows == "logspace15":
        x = x * torch.logspace(-30, 15, m)[:, None]
    elif rows == "offset300":
        s = torch.logspace(-2, 2, m)[:, None]
        x = x * s + 300.0 * s * torch.where(torch.arange(m)[:, None] % 2 == 0, 1.0, -1.0)
    elif rows == "special":
        for i in SPECIAL_ROWS["zero"]:
            x[i] = 0.0
        for j, i in enumerate(SPECIAL_ROWS["constant"]):
            x[i] = (3.0, -1e3)[j]
        for i in SPECIAL_ROWS["subnormal"]:
            x[i] = x[i] * 1e-41
        w = p["w"].clone()
        for j in ZERO_W_ROWS:
            if j < f["n"]:
                w[j] = 0.0
        p["w"] = _special_w.setdefault(case["name"], w)
    else:
        raise ValueError(rows)
    res = torch.randn(m, f["n"], generator=g) if f["epilogue"] == EPI_RESID else None
    return dict(x=x, w=p["w"], b=p["b"], ln=p["ln"], gamma=p["gamma"], residual=res, epilogue=f["epilogue"])


_special_w = {}


def erf_sweep():
    """x [66, 384] for form g384 (identity weight, no bias, plain prologue): every multiple of 2^-10 in [-12, 12) and +-40 in every row.  With a
    row maximum of 40 the row scale is 2^8 and every entry has at most 16 significant bits: the two planes hold it exactly, the product with
    the identity is exact, and the kernel's pre-activation IS the entry -- what differs from gelu64 is the epilogue's erf alone."""
    v = (torch.arange(-12 * 1024, 12 * 1024, dtype=torch.float64) / 1024.0).float()
    body = torch.zeros(66 * 382)
    body[: v.numel()] = v
    x = torch.zeros(66, 384)
    x[:, :382] = body.view(66, 382)
    x[:, 382], x[:, 383] = 40.0, -40.0
    return x


def make_attention_inputs(case):
    """qkv [images * tokens, 3 * heads * 64] on the CPU from the case's seed."""
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    im, t, h = case["images"], case["tokens"], case["heads"]
    c = h * 64
    qkv = torch.randn(im * t, 3 * c, generator=g)
    for i, s in enumerate(case["mags"]):
        qkv[:, i * c:(i + 1) * c] *= s
    kind = case["kind"]
    if kind == "zero_k":              # every logit 0: the output is the exact mean of V over `tokens` keys; V[key] = key
        qkv[:, c:2 * c] = 0.0
        qkv[:, 2 * c:] = torch.arange(t, dtype=torch.float32).repeat(im)[:, None]
    elif kind == "zero_v":
        qkv[:, 2 * c:] = 0.0
    elif kind == "zero_q_row":
        qkv[0, :c] = 0.0
        qkv[im * t - 1, :c] = 0.0
    elif kind == "big_key":
        qkv[t // 2, c:2 * c] *= BIG
    elif kind == "big_value":
        qkv[t // 2, 2 * c:] *= BIG
    elif kind != "random":
        raise ValueError(kind)
    return qkv
