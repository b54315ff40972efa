"""The select path's contract (sixdgs_score_select: an exact top-k, or status -1 for the two-pass scorer) at every top-k size it takes, at
small and ragged ray counts, with a workspace too short for the batch, stage by stage, and through IdentificationModule.score_tokens --
against a float64 reference of the operands the kernels actually see.

Reference.  The keys are DECODED from the scaled fp16 planes, k = (h + l) * inv_scale (exact in fp64); q is the fp32 q in fp64;
s[r] = sum_t softmax_r(q_t . k_r / sqrt(384)), on the GPU in fp64, chunked over the rays (logsumexp per token, then the sums).

Bound.  With x = max_t |q_t| * max_r |k_r| / sqrt(384) (a bound on every |logit|, Cauchy-Schwarz) and u = 2^-24, a returned value is
  val = sum_t 2^(L'_t log2e + c_t) / g'_t
(csrc/score.hip: k_sel_rescore), and it differs from s[r] by a relative
  eps_r = (2^-21 + 5u) x          the logit: q's own plane split (<= 2^-22 |q_i| per element) and the dropped l_q l_k term (<= 2^-22
                                  |q_i k_i|) -- the keys' split is gone, they are decoded; fp64 accumulation of the 1152 exact plane
                                  products (< 2^-40 x), its rounding to fp32 (u), the four roundings of the epilogue constant (4u)
        + 128 u ln2               the fma forming the exp2 argument (|argument| <= 128, or e' is 0 / inf)
        + 12 u                    v_exp_f32 (2u), 1 / g' and the product with it (2u), the sum over 256 tokens in the waves (8u)
  + eps_g                         the normaliser g'_t = sum_r e'_t,r of the sweep: each of its terms is within the kernel's own derived
                                  eps = 1.4e-4 x + 1.3e-5 (k_sel_bounds) of the re-score's, which is within eps_r - 10u of the exact
                                  term, and the sum of R positive fp32 terms adds at most D u: a tile's 256 rays in any order (255), the
                                  tiles of one run of the persistent grid (<= R / 2^16 + 1), the 16 lanes x <= 64 runs of the merge (80)
                                  and the += of the sweep (1).
So |val - s[r]| <= beta s[r], beta = 1.01 (eps_r + eps_g) (the 1.01 covers the second-order products).  Two rays whose fp64 scores are
within a factor rho = (1 + beta) / (1 - beta) of each other may come back in either order: that is the margin of every rank check.

Undecidable (status -1 with idx all -1 allowed): a candidate list of ceil8(k) slots (any near-tie within the bound's reach beyond it
refuses), and an image whose candidate count -- the staged sixdgs_select_candidates on the same inputs -- exceeds max_candidates.
Nowhere else."""
import importlib
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 2.0 ** -24
CMAX = 4096


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = importlib.import_module("6dgs_amd.ops")
    o.set_mma_mode(o.MMA_DEFAULT)
    return o


def ceil8(k):
    return (k + 7) // 8 * 8


def beta(x, r):
    eps_r = (2.0 ** -21 + 5 * U) * x + 128 * U * math.log(2.0) + 12 * U
    d = 255 + math.ceil(r / 65536) + 1 + 80 + 1
    eps_g = 1.4e-4 * x + 1.3e-5 + (eps_r - 10 * U) + d * U
    return 1.01 * (eps_r + eps_g)


def decode(planes, scale, r):
    pl = planes.view(torch.float16).view(r, 12, 2, 32).double()
    return (pl[:, :, 0] + pl[:, :, 1]).reshape(r, 384) * scale.double().repeat_interleave(128)[:r, None]


def reference(q, n_tok, keyd, chunk=65536):
    """fp64 scores [R] per image and x per image (see the module docstring)."""
    r = keyd.shape[0]
    kmax = float(keyd.norm(dim=1).max())
    inv = 1.0 / math.sqrt(384.0)
    out = []
    for b, t in enumerate(n_tok):
        if t == 0:
            out.append((torch.zeros(r, dtype=torch.float64, device=keyd.device), 0.0))
            continue
        qb = q[b, :t].double()
        lse = None
        for r0 in range(0, r, chunk):
            m = torch.logsumexp((qb @ keyd[r0:r0 + chunk].T) * inv, dim=1)
            lse = m if lse is None else torch.logaddexp(lse, m)
        s = torch.empty(r, dtype=torch.float64, device=keyd.device)
        for r0 in range(0, r, chunk):
            s[r0:r0 + chunk] = torch.exp((qb @ keyd[r0:r0 + chunk].T) * inv - lse[:, None]).sum(0)
        out.append((s, float(qb.norm(dim=1).max()) * kmax * inv))
    return out


def make_case(ops, r, seed, q_scale, n_tok, sample="default"):
    """make_case of test_gpu_select (keys 0.07 N(0,1), q q_scale N(0,1), zero beyond each image's tokens) with a choice of ray sample:
    'default' (select_sample_indices), 'one' (the middle ray alone) or 'full' (every ray)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    key = torch.randn(r, 384, generator=g) * 0.07
    q = torch.randn(len(n_tok), 256, 384, generator=g) * q_scale
    for b, t in enumerate(n_tok):
        q[b, t:] = 0.0
    key, q = key.cuda(), q.cuda()
    nt = torch.tensor(n_tok, dtype=torch.int32, device="cuda")
    planes, scale = ops.split_planes_f16(key)
    si = {"default": lambda: ops.select_sample_indices(r, "cuda"), "one": lambda: torch.tensor([r // 2], device="cuda"),
          "full": lambda: torch.arange(r, device="cuda")}[sample]()
    assert si.numel() >= 1
    s_planes, s_scale = ops.split_planes_f16(key[si].contiguous())
    c = dict(r=r, q=q, nt=nt, n_tok=list(n_tok), planes=planes, scale=scale, s_planes=s_planes, s_scale=s_scale)
    c["ref"] = reference(q, list(n_tok), decode(planes, scale, r))
    return c


def select(ops, c, k, cmax=CMAX, workspace=None):
    return ops.score_select(c["q"], c["nt"], c["planes"], c["scale"], c["s_planes"], c["s_scale"], k, max_candidates=cmax,
                            workspace=workspace, n_tok_host=c["n_tok"])


def staged_counts(ops, c, k, cmax=CMAX):
    """Candidate counts of the staged path on the same inputs (one chunk): what the resident call's status is made of."""
    ss = ops.SelectStream(c["q"], c["nt"], c["r"], k, cmax, c["n_tok"])
    ss.begin(c["s_planes"], c["s_scale"])
    ss.sweep(c["planes"], c["scale"], 0)
    return ss.candidates()[1].tolist()


def check_image(tag, idx, val, st, s, x, k, may_refuse):
    """The contract for one image -> largest |val - s| / (beta s) (0 for a refusal or an image without tokens)."""
    r = s.shape[0]
    ke = min(r, k)
    idx, val = idx.cpu(), val.cpu().double()
    if st < 0:
        assert may_refuse, f"{tag}: status {st} where the bounds must decide"
        assert st == -1 and bool((idx == -1).all()), f"{tag}: a refusal with a partial answer"
        return 0.0
    assert bool((idx[ke:] == -1).all()) and bool(val[ke:].isnan().all()), f"{tag}: not padded with (-1, NaN) beyond {ke}"
    got = idx[:ke]
    v = val[:ke]
    assert bool((got >= 0).all()) and bool((got < r).all()) and len(set(got.tolist())) == ke, f"{tag}: indices out of range or repeated"
    assert bool((v[:-1] >= v[1:]).all()), f"{tag}: values not non-increasing"
    sc = s.cpu()
    if float(sc.abs().max()) == 0.0:                                   # no tokens: every score is exactly 0, the lowest indices win
        assert torch.equal(got, torch.arange(ke)) and float(v.abs().max()) == 0.0 and st == 0, tag
        return 0.0
    b = beta(x, r)
    rho = (1.0 + b) / (1.0 - b)
    order = torch.argsort(-sc, stable=True)
    ss = sc[order]
    s_k, s_k1 = float(ss[ke - 1]), (float(ss[ke]) if r > ke else 0.0)
    must = order[:ke][ss[:ke] > s_k1 * rho]
    missing = set(must.tolist()) - set(got.tolist())
    assert not missing, f"{tag}: rays of the true top-{ke} not returned: {sorted(missing)[:8]}"
    assert float(sc[got].min()) >= s_k / rho, f"{tag}: a returned ray scores below the {ke}-th by more than the bound"
    err = float(((v - sc[got]).abs() / (b * sc[got])).max())
    assert err <= 1.0, f"{tag}: a value off its fp64 score by {err:.3f} of the bound"
    real = bool((ss[:ke - 1] > rho * ss[1:ke]).all()) and (r == ke or s_k > rho * s_k1)
    if real:
        assert torch.equal(got, order[:ke]), f"{tag}: every gap is real and the order differs"
    return err


def real_gaps(s, x, k):
    r = s.shape[0]
    ke = min(r, k)
    b = beta(x, r)
    rho = (1.0 + b) / (1.0 - b)
    ss = torch.sort(s.cpu(), descending=True).values
    return bool((ss[:ke - 1] > rho * ss[1:ke]).all()) and (r == ke or float(ss[ke - 1]) > rho * float(ss[ke]))


def check_call(ops, c, k, idx, val, status, tag, cmax=CMAX, may_refuse_all=False, two_pass=True):
    """Every image of one call against the reference (and the two-pass scorer on the same planes)."""
    st = status.tolist()
    counts = None
    if not may_refuse_all and min(st) < 0:
        counts = staged_counts(ops, c, k, cmax)
    worst = 0.0
    i2 = v2 = None
    if two_pass:
        i2, v2, _, _ = ops.score_topk(c["q"], c["nt"], None, k, key_planes=c["planes"], key_scale=c["scale"], want_scores=False)
    for b, (s, x) in enumerate(c["ref"]):
        t = f"{tag} image {b} ({c['n_tok'][b]} tokens)"
        may = may_refuse_all or (counts is not None and counts[b] > cmax)
        worst = max(worst, check_image(t, idx[b], val[b], st[b], s, x, k, may))
        if two_pass and st[b] >= 0 and (c["n_tok"][b] == 0 or real_gaps(s, x, k)):
            assert torch.equal(idx[b], i2[b]), f"{t}: the two-pass scorer returns other rays where every gap is real"
            ke = min(c["r"], k)
            if c["n_tok"][b] > 0:
                bnd = 2 * beta(x, c["r"]) * s[idx[b][:ke]].cpu()
                assert bool(((val[b][:ke] - v2[b][:ke]).double().cpu().abs() <= bnd).all()), f"{t}: values differ from the two-pass scorer's"
    return worst, st


# ---- top-k sizes ------------------------------------------------------------------------------------------------------------------------

KS = (1, 2, 7, 99, 100, 101, 256, 1000, 1024)


@pytest.mark.parametrize("q_scale,name", [(0.02, "flat"), (45.0, "peaked")])
def test_select_at_every_topk_size(ops, q_scale, name):
    """k from 1 to 1024 at R = 300 001 (1172 tiles: the tile-maxima threshold for k <= 586, the exact U_(k) above), ragged token counts
    (256, 137, 1, 0, 64), at the default candidate budget and at the smallest legal one, ceil8(k) -- which may refuse, never answer wrongly."""
    c = make_case(ops, 300_001, 7, q_scale, (256, 137, 1, 0, 64))
    worst, answered = 0.0, 0
    for k in KS:
        for cmax in (CMAX, ceil8(k)):
            idx, val, status = select(ops, c, k, cmax)
            assert idx.shape == (5, k) and val.shape == (5, k)
            w, st = check_call(ops, c, k, idx, val, status, f"{name} k={k} cmax={cmax}", cmax, may_refuse_all=cmax != CMAX, two_pass=cmax == CMAX)
            worst = max(worst, w)
            assert st[3] == 0                                  # the image without tokens is always decided
            answered += sum(v >= 0 for v in st)
    print(f"[select contract] k sweep {name}: worst |val - s| = {worst:.3g} of the bound, {answered} image answers")
    assert answered >= 5 * len(KS)


# ---- small and ragged ray counts --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 5, 255, 256, 257, 4096, 4096 + 37, 65_537])
def test_select_at_small_and_ragged_ray_counts(ops, r):
    """R below one 256-ray tile, at a tile edge, one ray past it, and R < k: exactly min(R, k) answers then (-1, NaN), as score_topk.
    Ray samples: select_sample_indices (where it is not empty), a single ray, every ray."""
    samples = (["default"] if r >= ops.SELECT_SAMPLE_STRIDE else []) + ["one", "full"]
    worst = 0.0
    for smp in samples:
        c = make_case(ops, r, 100 + r % 97, 6.0, (256, 37, 0, 1), sample=smp)
        for k in (1, 100, 1024):
            idx, val, status = select(ops, c, k)
            w, st = check_call(ops, c, k, idx, val, status, f"R={r} sample={smp} k={k}")
            worst = max(worst, w)
            if r <= k:
                assert st[:2] == [r, r] and st[2] == 0 and st[3] == r, st       # every ray is a candidate
    print(f"[select contract] R = {r}: worst |val - s| = {worst:.3g} of the bound")


# ---- a workspace too short for the batch ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [101, 1000])
def test_select_in_image_groups_is_the_full_call(ops, k):
    """A workspace of score_select_workspace_bytes(r, g, k, cmax) makes sixdgs_score_select run the batch of 7 in groups of g images
    (then equal groups: 1 x 7, 2 2 2 1 -> 4 x 2, 3 3 1): the same bits as the call with room for all 7."""
    n_tok = (256, 1, 137, 0, 64, 200, 31)
    c = make_case(ops, 200_003, 19, 6.0, n_tok)
    full = select(ops, c, k)
    check_call(ops, c, k, *full, f"7 images k={k}")
    for g in (1, 2, 3):
        ws = torch.empty(ops.score_select_workspace_bytes(c["r"], g, k, CMAX), dtype=torch.uint8, device="cuda")
        assert ws.numel() < ops.score_select_workspace_bytes(c["r"], g + 1, k, CMAX)
        got = select(ops, c, k, workspace=ws)
        for a, b, name in zip(got, full, ("idx", "val", "status")):
            assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), f"groups of {g}, k={k}: {name} differs"


# ---- stage by stage ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 256, 1024])
def test_select_stage_by_stage_is_the_resident_call(ops, k):
    """sixdgs_select_begin / _sweep / _candidates / _rescore over the scene in one chunk: the bits of score_select.  Over three 256-aligned
    chunks (g'_t then sums the chunks' partial sums: a different association, <= 2 D u apart): the same candidate counts, the contract
    against the reference, and where every gap is real the same rays with values within that."""
    c = make_case(ops, 300_001, 23, 6.0, (256, 137, 1))
    idx, val, status = select(ops, c, k)
    check_call(ops, c, k, idx, val, status, f"resident k={k}")
    for chunks in (((0, 300_001),), ((0, 100_096), (100_096, 200_192), (200_192, 300_001))):
        ss = ops.SelectStream(c["q"], c["nt"], c["r"], k, CMAX, c["n_tok"])
        ss.begin(c["s_planes"], c["s_scale"])
        for r0, r1 in chunks:                      # a chunk starts on a 128-ray scale tile: its planes and scales are slices of the scene's
            ss.sweep(c["planes"][r0:r1], c["scale"][r0 // 128:(r1 + 127) // 128], r0)
        cand, count = ss.candidates()
        i2, v2, st2 = ss.rescore(c["planes"], c["scale"], cand, count, compact=False)
        want = [-1 if n > CMAX else n for n in count.tolist()]            # more candidates than the list holds: refused, in both
        assert st2.tolist() == status.tolist() == want, (len(chunks), st2.tolist(), status.tolist(), count.tolist())
        if len(chunks) == 1:
            assert torch.equal(i2, idx)
            assert torch.equal(torch.nan_to_num(v2, nan=-7.0), torch.nan_to_num(val, nan=-7.0))
            continue
        d = 2 * (255 + 2 + 80 + 3) * U
        for b, (s, x) in enumerate(c["ref"]):
            check_image(f"3 chunks k={k} image {b}", i2[b], v2[b], int(st2[b]), s, x, k, int(st2[b]) == -1 and want[b] == -1)
            if int(st2[b]) >= 0 and real_gaps(s, x, k):           # near-ties may swap with the rounding of g'_t; real gaps may not
                assert torch.equal(i2[b], idx[b]), b
                assert bool(((v2[b] - val[b]).abs() <= d * val[b].abs()).all()), b


def test_select_shard_with_fewer_candidates_than_k_pads(ops):
    """allow_fewer (a shard of a ray-sharded scene): (a) a shard of 37 rays at k = 100: its 37 rays in order, then (-1, NaN) -- not a refusal;
    (b) a shard whose threshold comes from a larger scene's U (here: the shard's own 10th largest U stands in for the merged U_(k)) and
    images of 1 and 2 tokens (g_min / g_max ~ 1: the threshold sits just below that U): fewer than k candidates, answered and padded; the
    first 10 are the shard's true top-10."""
    c = make_case(ops, 37, 3, 6.0, (256, 5), sample="full")
    ss = ops.SelectStream(c["q"], c["nt"], 37, 100, CMAX, c["n_tok"])
    ss.begin(c["s_planes"], c["s_scale"])
    ss.sweep(c["planes"], c["scale"], 0)
    cand, count = ss.candidates()
    idx, val, st = ss.rescore(c["planes"], c["scale"], cand, count, compact=False, allow_fewer=True)
    for b, (s, x) in enumerate(c["ref"]):
        assert int(st[b]) == 37
        check_image(f"37-ray shard image {b}", idx[b], val[b], int(st[b]), s, x, 100, False)
    c = make_case(ops, 65_537, 4, 6.0, (1, 2))
    ss = ops.SelectStream(c["q"], c["nt"], c["r"], 100, CMAX, c["n_tok"])
    ss.begin(c["s_planes"], c["s_scale"])
    ss.sweep(c["planes"], c["scale"], 0)
    uk = ss.topk_u(exact=True)[:, 9].contiguous()
    cand, count = ss.candidates(uk=uk)
    idx, val, st = ss.rescore(c["planes"], c["scale"], cand, count, compact=False, allow_fewer=True)
    for b, (s, x) in enumerate(c["ref"]):
        n = int(st[b])
        assert 10 <= n < 100 and n == int(count[b]), (b, n)
        assert bool((idx[b, n:] == -1).all()) and bool(val[b, n:].isnan().all())
        check_image(f"shard top-10 image {b}", idx[b, :10], val[b, :10], n, s, x, 10, False)
        assert bool((val[b, :n - 1] >= val[b, 1:n]).all()) and len(set(idx[b, :n].tolist())) == n


# ---- the module route and the top-k limit -----------------------------------------------------------------------------------------------

@pytest.fixture
def small_scene(syn):
    pkg = importlib.import_module("6dgs_amd")
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(0).items()}, strict=False)
    idm = idm.cuda().eval()
    rays = syn.make_rays(40_000, 5)
    o, d, c = (torch.from_numpy(rays[k]).cuda() for k in ("ori", "dir", "rgb"))
    toks = [torch.from_numpy(syn.make_tokens(t, 70 + i, 40.0)).cuda() for i, t in enumerate((256, 173, 1))]
    return idm, (o, d, c), toks


def test_module_takes_the_select_path_at_every_k(ops, small_scene, monkeypatch):
    """score_tokens(want_scores=False) on a 40 000-ray scene with SELECT_MIN_RAYS lowered: the select path, the fp64 contract, and the
    two-pass path's rays (select disabled) wherever the gaps are real."""
    monkeypatch.setattr(ops, "SELECT_MIN_RAYS", 4096)
    idm, rays, toks = small_scene
    kc = idm._ensure_keys(*rays)
    assert kc["sample"] is not None
    q, n_tok, n_host = idm._tokens_to_q(toks, rays[0].device)
    ref = reference(q, n_host, decode(kc["planes"], kc["scale"], rays[0].shape[0]))
    for k in (1, 256, 1024):
        i_s, v_s, none = idm.score_tokens(toks, *rays, k, want_scores=False)
        assert none is None and idm.last_scoring_path.startswith("select"), idm.last_scoring_path
        st = idm.last_select_candidates
        ops.set_select_enabled(False)
        try:
            i_t, v_t, _ = idm.score_tokens(toks, *rays, k, want_scores=False)
            assert idm.last_scoring_path == "two-pass"
        finally:
            ops.set_select_enabled(True)
        for b, (s, x) in enumerate(ref):
            # a refused image was re-done by the two-pass scorer: its answer then IS the two-pass one
            if st[b] >= 0:
                check_image(f"module k={k} image {b}", i_s[b], v_s[b], st[b], s, x, k, False)
            if st[b] < 0 or real_gaps(s, x, k):
                assert torch.equal(i_s[b], i_t[b]), (k, b)


def test_topk_limit_is_refused_before_any_gpu_work(ops, small_scene, monkeypatch):
    """k outside [1, MAX_TOPK]: ValueError naming the limit on the select path, the two-pass path, the streamed and the ray-sharded scorer;
    the module works afterwards."""
    monkeypatch.setattr(ops, "SELECT_MIN_RAYS", 4096)
    assert ops.MAX_TOPK == 1024
    idm, rays, toks = small_scene
    for k in (2000, 1025, 0):
        for want in (False, True):
            with pytest.raises(ValueError, match="1024"):
                idm.score_tokens(toks, *rays, k, want_scores=want)
        with pytest.raises(ValueError, match="1024"):
            idm.score_tokens_streamed(toks, *rays, k)
        with pytest.raises(ValueError, match="1024"):
            idm.score_tokens_ray_sharded(toks, *rays, 0, rays[0].shape[0], k)
    i_s, _, _ = idm.score_tokens(toks, *rays, 1024, want_scores=False)
    assert idm.last_scoring_path.startswith("select") and i_s.shape == (3, 1024)
    i_t, _, _ = idm.score_tokens(toks, *rays, 1024, want_scores=True)
    assert idm.last_scoring_path == "two-pass" and i_t.shape == (3, 1024)
