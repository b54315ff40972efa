"""The least-squares pose tail on the GPU (ops.solve_pose: k_solve_pose, one 1024-thread workgroup per image) against the fp64 restatement
tests/pose_tail_reference.py, at every k the callers allow and on padded lists.

Cases: pose_tail_reference.cases(k) -- plain, behind, fewdup, heavydup, straddle (once-only origins just below and just above
torch.isin's algorithm switch, the two lists of a pair one origin apart), alphabet (integer coordinates: rays kept through a single
coinciding coordinate), allbehind, parallel, upsing -- 30 lists at each k of 1, 2, 3, 63, 64, 65, 100, 101, 127, 128, 129, 191, 192, 193,
255, 256, each k one launch of 30 images with gt_c2w.  Above 128 valid rays the 64-lane scans run a third and fourth round, the
(ray, quarter) loop of the origin counts wraps the block (kv * 4 > 1024) and the membership test has up to 2304 work items.

Tolerances.  keep / n_kept: exact.  Status: exact wherever the fp64 quantity each decision rests on is clear of its threshold by a
factor of 2 (the two determinants against 1e-7).  w_final and the rotation block: unless a kept ray's fp64 |(c - o).d| < 1e-4; w_final
within 1e-6.  Centre (checked whenever the centre determinant is clear) and the
translation of c2w: |c - c_64|_inf <= CENTRE_C cond(A) max(1, |c_64|_inf) with CENTRE_C = 3.8e-06 = 4 x the CPU oracle's worst value
over the same lists (9.41e-07, measured by tests/test_pose_tail_host.py; the kernel adds in the oracle's order).  Rotation block: 2e-4;
errors: 1e-5 and 1e-3 degrees against oracle.pose_errors on the kernel's own c2w (the tolerances of test_a17_to_a21_solve_pose).  Lists
with a decision inside rounding: 3 of 480 = 0.62 % (asserted <= 1 %), none of them allbehind, parallel or upsing.

Padding: a position is valid when 0 <= idx < R, wherever it sits.  A padded list of 256 (padding at the tail, at the head, interleaved
-- every third position, as far as the padding goes -- mixing -1, other negatives and idx >= R) gives the bits of the call on the
stripped list."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_tail_reference as PT  # noqa: E402

K = PT.MAX_K
PADS = (-1, PT.R, -7, PT.R + 12345, 1 << 40)
ARRANGEMENTS = ("tail", "head", "interleaved")
OUTPUTS = ("c2w", "status", "w_final", "n_kept", "centre", "errors")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    """torch.equal on the bit patterns (a NaN equals the same NaN)."""
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def check_against_reference(tag, out, i, r, gt, oracle):
    """Image i of a solve_pose result (numpy) against the reference r of its list.  -> True when a check was skipped for rounding."""
    centre_ok, status_ok, weights_ok = PT.centre_is_decided(r), PT.status_is_decided(r), PT.weights_are_decided(r)
    wf, st, c2w, ctr = out["w_final"][i], int(out["status"][i]), out["c2w"][i], out["centre"][i]
    assert int(out["n_kept"][i]) == r["n_kept"], tag
    assert (wf[~r["keep"]] == 0).all(), tag
    if centre_ok and weights_ok:
        assert ((wf != 0) == (r["w_final"] != 0)).all(), tag            # kept-but-excluded rays are 0 on both sides; NaN != 0 on both
        assert np.allclose(wf, r["w_final"], rtol=0, atol=1e-6, equal_nan=True), tag
    bound = PT.CENTRE_C * r["cond"] * max(1.0, float(np.abs(r["centre"]).max())) if not r["nan_centre"] else None
    if centre_ok and r["nan_centre"]:
        assert np.isnan(ctr).all(), tag
    elif centre_ok:
        assert np.abs(ctr - r["centre"]).max() <= bound, (tag, np.abs(ctr - r["centre"]).max(), bound)
    if status_ok:
        assert st == r["status"], (tag, st, r["status"])
        if r["nan_pose"]:
            assert np.array_equal(c2w, np.eye(4, dtype=np.float32)), tag
        else:
            assert np.abs(c2w[:3, 3] - r["centre"]).max() <= bound, tag
            if weights_ok:
                assert np.abs(c2w[:3, :3] - r["c2w"][:3, :3]).max() <= 2e-4, tag
    assert np.array_equal(c2w[3], [0, 0, 0, 1]), tag
    if gt is not None:
        te, ae = oracle.pose_errors(gt, c2w)
        assert abs(float(out["errors"][i, 0]) - te) < 1e-5 and abs(float(out["errors"][i, 1]) - ae) < 1e-3, tag
    return not (status_ok and weights_ok)


SKIPPED = {}                  # k -> (lists checked, tags of those with a check skipped for rounding), filled by test_every_kind_at_every_k


@pytest.mark.parametrize("k", PT.KS)
def test_every_kind_at_every_k(ops, oracle, k):
    cs, refs = PT.reference_cases(k)
    ori, dr, idx, val, up, gt = PT.stack(cs)
    out = {n: N(t) for n, t in ops.solve_pose(G(ori), G(dr), G(idx), G(val), G(up), G(gt)).items()}
    assert out["w_final"].shape == (len(cs), k)
    tags = [(c["kind"], k, c["j"], c["note"]) for c in cs]
    skipped = [t for i, (t, c, r) in enumerate(zip(tags, cs, refs)) if check_against_reference(t, out, i, r, c["gt"], oracle)]
    SKIPPED[k] = (len(cs), skipped)


def test_checks_skipped_for_rounding_stay_under_one_percent():
    """Over the launches of test_every_kind_at_every_k that ran before this: the lists with any check skipped, none of them constructed."""
    n, tags = sum(v[0] for v in SKIPPED.values()), [t for v in SKIPPED.values() for t in v[1]]
    print(f"[pose tail] lists with a check skipped for rounding: {len(tags)} of {n}: {tags}")
    assert len(tags) <= PT.SKIP_SHARE * n and not [t for t in tags if t[0] in ("allbehind", "parallel", "upsing")]


# ---- padding ------------------------------------------------------------------------------------------------------------------------------

def arrange(idx, val, how):
    """The valid list (idx, val) padded to K positions.  -> (idx [K], val [K] with NaN at the padding, positions of the valid entries)."""
    n = len(idx)
    if how == "tail":
        pos = np.arange(n)
    elif how == "head":
        pos = np.arange(K - n, K)
    else:
        pad = np.arange(2, K, 3)[: K - n]                                # every third position, as far as the padding goes; the rest at the tail
        pos = np.setdiff1d(np.arange(K), pad)[:n]
    out_i = np.array([PADS[p % len(PADS)] for p in range(K)], np.int64)
    out_v = np.full(K, np.nan, np.float32)
    out_i[pos], out_v[pos] = idx, val
    return out_i, out_v, pos


def padding_bases():
    cs = PT.cases(K)
    return [next(c for c in cs if c["kind"] == kind and c["j"] == j) for kind, j in (("fewdup", 0), ("behind", 1), ("alphabet", 2), ("straddle", 1))]


@pytest.mark.parametrize("how", ARRANGEMENTS)
@pytest.mark.parametrize("n_valid", [0, 1, 37, 64, 65, 129, 200])
def test_padding_at_any_position_is_the_stripped_list(ops, n_valid, how):
    for c in padding_bases()[: 1 if n_valid == 0 else None]:           # no valid entry: every base is the same call
        tag = (c["kind"], n_valid, how)
        ori, dr, up, gt = G(c["ori"]), G(c["dir"]), G(c["up"])[None], G(c["gt"])[None]
        vi, vv = c["idx"][:n_valid], c["val"][:n_valid]
        idx, val, pos = arrange(vi, vv, how)
        got = ops.solve_pose(ori, dr, G(idx)[None], G(val)[None], up, gt)
        if n_valid == 0:
            assert same_bits(got["c2w"][0], torch.eye(4, device="cuda")) and int(got["status"][0]) == 6 and int(got["n_kept"][0]) == 0, tag
            assert same_bits(got["w_final"][0], torch.zeros(K, device="cuda")) and bool(torch.isnan(got["centre"][0]).all()), tag
            continue
        want = ops.solve_pose(ori, dr, G(vi)[None], G(vv)[None], up, gt)
        for name in ("c2w", "status", "n_kept", "centre", "errors"):
            assert same_bits(got[name], want[name]), (tag, name)
        p = torch.from_numpy(pos).cuda()
        assert same_bits(got["w_final"][0][p], want["w_final"][0]), tag
        rest = torch.ones(K, dtype=torch.bool, device="cuda")
        rest[p] = False
        assert same_bits(got["w_final"][0][rest], torch.zeros(K - n_valid, device="cuda")), tag


def test_images_of_different_valid_lengths_in_one_launch(ops):
    c = padding_bases()[0]
    lengths = (0, 1, 2, 63, 64, 65, 255, 256)
    lists = [arrange(c["idx"][:n], c["val"][:n], ARRANGEMENTS[i % 3]) for i, n in enumerate(lengths)]
    ori, dr = G(c["ori"]), G(c["dir"])
    idx, val = G(np.stack([l[0] for l in lists])), G(np.stack([l[1] for l in lists]))
    up = torch.nn.functional.normalize(torch.randn(8, 3, generator=torch.Generator().manual_seed(5)), dim=1).cuda()
    gt = G(c["gt"])[None].expand(8, 4, 4).contiguous()
    got = ops.solve_pose(ori, dr, idx, val, up, gt)
    for i, n in enumerate(lengths):
        assert int(got["n_kept"][i]) == PT.pose_tail(c["ori"], c["dir"], lists[i][0], lists[i][1], N(up[i]))["n_kept"], n
        one = ops.solve_pose(ori, dr, idx[i:i + 1].contiguous(), val[i:i + 1].contiguous(), up[i:i + 1].contiguous(), gt[i:i + 1].contiguous())
        for name in OUTPUTS:
            assert same_bits(got[name][i], one[name][0]), (n, name)


def test_score_topk_of_fewer_rays_than_k_into_solve_pose(ops, oracle):
    """The join the product runs: score_topk on 37 rays with k = 100 answers 37 entries, then (-1, NaN); solve_pose takes that as it comes."""
    c = PT.cases(100)[0]
    ori, dr = c["ori"][:37], c["dir"][:37]
    g = torch.Generator().manual_seed(11)
    key = (torch.randn(37, 384, generator=g) * 0.07).cuda()
    q = (torch.randn(1, 256, 384, generator=g) * 6.0).cuda()
    planes, scale = ops.split_planes_f16(key)
    idx, val, _, _ = ops.score_topk(q, torch.tensor([256], dtype=torch.int32, device="cuda"), None, 100, key_planes=planes, key_scale=scale,
                                    want_scores=False)
    assert sorted(idx[0, :37].tolist()) == list(range(37)) and (idx[0, 37:] == -1).all() and bool(torch.isnan(val[0, 37:]).all())
    out = {n: N(t) for n, t in ops.solve_pose(G(ori), G(dr), idx, val, G(c["up"])[None], G(c["gt"])[None]).items()}
    r = PT.pose_tail(ori, dr, N(idx)[0], N(val)[0], c["up"], c["gt"])
    assert r["n_valid"] == 37 and r["status"] == 0 and not PT.undecided(r)
    check_against_reference("score_topk join", out, 0, r, c["gt"], oracle)
    assert (out["w_final"][0, 37:] == 0).all()


def test_argument_edges_are_answered_without_a_launch(ops):
    """batch = 0 with every pointer NULL: after the range check of k the wrapper returns 0 before it looks at an operand, so only that
    check can answer SIXDGS_E_BADARG here.  It is all that stands between a k = 257 caller and the kernel's 256-entry arrays."""
    L = importlib.import_module("6dgs_amd._lib").load()

    def call(k, batch):
        n = None
        return L.sixdgs_solve_pose(n, n, 10, n, n, k, n, n, batch, n, n, n, n, n, n, n)

    assert call(0, 0) == -1 and call(257, 0) == -1 and call(-1, 0) == -1           # SIXDGS_E_BADARG
    assert call(1, 0) == 0 and call(100, 0) == 0 and call(256, 0) == 0             # no images: nothing to do
    assert call(100, -1) == -1 and call(100, 1) == -1                              # a negative batch; NULL operands
