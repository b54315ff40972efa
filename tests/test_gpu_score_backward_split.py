"""The scorer backward split over ray groups (sixdgs_score_backward_split through ops.ray_attention_scores(..., ray_groups=G)) against
PyTorch in fp64, for G in {2, 3, 8, auto}; its determinism, its zero rows, its clamping and the bits of G = 1.  The bound is the one of
test_gpu_train_window.test_ray_attention_scores_against_fp64: the error of the fp32 PyTorch evaluation against fp64 is the yardstick,
and the HIP path may be at most 4 x that plus u sqrt(R), relative to the largest fp64 entry."""
import importlib
import math

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24
GROUPS = (2, 3, 8, 0)          # 0 = auto


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


def _rel_max(a, ref):
    return float((a.detach().double() - ref).abs().max() / ref.abs().max())


def _scores_ref(q, n_host, k):
    """sum_t softmax_r(q_t . k_r / sqrt(384)) per image with PyTorch, in the dtype of q / k (images with 0 tokens: zeros)."""
    out = []
    for i, n in enumerate(n_host):
        if n == 0:
            out.append(k.new_zeros(k.shape[0]) + 0 * k.sum())
        else:
            out.append(torch.softmax((q[i, :n] @ k.t()) / math.sqrt(384), dim=-1).sum(0))
    return torch.stack(out)


def _operands(b, r, regime, seed):
    """Flat: logits of spread ~0.05; peaked: queries scaled x45 .. x230 (softmax rows dominated by a few rays).  q rows at or beyond
    n_tok hold random values the op must ignore."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.ones(b, 1, 1) if regime == "flat" else 45 + 185 * torch.rand(b, 1, 1, generator=gen)
    q = (torch.randn(b, 256, 384, generator=gen) * scale * (1.0 if regime == "peaked" else 0.05)).cuda()
    k = (torch.randn(r, 384, generator=gen) / math.sqrt(384) * (1.0 if regime == "peaked" else 19.6)).cuda()
    g = torch.randn(b, r, generator=gen).cuda()
    return q, k, g


def _references(q, k, g, n_host):
    def run(dt):
        qq, kk = q.to(dt).requires_grad_(True), k.to(dt).requires_grad_(True)
        s = _scores_ref(qq, n_host, kk)
        return torch.autograd.grad((s * g.to(dt)).sum(), (qq, kk))

    return run(torch.float64), run(torch.float32)


def _hip_grads(ops, q, n_tok, k, g, groups):
    qh, kh = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    sh = ops.ray_attention_scores(qh, n_tok, kh, ray_groups=groups)
    first = torch.autograd.grad((sh * g).sum(), (qh, kh), retain_graph=True)
    second = torch.autograd.grad((sh * g).sum(), (qh, kh))
    return first, second


# (batch, token counts, rays): 17 / 5003 / 28 691 rays, and 300 (three 128-ray tiles, the last one partial); B = 4 at R = 28 691 is a
# rank's share of a 32-image window at 8 ranks
CASES = ((1, (256,), 17), (3, (256, 137, 0), 5003), (3, (1, 256, 137), 28691), (1, (137,), 300), (4, (256, 137, 256, 1), 28691),
         (32, (256, 137, 1, 0, 64, 200, 255, 128) * 4, 5003), (32, (256, 137, 1, 0) * 8, 28691))


@pytest.mark.parametrize("b,counts,r", CASES)
@pytest.mark.parametrize("regime", ("flat", "peaked"))
def test_split_backward_against_fp64(ops, b, counts, r, regime):
    """dq and dk for every G of GROUPS within 4 x the fp32 PyTorch error + u sqrt(R) of fp64; two backward passes give the same bits; dq
    rows at or beyond n_tok are exactly 0."""
    q, k, g = _operands(b, r, regime, 1000 * b + r + (7 if regime == "peaked" else 0))
    n_host = list(counts)
    n_tok = torch.tensor(n_host, dtype=torch.int32).cuda()
    (dq64, dk64), (dq32, dk32) = _references(q, k, g, n_host)
    floor = U * math.sqrt(r)
    e_q32, e_k32 = _rel_max(dq32, dq64), _rel_max(dk32, dk64)
    worst = 0.0
    for groups in GROUPS:
        (dq, dk), (dq2, dk2) = _hip_grads(ops, q, n_tok, k, g, groups)
        assert torch.equal(dq, dq2) and torch.equal(dk, dk2), f"two backward passes differ at G = {groups}"
        for name, got, ref, e_32 in (("dq", dq, dq64, e_q32), ("dk", dk, dk64, e_k32)):
            assert bool(torch.isfinite(got).all()), (name, groups)
            e_h = _rel_max(got, ref)
            assert e_h <= 4 * e_32 + floor, (name, groups, b, r, regime, e_h, e_32)
            worst = max(worst, e_h / (4 * e_32 + floor))
        for i, n in enumerate(n_host):
            assert not bool(dq[i, n:].any()), f"dq rows beyond n_tok of image {i} are not 0 at G = {groups}"
    print(f"B={b} R={r} {regime}: largest error / bound over G in {GROUPS}: {worst:.2f}")


def test_one_group_is_the_unsplit_backward(ops):
    """ray_groups = 1 through the autograd op, and ops.score_backward with ray_groups=1, give the bits of ops.score_backward without the
    argument; so does any G that clamps to one 128-ray tile (R = 17, G = 8 and auto)."""
    for b, counts, r in ((3, (256, 137, 1), 5003), (2, (256, 0), 17)):
        q, k, g = _operands(b, r, "peaked", 5 + r)
        n_tok = torch.tensor(counts, dtype=torch.int32).cuda()
        _, stats = ops._ray_attention_forward(q, n_tok, k)
        ref = ops.score_backward(q, n_tok, k, stats, g)
        variants = [ops.score_backward(q, n_tok, k, stats, g, ray_groups=1), _hip_grads(ops, q, n_tok, k, g, 1)[0]]
        if r <= 128:
            variants += [ops.score_backward(q, n_tok, k, stats, g, ray_groups=8), ops.score_backward(q, n_tok, k, stats, g, ray_groups=0)]
        for dq, dk in variants:
            assert torch.equal(dq, ref[0]) and torch.equal(dk, ref[1])


def test_groups_clamp_to_the_ray_tiles(ops):
    """R = 300 has three 128-ray tiles: G = 8 runs G = 3 (same bits); G = 2 is another split (other rounding, same bound)."""
    q, k, g = _operands(3, 300, "flat", 77)
    n_tok = torch.tensor([256, 137, 1], dtype=torch.int32).cuda()
    _, stats = ops._ray_attention_forward(q, n_tok, k)
    d3 = ops.score_backward(q, n_tok, k, stats, g, ray_groups=3)
    d8 = ops.score_backward(q, n_tok, k, stats, g, ray_groups=8)
    assert torch.equal(d3[0], d8[0]) and torch.equal(d3[1], d8[1])


def test_negative_groups_are_refused(ops):
    q = torch.zeros(1, 256, 384, device="cuda")
    k = torch.zeros(300, 384, device="cuda")
    n_tok = torch.tensor([256], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.ray_attention_scores(q, n_tok, k, ray_groups=-1)
    with pytest.raises(ValueError):
        ops.score_backward(q, n_tok, k, torch.zeros(1, 256, 2, device="cuda"), torch.zeros(1, 300, device="cuda"), ray_groups=-2)
