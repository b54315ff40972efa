"""The batched training window on the GPU: ops.ray_attention_scores (the two-pass scorer forward + sixdgs_score_backward) against fp64,
the window's gradients against the per-image loop, the skip of a non-finite image, the absence of host syncs inside a window, and
train_id_module(batched_window=True) end to end.  Bounds follow test_gpu_training_path.py: the error of the fp32 PyTorch evaluation
against fp64 is the yardstick, and the HIP path may be at most 4 x that plus u sqrt(R), relative to the largest fp64 entry."""
import functools
import importlib
import math
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24
MARGIN = 2.0 ** -20
ZERO_GRADIENT = ("ray_preprocessor.mlp2.2.bias", "attention.k_proj.bias")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module("6dgs_amd.train")


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


# ------------------------------------------------------------------------------------------------------------------------------
# 1. ray_attention_scores against fp64
# ------------------------------------------------------------------------------------------------------------------------------
# (batch, token counts, rays): 17 / 5003 / 28 691 rays, and 300 (no multiple of the 128-ray tile, nor of the forward's 256)
CASES = ((1, (256,), 17), (3, (256, 137, 0), 5003), (3, (1, 256, 137), 28691), (1, (137,), 300),
         (32, (256, 137, 1, 0, 64, 200, 255, 128) * 4, 5003), (32, (256, 137, 1, 0) * 8, 28691))


@pytest.mark.parametrize("b,counts,r", CASES)
@pytest.mark.parametrize("regime", ("flat", "peaked"))
def test_ray_attention_scores_against_fp64(ops, b, counts, r, regime):
    """Forward scores, dq and dk of ops.ray_attention_scores for a random upstream gradient, against PyTorch's softmax + column sum in
    fp64; the fp32 PyTorch evaluation is the yardstick (4 x its error + u sqrt(R), relative to the largest fp64 entry).  Flat: logits
    of spread ~0.05; peaked: queries scaled x45 .. x230 (logit spreads ~2 .. 12 on unit-variance keys), softmax rows dominated by a
    few rays.  q rows at or beyond n_tok hold random values the op must ignore: their dq rows are exactly 0.  Two backward passes
    return the same bits."""
    gen = torch.Generator().manual_seed(1000 * b + r + (7 if regime == "peaked" else 0))
    scale = torch.ones(b, 1, 1) if regime == "flat" else 45 + 185 * torch.rand(b, 1, 1, generator=gen)
    q = (torch.randn(b, 256, 384, generator=gen) * scale * (1.0 if regime == "peaked" else 0.05)).cuda()
    k = (torch.randn(r, 384, generator=gen) / math.sqrt(384) * (1.0 if regime == "peaked" else 19.6)).cuda()
    g = torch.randn(b, r, generator=gen).cuda()
    n_host = list(counts)
    n_tok = torch.tensor(n_host, dtype=torch.int32).cuda()

    def run(dt):
        qq, kk = q.to(dt).requires_grad_(True), k.to(dt).requires_grad_(True)
        s = _scores_ref(qq, n_host, kk)
        dq, dk = torch.autograd.grad((s * g.to(dt)).sum(), (qq, kk), allow_unused=True)
        return s.detach(), dq, dk

    s64, dq64, dk64 = run(torch.float64)
    s32, dq32, dk32 = run(torch.float32)
    qh, kh = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    sh = ops.ray_attention_scores(qh, n_tok, kh)
    dqh, dkh = torch.autograd.grad((sh * g).sum(), (qh, kh), retain_graph=True)
    dqh2, dkh2 = torch.autograd.grad((sh * g).sum(), (qh, kh))
    assert torch.equal(dqh, dqh2) and torch.equal(dkh, dkh2), "two backward passes differ"
    floor = U * math.sqrt(r)
    for name, got, ref, f32 in (("scores", sh, s64, s32), ("dq", dqh, dq64, dq32), ("dk", dkh, dk64, dk32)):
        assert bool(torch.isfinite(got).all()), name
        e_h, e_32 = _rel_max(got, ref), _rel_max(f32, ref)
        assert e_h <= 4 * e_32 + floor, (name, b, r, regime, e_h, e_32)
    for i, n in enumerate(n_host):
        assert not bool(dqh[i, n:].any()), f"dq rows beyond n_tok of image {i} are not 0"
        if n == 0:
            assert not bool(sh[i].any()), f"image {i} with no tokens has nonzero scores"


def test_ray_attention_scores_rejects_bad_operands(ops):
    q = torch.zeros(2, 256, 384, device="cuda")
    k = torch.zeros(10, 384, device="cuda")
    n = torch.tensor([256, 3], dtype=torch.int32, device="cuda")
    for bad in ((q.double(), n, k), (q, n.long(), k), (q[:, :100], n, k), (q, n, k.t().contiguous().t()), (q, n, k[:, :100]), (q.cpu(), n, k)):
        with pytest.raises(RuntimeError):
            ops.ray_attention_scores(*bad)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the window against the per-image loop
# ------------------------------------------------------------------------------------------------------------------------------
def _scorer(pkg):
    syn = importlib.import_module("6dgs_amd.synthetic")
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(0, with_cnn=True).items()}, strict=False)
    return idm.cuda().train()


def _ray_margin(idm64, ori, dr, rgb):
    """test_gpu_training_path._ray_margin: per ray, the smallest |pre-activation| / (|a| |w|^T + |b|) over the ReLU layers of the ray MLP."""
    rp = idm64.ray_preprocessor
    with torch.no_grad():
        ori, dr, rgb = ori.double(), dr.double(), rgb.double()
        x = torch.cat((ori, dr, rgb, idm64._pe(ori, rp.pospe), idm64._pe(dr, rp.viewpe), idm64._pe(rgb, rp.rgbpe)), -1)
        margin = torch.full((x.shape[0],), math.inf, dtype=torch.float64, device=x.device)
        a = x
        for lin in (rp.mlp[0], rp.mlp[2], rp.mlp2[0]):
            if lin is rp.mlp2[0]:
                a = torch.cat((a, x), -1)
            z = torch.nn.functional.linear(a, lin.weight, lin.bias)
            margin = torch.minimum(margin, (z.abs() / (a.abs() @ lin.weight.abs().t() + lin.bias.abs())).min(dim=1).values)
            a = torch.relu(z)
    return margin


class _Window:
    """A pool of 6 training views with pinned image sides (tokens 256 / 137 / 256 / 200 / 1 / 256, fixed feature maps), 32 draws from it,
    and ~3000 rays away from ReLU ties and from every view's camera plane."""

    def __init__(self, pkg):
        syn = importlib.import_module("6dgs_amd.synthetic")
        gen = torch.Generator().manual_seed(11)
        self.counts = (256, 137, 256, 200, 1, 256)
        self.toks = [torch.randn(n, 398, generator=gen).cuda() for n in self.counts]
        self.fmaps = torch.randn(len(self.counts), 384, 16, 16, generator=gen).cuda()
        self.cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(len(self.counts), 23, width=16, height=16)]
        test = importlib.import_module("6dgs_amd.test")
        self.poses = torch.stack([test.gt_pose_and_intrinsics(c, "cuda")[0] for c in self.cams]).cuda()
        self.draw = torch.randint(0, len(self.counts), (32,), generator=gen).tolist()
        idm64 = _scorer(pkg).double()
        rays = syn.make_rays(3600, 4)
        o, d, c = (torch.from_numpy(rays[k]).cuda() for k in ("ori", "dir", "rgb"))
        ok = _ray_margin(idm64, o, d, c) > MARGIN
        for p in self.poses.double():
            ctr, z = p[:3, 3], p[:3, 2]
            ok &= ((o.double() - ctr) * z).sum(-1).abs() / ((o.double() - ctr).abs() @ z.abs()) > MARGIN
        keep = torch.nonzero(ok).flatten()[:3000]
        assert keep.numel() == 3000
        self.rays = (o[keep].contiguous(), d[keep].contiguous(), c[keep].contiguous())
        self.model_up = torch.tensor([0.0, 1.0, 0.0], device="cuda")

    def pin(self, m, dt):
        """Backbone of the per-image forward (by image: the drawn view is found from the image, which carries its pool index)."""
        m.backbone_wrapper.forward = lambda img, mask: (self.toks[int(img[0, 0, 0])].to(dt),
                                                        self.fmaps[int(img[0, 0, 0])].to(dt).permute(1, 2, 0).reshape(-1, 384),
                                                        self.fmaps[int(img[0, 0, 0])].to(dt))
        m.image_tokens = lambda imgs, masks: ([self.toks[int(i[0, 0, 0])].to(dt) for i in imgs],
                                              torch.stack([self.fmaps[int(i[0, 0, 0])] for i in imgs]).to(dt))

    def image(self, v, dt=torch.float32):
        return torch.full((4, 4, 3), float(v), device="cuda", dtype=dt)

    def targets(self, ops):
        return [ops.distance_target(self.rays[0], self.rays[1], self.poses[v], self.counts[v]) for v in range(len(self.counts))]


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _per_image_loop(w, m, dt, targets, skip=()):
    """sum over the draws of (mean((scores - target)^2) + 0.1 camera-up loss) / 32 through IdentificationModule.forward, image by image."""
    m.zero_grad()
    w.pin(m, dt)
    o, d, c = (t.to(dt) for t in w.rays)
    for j, v in enumerate(w.draw):
        if j in skip:
            continue
        s, _, _, up, used = m(w.image(v, dt), None, o, d, c)
        combined = torch.square(s - targets[v].to(dt)[used]).mean() + 0.1 * (-0.5 * torch.cosine_similarity(w.model_up.to(dt), up, dim=-1) + 0.5)
        (combined / 32).backward()
    return _grads(m)


def _window(w, m, train, draws=None):
    m.zero_grad()
    w.pin(m, torch.float32)
    draws = w.draw if draws is None else draws
    loss, logs, finite = train.window_step_loss(m, [w.image(v) for v in draws], [None] * len(draws), w.poses[torch.tensor(draws, device="cuda")],
                                                *w.rays, w.model_up, 32)
    loss.backward()
    return _grads(m), logs, finite


def _check_against(ref, f32, got, what):
    floor = U * math.sqrt(3000)
    assert set(ref) == set(f32) == set(got) and len(ref) == 24, what
    worst = 0.0
    for name in ref:
        scale = float(ref[name.replace(".bias", ".weight")].abs().max()) if name in ZERO_GRADIENT else float(ref[name].abs().max())
        e_h = float((got[name].double() - ref[name]).abs().max()) / scale
        e_32 = float((f32[name].double() - ref[name]).abs().max()) / scale
        assert e_h <= 4 * e_32 + floor, (what, name, e_h, e_32)
        worst = max(worst, e_h / (4 * e_32 + floor))
    return worst


def test_window_equals_the_per_image_loop(pkg, ops, train):
    """One iteration (32 draws from 6 views, 3000 rays, pinned image side): the gradients of all 24 trainable parameters from the window
    (train.window_step_loss: forward_window, ray_attention_scores, one ray-MLP backward) and from the per-image loop on the HIP layers
    (IdentificationModule.forward per draw) each against the per-image loop in fp64 with PyTorch's layers; the fp32 PyTorch per-image loop
    is the yardstick.  Targets: ops.distance_target once per view, the same numbers for every evaluation.  The biases of mlp2.2 and k_proj
    (true gradient 0) are measured against their layer's weight gradient."""
    w = _Window(pkg)
    targets = w.targets(ops)
    m64 = _scorer(pkg).double()
    m64.hip_autograd = False
    ref = _per_image_loop(w, m64, torch.float64, targets)
    m = _scorer(pkg)
    m.hip_autograd = False
    f32 = _per_image_loop(w, m, torch.float32, targets)
    m.hip_autograd = True
    loop = _per_image_loop(w, m, torch.float32, targets)
    win, logs, finite = _window(w, m, train)
    assert bool(finite.all()) and bool(torch.isfinite(logs).all())
    print(f"largest error / bound: per-image HIP loop {_check_against(ref, f32, loop, 'loop'):.2f}, "
          f"window {_check_against(ref, f32, win, 'window'):.2f}")


def test_non_finite_image_is_skipped(pkg, ops, train, monkeypatch):
    """A NaN planted in one target ray of draw 5: that image's combined loss is NaN and it must contribute exactly nothing -- the
    window's gradients equal those of the window without draw 5 (to rounding: the q_proj and camera-up contractions see one image
    fewer) and no gradient holds a NaN."""
    w = _Window(pkg)
    m = _scorer(pkg)
    clean, _, _ = _window(w, m, train, draws=[v for j, v in enumerate(w.draw) if j != 5])
    orig, calls = ops.distance_target, []

    def planted(*a, **k):
        t = orig(*a, **k)
        if len(calls) == 5:
            t[7] = float("nan")
        calls.append(1)
        return t

    monkeypatch.setattr(train.ops, "distance_target", planted)
    got, logs, finite = _window(w, m, train)
    assert finite.tolist() == [j != 5 for j in range(32)]
    assert bool(torch.isfinite(logs).all())
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), name
        scale = float(clean[name.replace(".bias", ".weight")].abs().max()) if name in ZERO_GRADIENT else float(clean[name].abs().max())
        assert float((g - clean[name]).abs().max()) <= 1e-5 * scale, name


def test_window_has_no_host_sync(pkg, ops, train):
    """Forward and backward of one window of 32 RGB images at full size (256 tokens each) under torch.cuda.set_sync_debug_mode("error")."""
    w = _Window(pkg)
    m = _scorer(pkg)
    imgs = [w.image(v) for v in w.draw]
    toks = w.toks[0][None].expand(32, -1, -1).contiguous()          # 256 tokens each
    fmaps = w.fmaps[:1].expand(32, -1, -1, -1).contiguous()
    m.image_tokens = lambda imgs, masks: (toks, fmaps)
    poses = w.poses[torch.zeros(32, dtype=torch.long, device="cuda")]
    loss, _, _ = train.window_step_loss(m, imgs, [None] * 32, poses, *w.rays, w.model_up, 32)      # warm-up (caches, workspaces)
    loss.backward()
    m.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, logs, _ = train.window_step_loss(m, imgs, [None] * 32, poses, *w.rays, w.model_up, 32)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(logs).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. train_id_module(batched_window=True)
# ------------------------------------------------------------------------------------------------------------------------------
def test_train_id_module_batched_window_learns(pkg, tmp_path):
    """The loop of train.py with batched_window=True on a 2 000-Gaussian scene for a few iterations: the weights move, every logged loss
    is finite, and the checkpoint has the keys of the default mode."""
    syn = importlib.import_module("6dgs_amd.synthetic")
    torch.manual_seed(0)
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 3), device="cuda")
    cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(3, 17, width=64, height=64)]
    info = types.SimpleNamespace(train_cameras=cams, test_cameras=cams[:1])
    idm = _scorer(pkg)
    before = {k: v.detach().clone() for k, v in idm.state_dict().items()}
    logged = []
    ckpt = str(tmp_path / "id_module.th")
    pkg.train_id_module(ckpt, "cuda", idm, functools.partial(pkg.generate_all_possible_rays, scene), info, "seq", "cat",
                        n_iterations=4, gradient_accumulation_steps=4, display_every_n_iterations=2, val_every_n_iterations=100,
                        log_fn=lambda tag, v, it: logged.append((tag, v, it)), batched_window=True)
    losses = [v for tag, v, _ in logged if tag == "train/loss"]
    assert len(losses) == 4 and all(np.isfinite(losses)) and all(v > 0 for v in losses)
    after = idm.state_dict()
    for prefix in ("ray_preprocessor.", "attention.", "camera_direction_prediction_network."):
        assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith(prefix)), prefix
    sd = torch.load(ckpt)
    assert set(sd) == {"epoch", "model_state_dict", "optimizer_state_dict", "running_loss"} and sd["epoch"] == 4
    assert set(sd["model_state_dict"]) == set(before)
