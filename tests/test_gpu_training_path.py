"""The training path's HIP kernels against float64 references: HipLinear (6dgs_amd/autograd.py) forward and backward, the ray MLP and
q/k projections as training composes them, one full training step, and sixdgs_distance_target (the loss targets).  Every reference is
evaluated in float64 -- by PyTorch on the GPU (its kernels are the yardstick here, not ours) or by numpy -- and nothing outside the
repository is read."""
import importlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24                 # unit roundoff of fp32
TOL_K = 2.0 ** -15             # element-wise bound of a contraction of length <= 512 (derivation: test_hip_linear_against_fp64)
MARGIN = 2.0 ** -20            # pre-activations closer to 0 than this (relative to their absolute product) are ReLU ties


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def hip(pkg):
    return importlib.import_module("6dgs_amd.autograd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def tol_m(m: int) -> float:
    """Element-wise bound of a contraction over the M rows (dW on the kernel: M padded to 16, 12 accumulator updates per 32-row slab;
    db: PyTorch's column sum, a shallower reduction)."""
    mp = m + (-m) % 16
    return max(TOL_K, (12 * -(-mp // 32) + 8) * U)


def check_elementwise(got, ref, scale, tol, what):
    """max |got - ref| / scale <= tol element by element; where the scale is 0 the exact value is 0 and `got` must be exactly 0."""
    assert got is not None and tuple(got.shape) == tuple(ref.shape), what
    d = (got.detach().double() - ref).abs()
    zero = scale == 0
    assert not bool((d[zero] != 0).any()), f"{what}: nonzero where the exact value is 0"
    nz = ~zero
    e = float((d[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0
    assert e <= tol, f"{what}: {e:.3e} > {tol:.3e}"
    return e


# ------------------------------------------------------------------------------------------------------------------------------
# 1. HipLinear against fp64 autograd
# ------------------------------------------------------------------------------------------------------------------------------
MS = (0, 1, 15, 16, 17, 129, 5003, 28691)
# (K, N): the scorer's layers (ray MLP 141->512, 512->512, W3 on h, mlp2.2 512->384, k_proj 384->384, q_proj 398->384), an N that is
# not a multiple of 128 (on both dx branches) and a K that is a multiple of 128 but not of 512
SHAPES = ((141, 512), (512, 512), (512, 384), (384, 384), (398, 384), (141, 37), (256, 37))
# (relu, bias, x requires grad, upstream gradient): every relu x bias x dx combination once; each upstream form twice
COMBOS = ((True, True, True, "dense"), (True, False, False, "dense"), (True, True, False, "strided"), (True, False, True, "transposed"),
          (False, True, True, "stride0"), (False, False, False, "transposed"), (False, True, False, "dense"), (False, False, True, "strided"))


def _layer_data(m, k, n, seed):
    """x [M,K], w [N,K], b [N] on the GPU, with exact zeros placed so that some pre-activations are exactly 0: every 7th row of x
    (from row 3), every 5th bias entry (from 1) and the whole weight row + bias of column N // 2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    b = 0.5 * torch.randn(n, generator=g)
    x[3::7] = 0
    b[1::5] = 0
    w[n // 2] = 0
    b[n // 2] = 0
    return x.cuda(), w.cuda(), b.cuda(), torch.randn(m, n, generator=g).cuda()


def _upstream(kind, y, g):
    """Scalar loss of y whose gradient is g (masked to the columns used) reaching HipLinear.backward contiguous, transposed,
    from a strided view, or as a stride-0 expansion (y.sum())."""
    if kind == "dense":
        return (y * g).sum()
    if kind == "transposed":
        return (y.t() * g.t().contiguous()).sum()                # dy arrives as the transpose of a contiguous [N,M]
    if kind == "strided":
        return (y[:, ::2] * g[:, ::2]).sum()
    return y.sum()


def _run_case(hip, m, k, n, relu, bias, xg, kind, seed):
    x, w, b, g = _layer_data(m, k, n, seed)
    x64, w64, b64 = x.double(), w.double(), b.double()
    z64 = torch.nn.functional.linear(x64, w64, b64 if bias else None)
    sy = x64.abs() @ w64.abs().t() + (b64.abs() if bias else 0)
    if relu:                       # ReLU ties (|z| within the forward bound of 0, but not exactly 0) get no upstream gradient
        g = torch.where((z64 != 0) & (z64.abs() <= TOL_K * sy), torch.zeros_like(g), g)
    # ---- fp64 reference
    xr, wr = x64.clone().requires_grad_(xg), w64.clone().requires_grad_(True)
    br = b64.clone().requires_grad_(True) if bias else None
    zr = torch.nn.functional.linear(xr, wr, br)
    zr.retain_grad()
    yr = torch.relu(zr) if relu else zr
    _upstream(kind, yr, g.double()).backward()
    dz = zr.grad                                                  # the masked upstream gradient dL/dz
    # ---- HIP
    xh, wh = x.clone().requires_grad_(xg), w.clone().requires_grad_(True)
    bh = b.clone().requires_grad_(True) if bias else None
    yh = hip.linear(xh, wh, bh, relu=relu)
    loss = _upstream(kind, yh, g)
    inputs = [t for t in (xh, wh, bh) if t is not None and t.requires_grad]
    grads = torch.autograd.grad(loss, inputs, retain_graph=True)
    again = torch.autograd.grad(loss, inputs)
    assert all(torch.equal(p, q) for p, q in zip(grads, again)), "two backward passes differ"
    got = dict(zip([id(t) for t in inputs], grads))
    tag = (m, k, n, relu, bias, xg, kind)
    yref = torch.relu(z64) if relu else z64
    err = {"y": check_elementwise(yh, yref, sy, TOL_K, ("y",) + tag)}
    err["dW"] = check_elementwise(got[id(wh)], wr.grad, dz.abs().t() @ x64.abs(), tol_m(m), ("dW",) + tag)
    if bias:
        err["db"] = check_elementwise(got[id(bh)], br.grad, dz.abs().sum(0), tol_m(m), ("db",) + tag)
    if xg:
        err["dx"] = check_elementwise(got[id(xh)], xr.grad, dz.abs() @ w64.abs(), TOL_K, ("dx",) + tag)
    return err


@pytest.mark.parametrize("k,n", SHAPES)
def test_hip_linear_against_fp64(hip, k, n):
    """autograd.linear (HipLinear: forward, dx, dW, db) against F.linear (+ ReLU) with fp64 autograd, at M in {0, 1, 15, 16, 17, 129,
    5003, 28 691} (no padding / padding of the dW contraction, the smoke-size ray count), with and without ReLU and bias, with and without
    dx (K = 141 -> 144 and 398 -> 400 reach the PyTorch branch, 256 / 384 / 512 the kernel), with exact-zero pre-activations, and with the
    upstream gradient contiguous, transposed, from a strided view and stride-0; two backward passes must agree bit for bit.

    Bound, element by element, on the error divided by the matching absolute product: |x| |w|^T + |b| for y, |dz| |w| for dx, |dz|^T |x|
    for dW and the column sums of |dz| for db, where dz is the fp64 gradient at the pre-activation.  Derivation: the kernel splits
    each fp32 operand into three bf16 planes (8 + 8 + 8 significant bits) and drops the three smallest of the nine plane products, <= 3u
    of each |a b| (u = 2^-24); the bf16 products are exact in fp32, and every v_mfma_f32_32x32x16_bf16 is at worst a 4-level pairwise
    tree plus one rounding of the accumulator, each bounded by u times the absolute product P -- 12 MFMAs per 32-wide slab.  Hence
    |err| <= (12 ceil(L/32) + 8) u P for a contraction of length L (bias add included).  For L <= 512 that is <= 200 u; PyTorch's fp32
    matmul (dx when K % 128 != 0) is bounded by the recursive-summation L u <= 512 u: both lie under the fixed 2^-15 = 512 u.  The
    dW contraction runs over the M rows: max(2^-15, (12 ceil(M'/32) + 8) u) with M' = M padded to 16, and the same bound for db.
    Where the absolute product is 0 the value must be exactly 0: that is where the ReLU masks an exactly-zero pre-activation (PyTorch
    gives 0 gradient there).  Upstream entries at ReLU ties (0 < |z| <= 2^-15 |x| |w|^T) are zeroed, since fp32 may round them either
    side of 0.  A single-precision loss in dx (bf16 operands: ~2^-9 of |a b| per product) exceeds the bound by an order of magnitude."""
    worst = {}
    for i, m in enumerate(MS):
        for j, (relu, bias, xg, kind) in enumerate(COMBOS):
            if kind == "stride0" and relu:
                continue
            for key, e in _run_case(hip, m, k, n, relu, bias, xg, kind, 1000 * k + 10 * i + j).items():
                worst[key] = max(worst.get(key, 0.0), e)
    print(f"K={k} N={n} worst normalised errors", {key: f"{e:.2e}" for key, e in worst.items()})


def test_hip_linear_w3_column_split_against_fp64(hip):
    """ray_mlp's W3: z = h W3[:, :512]^T + b + x W3[:, 512:]^T as two HipLinear calls whose weight gradients meet in one [512, 653]
    parameter, against fp64 F.linear on cat([h, x]), at M in {1, 17, 5003, 28 691}, with dh (K = 512: the kernel) and dx (K = 141 -> 144:
    the PyTorch branch) both requested.  Bounds as test_hip_linear_against_fp64: the forward is the sum of two contractions of 512 and
    144 plus one add, (200 + 68 + 1) u < 2^-15, element-wise on |[h, x]| |W3|^T + |b|; dW3 per column block tol_m(M)."""
    for m in (1, 17, 5003, 28691):
        gen = torch.Generator().manual_seed(77 + m)
        h = torch.relu(torch.randn(m, 512, generator=gen)).cuda()
        x = torch.randn(m, 141, generator=gen).cuda()
        w3 = (torch.randn(512, 653, generator=gen) / math.sqrt(653)).cuda()
        b3 = (0.5 * torch.randn(512, generator=gen)).cuda()
        g = torch.randn(m, 512, generator=gen).cuda()
        hh, xh, wh, bh = (t.clone().requires_grad_(True) for t in (h, x, w3, b3))
        z = hip.linear(hh, wh[:, :512], bh) + hip.linear(xh, wh[:, 512:], None)
        (z * g).sum().backward()
        h64, x64, w64, b64 = (t.double().requires_grad_(True) for t in (h, x, w3, b3))
        a64 = torch.cat((h64, x64), -1)
        z64 = torch.nn.functional.linear(a64, w64, b64)
        (z64 * g.double()).sum().backward()
        a_abs, w_abs, g_abs = a64.detach().abs(), w64.detach().abs(), g.double().abs()
        check_elementwise(z, z64.detach(), a_abs @ w_abs.t() + b64.detach().abs(), TOL_K, ("z", m))
        sw = g_abs.t() @ a_abs
        check_elementwise(wh.grad[:, :512], w64.grad[:, :512], sw[:, :512], tol_m(m), ("dW3[:, :512]", m))
        check_elementwise(wh.grad[:, 512:], w64.grad[:, 512:], sw[:, 512:], tol_m(m), ("dW3[:, 512:]", m))
        check_elementwise(bh.grad, b64.grad, g_abs.sum(0), tol_m(m), ("db3", m))
        check_elementwise(hh.grad, h64.grad, g_abs @ w_abs[:, :512], TOL_K, ("dh", m))
        check_elementwise(xh.grad, x64.grad, g_abs @ w_abs[:, 512:], TOL_K, ("dx", m))


@pytest.mark.parametrize("k,n", ((141, 512), (512, 37)))
def test_hip_linear_needs_input_grad_subsets(hip, k, n):
    """Every non-empty subset of {x, w, b} requiring grad (M = 17, ReLU): exactly the requested gradients come back, each within the
    bounds of test_hip_linear_against_fp64, and an M = 0 batch gives zero gradients of the right shapes (its dW has no rows to
    contract, which the kernel would reject as a contraction of length 0)."""
    for m in (17, 0):
        x, w, b, g = _layer_data(m, k, n, 5 + m)
        x64, w64, b64 = x.double(), w.double(), b.double()
        z64 = torch.nn.functional.linear(x64, w64, b64)
        g = torch.where((z64 != 0) & (z64.abs() <= TOL_K * (x64.abs() @ w64.abs().t() + b64.abs())), torch.zeros_like(g), g)
        dz = g.double() * (z64 > 0)
        ref = {"x": dz @ w64, "w": dz.t() @ x64, "b": dz.sum(0)}
        scale = {"x": dz.abs() @ w64.abs(), "w": dz.abs().t() @ x64.abs(), "b": dz.abs().sum(0)}
        tol = {"x": TOL_K, "w": tol_m(m), "b": tol_m(m)}
        for mask in range(1, 8):
            want = {"x": bool(mask & 1), "w": bool(mask & 2), "b": bool(mask & 4)}
            t = {"x": x.clone().requires_grad_(want["x"]), "w": w.clone().requires_grad_(want["w"]), "b": b.clone().requires_grad_(want["b"])}
            (hip.linear(t["x"], t["w"], t["b"], relu=True) * g).sum().backward()
            for name in "xwb":
                if want[name]:
                    check_elementwise(t[name].grad, ref[name], scale[name], tol[name], (name, m, mask))
                else:
                    assert t[name].grad is None, (name, m, mask)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the ray MLP and the q/k projections as training composes them
# ------------------------------------------------------------------------------------------------------------------------------
def _scorer(pkg, syn_seed=0, with_cnn=False):
    syn = importlib.import_module("6dgs_amd.synthetic")
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(syn_seed, with_cnn=with_cnn).items()}, strict=False)
    return idm.cuda().train()


def _ray_margin(idm64, ori, dr, rgb):
    """Per ray, the smallest |pre-activation| / (|a| |w|^T + |b|) over the three ReLU layers of the ray MLP, in fp64.  A ray whose
    margin is within rounding of 0 can take the other side of a ReLU in fp32 than in fp64 -- a jump in the gradient that no
    rounding bound describes -- so the tests below leave such rays out."""
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
            s = a.abs() @ lin.weight.abs().t() + lin.bias.abs()
            margin = torch.minimum(margin, (z.abs() / s).min(dim=1).values)
            a = torch.relu(z)
    return margin


def _rel_max(a, ref):
    return float((a.detach().double() - ref).abs().max() / ref.abs().max())


def test_ray_mlp_and_projections_against_fp64(pkg, hip):
    """IdentificationModule.ray_features_autograd with hip_autograd=True (autograd.ray_mlp: four HipLinear calls, W3 split in two),
    then k_proj on the features and q_proj on 137 tokens (K = 398 -> 400) through HipLinear, as IdentificationModule.forward composes
    them; against the same parameters evaluated by PyTorch in fp64, at R in {17, 5003, 28 691}: features, keys, queries and all 12
    parameter gradients (mlp2.0's weight per column block: the block fed by h and the block fed by the encoding).

    Bound: the fp32 PyTorch evaluation of the same module (hip_autograd=False) measures how far fp32 lands from fp64 on this data;
    the HIP path may be at most 4 x that (the kernel rounds its accumulator 12 times per 32-long slab where an fp32 MFMA GEMM rounds 8:
    sqrt(12/8) on a random walk, with room for the operand split), plus a floor of u max(16, sqrt(R)) of the largest entry: the
    random-walk size of an fp32 sum of R terms, for the weight gradients whose contraction runs over the rays.  Errors are taken
    relative to the tensor's largest fp64 entry.  Rays at a ReLU tie (_ray_margin <= 2^-20) are left out of the set."""
    syn = importlib.import_module("6dgs_amd.synthetic")
    idm, idm64 = _scorer(pkg), _scorer(pkg).double()
    idm64.hip_autograd = False
    tok = torch.from_numpy(syn.make_tokens(137, 4, 1.0)).cuda()
    for r in (17, 5003, 28691):
        rays = syn.make_rays(r + r // 10 + 16, 7)
        o, d, c = (torch.from_numpy(rays[k]).cuda() for k in ("ori", "dir", "rgb"))
        keep = torch.nonzero(_ray_margin(idm64, o, d, c) > MARGIN).flatten()[:r]
        assert keep.numel() == r
        o, d, c = o[keep], d[keep], c[keep]
        gen = torch.Generator().manual_seed(r)
        pf, pk, pq = (torch.randn(*s, generator=gen).cuda() for s in ((r, 384), (r, 384), (137, 384)))

        def run(m, use_hip):
            m.zero_grad()
            m.hip_autograd = use_hip
            cast = (lambda t: t.double()) if m is idm64 else (lambda t: t)
            feat = m.ray_features_autograd(cast(o), cast(d), cast(c))
            att = m.attention
            if use_hip:
                k = hip.linear(feat, att.k_proj.weight, att.k_proj.bias)
                q = hip.linear(tok, att.q_proj.weight, att.q_proj.bias)
            else:
                k, q = att.k_proj(feat), att.q_proj(cast(tok))
            ((feat * cast(pf)).sum() + (k * cast(pk)).sum() + (q * cast(pq)).sum()).backward()
            out = {"feat": feat.detach(), "k": k.detach(), "q": q.detach()}
            for name, p in m.named_parameters():
                if p.grad is None:
                    continue
                if name == "ray_preprocessor.mlp2.0.weight":
                    out[name + "[:, :512]"], out[name + "[:, 512:]"] = p.grad[:, :512].clone(), p.grad[:, 512:].clone()
                else:
                    out[name] = p.grad.detach().clone()
            return out

        ref = run(idm64, False)
        f32 = run(idm, False)
        got = run(idm, True)
        assert set(got) == set(ref) == set(f32) and len(ref) == 3 + 13
        floor = U * max(16.0, math.sqrt(r))
        worst = 0.0
        for name in ref:
            e_h, e_32 = _rel_max(got[name], ref[name]), _rel_max(f32[name], ref[name])
            assert e_h <= 4 * e_32 + floor, (r, name, e_h, e_32)
            worst = max(worst, e_h / (4 * e_32 + floor))
        print(f"R={r}: largest HIP error / bound {worst:.2f}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. one full training step
# ------------------------------------------------------------------------------------------------------------------------------
def _target64(ori, dr, pose, n_tokens):
    """distance_based_loss.py's target scores (device_math.h: distance_target, then the rescale to n_tokens) in fp64.
    Returns (targets, raw targets, raw sum)."""
    c, zc = pose[:3, 3], pose[:3, 2]
    t = ((c - ori) * dr).sum(-1)
    cl = torch.where((t < 0)[:, None], ori, ori + t[:, None] * dr)
    p = ((ori - c) * zc).sum(-1)
    raw = (1 - torch.tanh((cl - c).norm(dim=-1))) * ((p / p.abs() + 1) / 2)
    s = raw.sum()
    return raw * ((1 / s) * n_tokens), raw, s


def test_training_step_against_fp64(pkg, golden):
    """test_training_step_gradients_match_the_reference's step (its image-side boundary inputs, its fixed torch.randperm,
    DistanceBasedScoreLoss + 0.1 x camera-up, backward of combined / 32) on the HIP path, against the same module in fp64 with
    hip_autograd=False and targets from the fp64 formula: scores, loss, and all 24 parameter gradients.

    Bound as test_ray_mlp_and_projections_against_fp64: the error of the fp32 PyTorch step (hip_autograd=False, fp32 targets) against
    fp64 is the yardstick; the HIP step may be at most 4 x that plus u sqrt(R) (R = the rays of the step), relative to the largest fp64
    entry of each gradient.  The biases of mlp2.2 and k_proj shift every logit of a token equally, so their true gradient is 0: both
    steps return rounding noise of a sum over the rays, and for them the error is taken relative to max_j sum_r |dL/dy_rj| of the layer
    instead.  Rays at a ReLU tie of the ray MLP, or within rounding of the camera plane (where fp32 may flip the target's sign term),
    are dropped from the permutation."""
    import torch.nn.functional as F
    g, g7 = golden("g10_train_step"), golden("g7_e2e")
    n = int(g["n_rays"])
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    ori, dr, rgb = G(g7["n3000_p50_ori"][:n]), G(g7["n3000_p50_dir"][:n]), G(g7["n3000_p50_rgb"][:n])
    tok_pe, fmap, pose = G(g7["e2e0_tokens"]), G(g7["e2e0_fmap"]), G(g7["e2e0_gt_c2w"])
    idm, idm64 = _scorer(pkg, with_cnn=True), _scorer(pkg, with_cnn=True).double()
    idm64.hip_autograd = False
    perm = G(g["perm"])
    c64, z64 = pose.double()[:3, 3], pose.double()[:3, 2]
    plane = (((ori.double() - c64) * z64).sum(-1).abs() / ((ori.double() - c64).abs() @ z64.abs()))
    ok = (_ray_margin(idm64, ori, dr, rgb) > MARGIN) & (plane > MARGIN)
    perm = perm[ok[perm]]
    assert perm.numel() >= 0.9 * n
    r = perm.numel()

    def step(m, use_hip):
        m.zero_grad()
        m.hip_autograd = use_hip
        dt = torch.float64 if m is idm64 else torch.float32
        tp, fm = tok_pe.to(dt), fmap.to(dt)
        m.backbone_wrapper.forward = lambda img, mask: (tp, fm.permute(1, 2, 0).reshape(-1, fm.shape[0]), fm)
        dy = {}

        def grab(name):
            def hook(mod, args, out):
                out.register_hook(lambda gr: dy.__setitem__(name, gr.detach().clone()))
            return hook

        hooks = [m.attention.k_proj.register_forward_hook(grab("attention.k_proj.bias")),
                 m.ray_preprocessor.mlp2[2].register_forward_hook(grab("ray_preprocessor.mlp2.2.bias"))]
        orig = torch.randperm
        torch.randperm = lambda *a, **k: perm
        try:
            scores, att, _, up, used = m(torch.zeros(8, 8, 3, device="cuda"), torch.ones(8, 8, dtype=torch.bool, device="cuda"),
                                         ori.to(dt), dr.to(dt), rgb.to(dt))
        finally:
            torch.randperm = orig
            for h in hooks:
                h.remove()
        model_up = torch.tensor([0.0, 1.0, 0.0], device="cuda", dtype=dt)
        if m is idm64:
            target = _target64(ori.double()[used], dr.double()[used], pose.double(), att.shape[-2])[0]
            loss_score = torch.square(scores - target).mean()
        else:
            loss_score, _ = pkg.DistanceBasedScoreLoss()(scores, pose, torch.eye(3).cuda(), ori[used], dr[used], att.shape[-2],
                                                         m.backbone_wrapper.backbone_wh, model_up=model_up)
        combined = loss_score + 0.1 * (-0.5 * F.cosine_similarity(model_up, up, dim=-1) + 0.5)
        (combined / 32).backward()
        grads = {name: p.grad.detach().clone() for name, p in m.named_parameters() if p.grad is not None}
        return scores.detach(), float(combined.detach()), grads, dy

    s64, l64, ref, dy64 = step(idm64, False)
    s32, l32, f32, _ = step(idm, False)
    sh, lh, got, _ = step(idm, True)
    assert set(ref) == set(got) == set(f32) and len(ref) == 24 and len(dy64) == 2
    floor = U * math.sqrt(r)
    e_h, e_32 = _rel_max(sh, s64), _rel_max(s32, s64)
    assert e_h <= 4 * e_32 + floor, ("scores", e_h, e_32)
    assert abs(lh - l64) <= 4 * abs(l32 - l64) + floor * abs(l64), ("loss", lh, l32, l64)
    worst = 0.0
    for name in ref:
        scale = float(dy64[name].abs().sum(0).max()) if name in dy64 else float(ref[name].abs().max())
        e_h = float((got[name].double() - ref[name]).abs().max()) / scale
        e_32 = float((f32[name].double() - ref[name]).abs().max()) / scale
        assert e_h <= 4 * e_32 + floor, (name, e_h, e_32)
        worst = max(worst, e_h / (4 * e_32 + floor))
    print(f"training step, R={r}: largest HIP error / bound {worst:.2f}")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. sixdgs_distance_target
# ------------------------------------------------------------------------------------------------------------------------------
def _distance_case(r, seed, nan_ray=False):
    """Rays around a random camera: origins ~ 2 N(0,1) about the centre, pulled in to within 6 of it (so that 1 - tanh(dist) stays
    far above the fp32 resolution), unit directions -- both branches of the closest point (t < 0 and t >= 0) and origins on both sides
    of the camera plane (a single ray is put in front of it).  Origins within rounding of the plane (|p| <= 2^-15 |o - c|.|z|, where
    fp32 may give the other sign) are moved off it; with nan_ray, ray r // 2 starts exactly at the camera centre (p = 0: sign term
    0/0)."""
    syn = importlib.import_module("6dgs_amd.synthetic")
    rng = np.random.default_rng(seed)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = syn.random_rotation(rng)
    pose[:3, 3] = 2.0 * rng.standard_normal(3)
    c, z = pose[:3, 3].astype(np.float64), pose[:3, 2].astype(np.float64)
    off = 2.0 * rng.standard_normal((r, 3))
    off *= np.minimum(1.0, 6.0 / np.linalg.norm(off, axis=1, keepdims=True))
    if r == 1:
        off[0] += (1.0 - off[0] @ z) * z                     # in front of the camera plane
    p = off @ z
    near = np.abs(p) <= TOL_K * (np.abs(off) @ np.abs(z))
    off[near] -= 0.5 * np.sign(p[near] + 0.25)[:, None] * z  # off the plane (stays within 6.5 of the centre)
    ori = (c + off).astype(np.float32)
    d = rng.standard_normal((r, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if nan_ray:
        ori[r // 2] = pose[:3, 3]
    return ori, d, pose


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("r", (1, 255, 257, 262143, 262145, 3000017))
def test_distance_target_against_fp64(ops, oracle, r):
    """ops.distance_target (k_distance_target + k_distance_scale) against the fp64 formula of device_math.h:distance_target and
    distance_based_loss.py's rescale, and against the oracle, at R in {1, 255, 257, 262 143, 262 145, 3 000 017} (the grid is capped at
    1024 x 256 threads: the last two run the grid-stride loops, the largest about 11 times per thread), n_tokens in {0, 1, 256}.

    Bounds, from the fp32 evaluation of the same formula: the raw target of a ray is off by A_i <= 32 u (1 + |o_i| + |c|) (v = c - o,
    t = v.d, the closest point, its distance: a few roundings of terms <= |o| + |c| each; tanh within 2 ulp and its slope <= 1;
    twice that for margin); the raw sum, taken in double and rounded to float, by sum_i A_i + u s; the rescaled target T_i = raw_i
    (1/s) n by m A_i + |T_i| (4u + sum A / s) with m = n / s.  The rescaled targets sum to n within 4u n whatever A is, since they are
    normalised by their own sum.  NaN and zero patterns match the oracle's; repeated calls are bit-identical."""
    ori, d, pose = _distance_case(r, 11 + r)
    o64, d64, pose64 = (torch.from_numpy(a).cuda().double() for a in (ori, d, pose))
    oc, dc, pc = (torch.from_numpy(a).cuda() for a in (ori, d, pose))
    t = ((pose64[:3, 3] - o64) * d64).sum(-1)
    p = ((o64 - pose64[:3, 3]) * pose64[:3, 2]).sum(-1)
    if r >= 255:
        assert bool((t < 0).any()) and bool((t >= 0).any()) and bool((p < 0).any()) and bool((p > 0).any())
    a = 32 * U * (1 + o64.norm(dim=-1) + float(pose64[:3, 3].norm()))
    for n_tok in (0, 1, 256):
        ref, raw, s64 = _target64(o64, d64, pose64, n_tok)
        tg, s = ops.distance_target(oc, dc, pc, n_tok, want_sum=True)
        tg2 = ops.distance_target(oc, dc, pc, n_tok)
        assert _same_bits(tg, tg2) and tg.dtype == torch.float32 and tg.shape == (r,)
        o_t, _ = oracle.distance_target(ori, d, pose, n_tok)
        o_t = torch.from_numpy(o_t).cuda()
        assert torch.equal(torch.isnan(tg), torch.isnan(ref)) and torch.equal(torch.isnan(tg), torch.isnan(o_t)), (r, n_tok)
        assert torch.equal(tg == 0, o_t == 0), (r, n_tok)
        fin = ~torch.isnan(ref)
        if not bool(fin.any()):                   # every raw target 0 (all rays behind the camera): 0 * (1/0) in both
            continue
        assert bool(fin.all())
        s64 = float(s64)
        sa = float(a.sum())
        assert abs(float(s) - s64) <= sa + U * s64, (r, n_tok, float(s), s64)
        m = n_tok / s64
        bound = m * a + ref.abs() * (4 * U + sa / s64)
        assert bool(((tg.double() - ref).abs() <= bound).all()), (r, n_tok, float(((tg.double() - ref).abs() / bound).max()))
        assert bool(((o_t.double() - ref).abs() <= bound).all()), (r, n_tok)
        assert abs(float(tg.double().sum()) - n_tok) <= 4 * U * n_tok + 1e-300, (r, n_tok, float(tg.double().sum()))


@pytest.mark.parametrize("r", (257, 3000017))
def test_distance_target_nan_ray_against_the_oracle(ops, oracle, r):
    """One ray starting exactly at the camera centre (p = 0: the reference's sign term is 0/0 = NaN) poisons the sum and with it every
    target, in the reference formula, in the oracle and in the kernel -- also through the grid-stride loop; want_sum returns NaN."""
    ori, d, pose = _distance_case(r, 5, nan_ray=True)
    oc, dc, pc = (torch.from_numpy(a).cuda() for a in (ori, d, pose))
    ref = _target64(*(torch.from_numpy(a).cuda().double() for a in (ori, d, pose)), 256)[0]
    tg, s = ops.distance_target(oc, dc, pc, 256, want_sum=True)
    o_t, _ = oracle.distance_target(ori, d, pose, 256)
    assert bool(torch.isnan(ref).all()) and bool(torch.isnan(tg).all()) and bool(np.isnan(o_t).all()) and bool(torch.isnan(s).all())
