"""Fitting a scene's Gaussians on the GPU: sixdgs_fit_scene against the same loop composed in Python from the parts, bit for bit;
determinism; the capacity protocol; fit_scene with backend="fused" against backend="torch" on a perturbed copy of the scene that
rendered the views; the input scene stays untouched.  The fixture is the refinement fixture's size: make_scene(2000, 0) and three
64 x 64 views drawn by the rasteriser.  Everything runs inside this process."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORDER = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")             # the rasteriser's argument order
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scale": "_scaling", "rot": "_rotation"}
# the perturbation of the scene that rendered the views (standard deviations): colours, opacity logits, positions
PERTURB = {"f_dc": 0.3, "opacity": 0.5, "xyz": 0.002}
SIZE = 64
RATES = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def fixture(pkg, ops, syn):
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 0), device="cuda")
    views = render.render_views(scene, syn.make_cameras(3, 21, width=SIZE, height=SIZE), renderer="raster")
    c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
    rows = torch.from_numpy(render.camera_rows(views)).cuda()
    images = [v.image for v in views]
    target = torch.stack([torch.from_numpy(np.ascontiguousarray(im[..., :3])) for im in images]).cuda().contiguous()
    gen = torch.Generator().manual_seed(3)
    moved = pkg.GaussianScene(scene.max_sh_degree)
    for k, a in ATTR.items():
        t = getattr(scene, a).clone()
        if k in PERTURB:
            t += (PERTURB[k] * torch.randn(t.shape, generator=gen)).cuda()
        setattr(moved, a, t)
    return dict(scene=scene, moved=moved, images=images, c2w=torch.stack(c2w), K=torch.stack(Ks), rows=rows, target=target)


def params_of(scene):
    return {k: getattr(scene, a).detach().clone().contiguous() for k, a in ATTR.items()}


def schedule(steps, batch):
    """views, rates, degrees, resets of a case: a duplicated view in one step, a reset at step 2, the SH degree rising from 1 to 3 at
    step 3, a position rate that changes every step."""
    views = np.array([[(s + b) % 3 for b in range(batch)] for s in range(steps)], np.int32)
    if batch > 1 and steps > 1:
        views[1, :2] = 2
    lrs = np.array([[RATES[0] * 0.9 ** s, *RATES[1:]] for s in range(steps)])
    degrees = np.array([3] if steps == 1 else [1 if s < 3 else 3 for s in range(steps)], np.int32)
    resets = np.array([s == 2 for s in range(steps)])
    return views, lrs, degrees, resets


def hand_loop(ops, p, rows, target, views, lrs, degrees, resets, groups, capacity, lam=0.2, eps=1e-15, ceiling=0.01, **raster):
    """sixdgs_fit_scene composed in Python from its parts, on the dict p (in place); raster: scale_modifier, scale_is_log and
    opacity_is_logit of both rasteriser calls."""
    steps, batch = views.shape
    n, n_coef = p["xyz"].shape[0], 1 + p["f_rest"].shape[1]
    state = ops.gaussian_adam_state(p)
    sl = ops.gaussian_adam_slices(n, n_coef)["opacity"]
    history = torch.empty(steps, batch, device="cuda")
    needed_max = 0
    for s in range(steps):
        idx = torch.from_numpy(views[s].astype(np.int64)).cuda()
        cams, tgt = rows[idx].contiguous(), target[idx].contiguous()
        scene = [p[k] for k in ORDER]
        image, needed, fwd = ops.raster_views(*scene, int(degrees[s]), cams, SIZE, SIZE, want_float=True, want_u8=False, want_instances=True,
                                              want_state=True, max_instances=capacity, **raster)
        assert needed <= capacity and fwd[1] == capacity
        needed_max = max(needed_max, needed)
        loss, grad = ops.photometric_loss(image, tgt, lambda_dssim=lam, want_grad=True)
        grads = ops.raster_views_backward(*scene, int(degrees[s]), cams, SIZE, SIZE, grad, fwd, want=tuple(k for k in ORDER if k in groups),
                                          **raster)
        history[s] = loss
        ops.gaussian_adam(p, {k: g for k, g in zip(ops.RASTER_GRADIENTS, grads) if g is not None}, state, s, lrs[s], eps=eps,
                          instances=torch.tensor([needed], dtype=torch.int64, device="cuda"), max_instances=capacity)
        if resets[s]:
            ops.opacity_reset(p["opacity"], state["m"][sl], state["v"][sl], ceiling=ceiling, opacity_is_logit=raster.get("opacity_is_logit", True))
    return dict(history=history, m=state["m"], v=state["v"], status=state["status"], instances_needed=needed_max)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("steps,batch,kind,groups", ((1, 1, "f32", None), (5, 1, "u8", None), (4, 3, "u8", None), (4, 1, "u8", ("f_dc", "f_rest"))))
def test_loop_is_the_hand_composition_bit_for_bit(ops, fixture, steps, batch, kind, groups):
    f = fixture
    groups = ops.FIT_GROUPS if groups is None else groups
    target = f["target"] if kind == "u8" else (f["target"].float() / 255.0).contiguous()
    views, lrs, degrees, resets = schedule(steps, batch)
    if "opacity" not in groups:
        resets[:] = False                  # the C call resets whatever group_mask says; fit_scene asks for it only when the opacity moves
    capacity = ops.raster_instances_estimate(2000, batch)
    start = params_of(f["moved"])
    fused_p, hand_p = params_of(f["moved"]), params_of(f["moved"])
    fused = ops.fit_scene_raw(fused_p, f["rows"], SIZE, SIZE, target, views=views, lrs=lrs, sh_degrees=degrees, resets=resets, groups=groups,
                              max_instances=capacity, retry=False)
    hand = hand_loop(ops, hand_p, f["rows"], target, views, lrs, degrees, resets, groups, capacity)
    assert fused["history"].shape == (steps, batch) and bool(torch.isfinite(fused["history"]).all())
    for k in ("history", "m", "v", "status"):
        assert same(fused[k], hand[k]), k
    for k in ops.FIT_GROUPS:
        assert same(fused_p[k], hand_p[k]), k
        assert same(fused_p[k], start[k]) == (k not in groups), k              # the groups move, the frozen arrays keep the input's bits
    assert fused["instances_needed"] == hand["instances_needed"] > 0 and int(fused["status"]) == 0 and fused["max_instances"] == capacity
    if batch > 1:
        assert same(fused["history"][1, 0], fused["history"][1, 1])                      # the duplicated view: the same loss twice


def test_same_bytes_twice(ops, fixture):
    f = fixture
    views, lrs, degrees, resets = schedule(4, 3)
    runs = []
    for _ in range(2):
        p = params_of(f["moved"])
        out = ops.fit_scene_raw(p, f["rows"], SIZE, SIZE, f["target"], views=views, lrs=lrs, sh_degrees=degrees, resets=resets)
        runs.append((p, out))
    (p0, o0), (p1, o1) = runs
    assert all(same(p0[k], p1[k]) for k in p0) and all(same(o0[k], o1[k]) for k in ("history", "m", "v", "status"))
    assert o0["instances_needed"] == o1["instances_needed"]


def test_capacity_protocol(ops, fixture):
    f = fixture
    views, lrs, degrees, resets = schedule(4, 1)
    kw = dict(views=views, lrs=lrs, sh_degrees=degrees, resets=resets)
    ample_p = params_of(f["moved"])
    ample = ops.fit_scene_raw(ample_p, f["rows"], SIZE, SIZE, f["target"], **kw)
    need = ample["instances_needed"]
    assert int(ample["status"]) == 0 and need > 64
    small_p = params_of(f["moved"])
    small = ops.fit_scene_raw(small_p, f["rows"], SIZE, SIZE, f["target"], max_instances=need - 1, retry=False, **kw)
    assert int(small["status"]) == ops.FIT_STATUS_CAPACITY and small["instances_needed"] == need and small["max_instances"] == need - 1
    nan_rows = torch.isnan(small["history"]).all(dim=1).cpu().numpy()
    first = int(np.argmax(nan_rows))
    assert nan_rows[first:].all() and not nan_rows[:first].any() and same(small["history"][:first], ample["history"][:first])
    # the scene, m and v are the hand loop's, stopped before the step that overflowed
    hand_p = params_of(f["moved"])
    if first > 0:
        hand = hand_loop(ops, hand_p, f["rows"], f["target"], views[:first], lrs[:first], degrees[:first], resets[:first], ops.FIT_GROUPS, 4 * need)
        assert same(small["m"], hand["m"]) and same(small["v"], hand["v"])
    else:
        assert not bool(small["m"].any()) and not bool(small["v"].any())
    assert all(same(small_p[k], hand_p[k]) for k in hand_p)
    # with retry the call starts again from the scene as it was and gives the ample run's bytes
    rerun_p = params_of(f["moved"])
    rerun = ops.fit_scene_raw(rerun_p, f["rows"], SIZE, SIZE, f["target"], max_instances=need - 1, **kw)
    assert int(rerun["status"]) == 0 and rerun["max_instances"] > need - 1
    assert all(same(rerun_p[k], ample_p[k]) for k in ample_p) and all(same(rerun[k], ample[k]) for k in ("history", "m", "v"))


@pytest.fixture(scope="module")
def both_backends(pkg, fixture):
    f = fixture
    before = params_of(f["moved"])
    out = {b: pkg.fit_scene(f["moved"], f["images"], f["c2w"], f["K"], steps=40, batch=1, backend=b) for b in ("torch", "fused")}
    return out, before


def test_fused_fit_reduces_the_loss_as_the_torch_arm_does(ops, fixture, both_backends):
    f = fixture
    (out, _) = both_backends
    (scene_t, rep_t), (scene_f, rep_f) = out["torch"], out["fused"]
    # the common starting loss: the mean over the three views of the perturbed scene's loss
    image = ops.raster_views(*[getattr(f["moved"], ATTR[k]) for k in ORDER], 3, f["rows"], SIZE, SIZE, want_float=True, want_u8=False)
    start = float(ops.photometric_loss(image, f["target"]).mean())
    last_t, last_f = float(rep_t["loss_history"][-9:].mean()), float(rep_f["loss_history"][-9:].mean())           # the last three passes
    print(f"fit of 2000 Gaussians to three 64 x 64 views, 40 steps, perturbation {PERTURB}: mean loss {start:.5f} -> torch {last_t:.5f}, fused {last_f:.5f}; "
          f"max |history - torch's| {float((rep_f['loss_history'] - rep_t['loss_history']).abs().max()):.3e}")
    assert torch.equal(rep_t["views"], rep_f["views"]) and rep_t["views"].shape == (40, 1)
    for p0 in range(0, 39, 3):
        assert sorted(rep_t["views"][p0:p0 + 3, 0].tolist()) == [0, 1, 2]                                      # every view once per pass
    assert start - last_t >= 0.5 * start, "the torch arm alone does not halve the loss: the fixture's perturbation is unfit"
    assert start - last_f >= 0.9 * (start - last_t)
    # the same kernels on the same scene: the first loss is the torch arm's, bit for bit
    assert same(rep_f["loss_history"][0], rep_t["loss_history"][0])
    assert int(rep_f["status"]) == 0 and int(rep_t["status"]) == 0
    for rep in (rep_t, rep_f):
        assert rep["loss_history"].shape == (40, 1) and rep["loss_history"].dtype == torch.float32 and rep["status"].dtype == torch.int32
    for scene in (scene_t, scene_f):
        assert scene is not f["moved"] and len(scene) == 2000 and scene.active_sh_degree == 3 and scene.max_sh_degree == 3
        assert all(getattr(scene, a).shape == getattr(f["moved"], a).shape and getattr(scene, a).is_cuda for a in ATTR.values())


def test_input_scene_is_unchanged(fixture, both_backends):
    _, before = both_backends
    for k, a in ATTR.items():
        assert same(getattr(fixture["moved"], a), before[k]), k
