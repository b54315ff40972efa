"""Fitting with densification on the GPU: sixdgs_fit_scene_steps from zeroed state against sixdgs_fit_scene and cut into segments,
bit for bit; fit_scene(backend="fused", densify=...) against the same run composed in Python from the parts, bit for bit; the torch
arm on the same schedule; the input scene stays untouched; a thinned stand-in grows back.  The fixture is test_gpu_fit_scene.py's,
rebuilt here: make_scene(2000, 0) and three 64 x 64 views drawn by the rasteriser.  Everything runs inside this process."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORDER = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")             # the rasteriser's argument order
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scale": "_scaling", "rot": "_rotation"}
PERTURB = {"f_dc": 0.3, "opacity": 0.5, "xyz": 0.002}
SIZE = 64
RATES = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)
# two rounds in 14 steps, the second one with the big-Gaussian prune and an opacity reset on its iteration; the thresholds sit inside
# this small fixture's distributions (about half of the average gradients are above 1e-3, some opacities below 0.2), so that every round
# clones, splits and prunes
DENSIFY = dict(from_iter=2, until_iter=13, interval=6, grad_threshold=1e-3, min_opacity=0.2, prune_big_after=6, seed=5)
STEPS, RESET_EVERY = 14, 12


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def fit(pkg):
    return importlib.import_module("6dgs_amd.fit")


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
    """test_gpu_fit_scene.py's: a duplicated view in one step, a reset at step 2, the SH degree rising at step 3, a changing rate."""
    views = np.array([[(s + b) % 3 for b in range(batch)] for s in range(steps)], np.int32)
    if batch > 1 and steps > 1:
        views[1, :2] = 2
    lrs = np.array([[RATES[0] * 0.9 ** s, *RATES[1:]] for s in range(steps)])
    degrees = np.array([1 if s < 3 else 3 for s in range(steps)], np.int32)
    resets = np.array([s == 2 for s in range(steps)])
    return views, lrs, degrees, resets


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fresh_state(ops, p):
    state = ops.gaussian_adam_state(p)
    state["instances_needed"] = torch.zeros(1, dtype=torch.int64, device="cuda")
    return state


@pytest.mark.parametrize("steps,batch", ((5, 1), (4, 3)))
def test_steps_from_zeroed_state_are_fit_scene_and_segments_compose(ops, fixture, steps, batch):
    f = fixture
    views, lrs, degrees, resets = schedule(steps, batch)
    capacity = ops.raster_instances_estimate(2000, batch)
    whole_p = params_of(f["moved"])
    whole = ops.fit_scene_raw(whole_p, f["rows"], SIZE, SIZE, f["target"], views=views, lrs=lrs, sh_degrees=degrees, resets=resets,
                              max_instances=capacity, retry=False)
    # one call from zeroed state
    one_p = params_of(f["moved"])
    one = fresh_state(ops, one_p)
    history = ops.fit_scene_steps_raw(one_p, f["rows"], SIZE, SIZE, f["target"], one, views=views, lrs=lrs, sh_degrees=degrees, resets=resets,
                                      max_instances=capacity)
    assert same(history, whole["history"]) and all(same(one[k], whole[k]) for k in ("m", "v", "status"))
    assert int(one["instances_needed"]) == whole["instances_needed"] > 0 and all(same(one_p[k], whole_p[k]) for k in one_p)
    # two segments, 2 steps and the rest, with the state carried over
    two_p = params_of(f["moved"])
    two = fresh_state(ops, two_p)
    parts = []
    for seg, first in ((slice(0, 2), 0), (slice(2, steps), 2)):
        parts.append(ops.fit_scene_steps_raw(two_p, f["rows"], SIZE, SIZE, f["target"], two, views=views[seg], lrs=lrs[seg], sh_degrees=degrees[seg],
                                             resets=resets[seg], first_adam_step=first, max_instances=capacity))
    assert same(torch.cat(parts), whole["history"]) and all(same(two[k], whole[k]) for k in ("m", "v", "status"))
    assert all(same(two_p[k], whole_p[k]) for k in two_p) and int(two["instances_needed"]) == whole["instances_needed"]


def test_a_step_without_update_moves_nothing_and_statistics_follow_the_backward(ops, fixture):
    """updates = 0: the scene, m, v stay; Adam's counter does not advance (the next update is step 0's); the statistics are those of
    ops.densify_stats behind the same pass."""
    f = fixture
    views, lrs, degrees, _ = schedule(3, 1)
    capacity = ops.raster_instances_estimate(2000, 1)
    p = params_of(f["moved"])
    state, stats = fresh_state(ops, p), ops.densify_stats_state(2000, "cuda")
    h0 = ops.fit_scene_steps_raw(p, f["rows"], SIZE, SIZE, f["target"], state, views=views[:1], lrs=lrs[:1], sh_degrees=degrees[:1], updates=[0],
                                 stats_steps=[1], stats=stats, max_instances=capacity)
    start = params_of(f["moved"])
    assert all(same(p[k], start[k]) for k in p) and not bool(state["m"].any()) and not bool(state["v"].any())
    scene = [start[k] for k in ORDER]
    cams = f["rows"][views[0].astype(np.int64)].contiguous()
    image, radii, fwd = ops.raster_views(*scene, int(degrees[0]), cams, SIZE, SIZE, want_float=True, want_u8=False, want_radii=True, want_state=True,
                                         max_instances=capacity)
    loss, grad = ops.photometric_loss(image, f["target"][views[0].astype(np.int64)].contiguous(), want_grad=True)
    bwd_ws = torch.empty(ops.raster_views_backward_workspace_bytes(2000, 1, SIZE, SIZE, capacity), dtype=torch.uint8, device="cuda")
    ops.raster_views_backward(*scene, int(degrees[0]), cams, SIZE, SIZE, grad, fwd, workspace=bwd_ws)
    hand = ops.densify_stats_state(2000, "cuda")
    ops.densify_stats(fwd, bwd_ws, radii, hand, SIZE, SIZE)
    assert same(h0[0], loss) and all(same(stats[k], hand[k]) for k in hand) and int(stats["denom"].sum()) > 500
    # the update that follows is Adam's step 0: the same bits as a fit that starts here
    h1 = ops.fit_scene_steps_raw(p, f["rows"], SIZE, SIZE, f["target"], state, views=views[:1], lrs=lrs[:1], sh_degrees=degrees[:1],
                                 max_instances=capacity)
    plain_p = params_of(f["moved"])
    plain = ops.fit_scene_raw(plain_p, f["rows"], SIZE, SIZE, f["target"], views=views[:1], lrs=lrs[:1], sh_degrees=degrees[:1], max_instances=capacity,
                              retry=False)
    assert same(h1, plain["history"]) and same(state["m"], plain["m"]) and all(same(p[k], plain_p[k]) for k in p)
    # a capacity too small: bit 1, a NaN row, and no statistics
    small_p, small_stats = params_of(f["moved"]), ops.densify_stats_state(2000, "cuda")
    small = fresh_state(ops, small_p)
    h = ops.fit_scene_steps_raw(small_p, f["rows"], SIZE, SIZE, f["target"], small, views=views[:2], lrs=lrs[:2], sh_degrees=degrees[:2],
                                stats_steps=[1, 1], stats=small_stats, max_instances=64)
    assert int(small["status"]) == ops.FIT_STATUS_CAPACITY and bool(torch.isnan(h).all()) and int(small["instances_needed"]) > 64
    assert not any(bool(t.any()) for t in small_stats.values()) and all(same(small_p[k], start[k]) for k in start)


def fit_lrs(fit, steps):
    return np.array([[fit.position_lr(s + 1), 2.5e-3, 2.5e-3 / 20.0, 0.05, 5e-3, 1e-3] for s in range(steps)])


def hand_fit(ops, fit, p, rows, target, views, lrs, degrees, plan, opts, ceiling=0.01):
    """fit_scene(backend="fused", densify=...) composed in Python from the parts."""
    steps, batch = views.shape
    n, n_coef = p["xyz"].shape[0], 1 + p["f_rest"].shape[1]
    state, stats = ops.gaussian_adam_state(p), ops.densify_stats_state(n, "cuda")
    history = torch.empty(steps, batch, device="cuda")
    rounds, updates = [], 0
    for s in range(steps):
        idx = torch.from_numpy(views[s].astype(np.int64)).cuda()
        cams, tgt = rows[idx].contiguous(), target[idx].contiguous()
        scene = [p[k] for k in ORDER]
        capacity = ops.raster_instances_estimate(n, batch)
        image, radii, needed, fwd = ops.raster_views(*scene, int(degrees[s]), cams, SIZE, SIZE, want_float=True, want_u8=False, want_radii=True,
                                                     want_instances=True, want_state=True, max_instances=capacity)
        assert needed <= capacity and fwd[1] == capacity
        loss, grad = ops.photometric_loss(image, tgt, want_grad=True)
        bwd_ws = torch.empty(ops.raster_views_backward_workspace_bytes(n, batch, SIZE, SIZE, capacity), dtype=torch.uint8, device="cuda")
        grads = ops.raster_views_backward(*scene, int(degrees[s]), cams, SIZE, SIZE, grad, fwd, workspace=bwd_ws, want=ORDER)
        history[s] = loss
        if plan["stats"][s]:
            ops.densify_stats(fwd, bwd_ws, radii, stats, SIZE, SIZE)
        if plan["update"][s]:
            ops.gaussian_adam(p, {k: g for k, g in zip(ops.RASTER_GRADIENTS, grads) if g is not None}, state, updates, lrs[s])
            updates += 1
        if plan["round"][s]:
            noise = fit.round_noise(n, opts["seed"], len(rounds), "cuda")
            p, new_state, counts = ops.densify(p, state, stats, noise, grad_threshold=opts["grad_threshold"], percent_dense=opts["percent_dense"],
                                               extent=opts["extent"], min_opacity=opts["min_opacity"], prune_big=bool(plan["prune_big"][s]),
                                               screen_size=opts["screen_size"])
            c = counts.cpu().tolist()
            rounds.append([s + 1, n, c[1], c[2], c[3], c[0]])
            n, state, stats = c[0], new_state, ops.densify_stats_state(c[0], "cuda")
        if plan["reset"][s]:
            sl = ops.gaussian_adam_slices(n, n_coef)["opacity"]
            ops.opacity_reset(p["opacity"], state["m"][sl], state["v"][sl], ceiling=ceiling)
    return p, state, history, torch.tensor(rounds, dtype=torch.int64).reshape(-1, 6)


@pytest.fixture(scope="module")
def both_backends(pkg, fixture):
    f = fixture
    before = params_of(f["moved"])
    kw = dict(steps=STEPS, batch=1, densify=DENSIFY, opacity_reset_every=RESET_EVERY, sh_degree_start=1, sh_up_every=5)
    out = {b: pkg.fit_scene(f["moved"], f["images"], f["c2w"], f["K"], backend=b, **kw) for b in ("fused", "torch")}
    return out, before


def test_fused_fit_with_densification_is_the_hand_composition_bit_for_bit(ops, fit, fixture, both_backends):
    f = fixture
    scene, rep = both_backends[0]["fused"]
    opts = fit.densify_options(DENSIFY)
    opts["extent"] = fit.cameras_extent(f["c2w"])
    plan = fit.densify_plan(STEPS, DENSIFY, RESET_EVERY, True)
    assert (np.nonzero(plan["round"])[0] + 1).tolist() == [6, 12] and (np.nonzero(plan["reset"])[0] + 1).tolist() == [12]
    assert plan["prune_big"][11] and not plan["prune_big"][5] and not plan["stats"][12:].any() and plan["update"].sum() == STEPS - 2
    views = rep["views"].cpu().numpy().astype(np.int32)
    degrees = np.minimum(1 + (np.arange(STEPS) + 1) // 5, 3)
    # the camera rows and the target as fit_scene makes them from the poses (the fixture's rows come from the renderer's cameras)
    refine = importlib.import_module("6dgs_amd.refine")
    target, rows, width, height = refine.posed_views(f["images"], *refine.check_poses(f["images"], f["c2w"], f["K"], min_views=1), "cuda", 1, "ignore",
                                                     (1.0, 1.0, 1.0))
    assert (width, height) == (SIZE, SIZE) and torch.equal(target, f["target"])
    p, state, history, rounds = hand_fit(ops, fit, params_of(f["moved"]), rows, target, views, fit_lrs(fit, STEPS), degrees, plan, opts)
    print(f"rounds (iteration, n, clones, splits, pruned, n after): {rep['rounds'].tolist()}")
    assert torch.equal(rep["rounds"], rounds) and rounds.shape == (2, 6)
    assert bool((rounds[:, 2:5] > 0).all()), "the fixture's rounds do not all clone, split and prune"
    assert rounds[0, 1] == 2000 and rounds[1, 1] == rounds[0, 5] and rep["n_final"] == int(rounds[1, 5]) == len(scene) != 2000
    assert bool((rounds[:, 5] == rounds[:, 1] + rounds[:, 2] + rounds[:, 3] - rounds[:, 4]).all())
    assert same(rep["loss_history"], history) and bool(torch.isfinite(history).all()) and int(rep["status"]) == 0
    for k, a in ATTR.items():
        assert same(getattr(scene, a), p[k]), k
    assert scene.active_sh_degree == 3
    # after the reset on the last round's iteration every opacity is at most the ceiling (two more updates moved them a little)
    assert float(torch.sigmoid(scene._opacity).max()) < 0.05


def test_torch_arm_runs_the_same_schedule(fixture, both_backends):
    (scene_f, rep_f), (scene_t, rep_t) = both_backends[0]["fused"], both_backends[0]["torch"]
    assert rep_t["loss_history"].shape == (STEPS, 1) and bool(torch.isfinite(rep_t["loss_history"]).all()) and int(rep_t["status"]) == 0
    assert torch.equal(rep_t["views"], rep_f["views"]) and same(rep_t["loss_history"][0], rep_f["loss_history"][0])
    rt, rf = rep_t["rounds"], rep_f["rounds"]
    print(f"torch arm's rounds: {rt.tolist()}; max |history - fused's| {float((rep_t['loss_history'] - rep_f['loss_history']).abs().max()):.3e}")
    assert rt.shape == rf.shape == (2, 6) and rt.dtype == torch.int64 and torch.equal(rt[:, 0], rf[:, 0]) and rt[0, 1] == 2000
    assert rt[1, 1] == rt[0, 5] and rep_t["n_final"] == int(rt[1, 5]) == len(scene_t)
    assert bool((rt[:, 5] == rt[:, 1] + rt[:, 2] + rt[:, 3] - rt[:, 4]).all())
    for scene in (scene_t, scene_f):
        assert all(getattr(scene, a).shape[0] == len(scene) and getattr(scene, a).is_cuda for a in ATTR.values())


def test_input_scene_is_unchanged(fixture, both_backends):
    _, before = both_backends
    for k, a in ATTR.items():
        assert same(getattr(fixture["moved"], a), before[k]), k


def test_thinned_scene_grows_and_the_loss_falls(pkg, fixture):
    """Half of the Gaussians removed and the rest enlarged by a half: the fit adds Gaussians, and the last pass's loss is below the
    first's.  One round, after the statistics of ten passes, and thirty steps to settle: a round first RAISES the loss (a clone doubles
    its source's opacity where it stands), so rounds a few steps apart, as in the bit-for-bit test above, never settle; the threshold
    sits in the upper quarter of this fixture's average gradients.  (No comparison with a fixed-n fit is asserted: see
    profiles/densify.md.)"""
    f = fixture
    gen = torch.Generator().manual_seed(9)
    keep = torch.randperm(2000, generator=gen)[:1000].sort().values.cuda()
    thin = pkg.GaussianScene(f["scene"].max_sh_degree)
    for k, a in ATTR.items():
        setattr(thin, a, getattr(f["scene"], a)[keep].clone() + (float(np.log(1.5)) if k == "scale" else 0.0))
    new, rep = pkg.fit_scene(thin, f["images"], f["c2w"], f["K"], steps=40, backend="fused",
                             densify=dict(from_iter=5, until_iter=15, interval=10, grad_threshold=5e-3))
    h = rep["loss_history"]
    print(f"thinned stand-in: n 1000 -> {rep['n_final']}, rounds {rep['rounds'].tolist()}, loss {float(h[:3].mean()):.5f} -> {float(h[-3:].mean()):.5f}")
    assert rep["n_final"] == len(new) > 1000 and rep["rounds"].shape[0] == 1 and int(rep["status"]) == 0
    assert float(h[-3:].mean()) < float(h[:3].mean())
