"""sixdgs_raster_views and sixdgs_raster_views_backward on the GPU against fp64 in the parameterisations they accept beyond the corner
test_gpu_raster.py and test_gpu_raster_backward.py cover: an active SH degree below the stored one, raw scales, raw opacities,
scale_modifier != 1; more than 65 536 Gaussians through the backward (a second staging round of k_raster_cams_bwd); an early stop inside
a tile whose list takes several rounds, in workspaces filled with NaN; and the same switches through the fused entry points.  The
restatements are tests/raster_reference.py and tests/raster_backward_reference.py, the bounds are theirs, and
tests/test_raster_parameterisation_host.py asserts without a GPU that every case here is fit; the two larger scenes are built in
tests/raster_parameterisation_cases.py.  Everything runs inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_parameterisation_cases as PC  # noqa: E402
import raster_reference as RR  # noqa: E402
import test_gpu_evaluate_views as TE  # noqa: E402
import test_gpu_fit_scene as TF  # noqa: E402
import test_gpu_raster as TR  # noqa: E402
import test_gpu_raster_backward as TB  # noqa: E402
import test_gpu_raster_contrib as TC  # noqa: E402
import test_gpu_refine_fused as TP  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, SCENE_SEED, VIEWS, CAM_SEED, WIDTH, HEIGHT = RB.PARAM_BASE
GAUSSIAN_KEYS = RB.NAMES[:-1]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def _flags(kw):
    return {k: v for k, v in kw.items() if k != "stored_degree"}


def _gpu(ops, scene, rows, width, height, g, fill=None, **flags):
    """Forward and backward with the capacity the scene needs -> (float image, uint8 image, radii, instances, dict of the gradients),
    as numpy.  fill: both calls run in workspaces of exactly *_workspace_bytes, every byte set to `fill` before the call."""
    args, cams = TB._dev(scene), torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    n, views = scene["xyz"].shape[0], rows.shape[0]
    kw = dict(background=RR.BACKGROUND, **flags)
    cap = max(ops.raster_views(*args, cams, width, height, want_u8=False, want_instances=True, **kw), 1)
    fwd_ws = bwd_ws = None
    if fill is not None:
        fwd_ws = torch.full((ops.raster_views_workspace_bytes(n, views, width, height, cap),), fill, dtype=torch.uint8, device="cuda")
        bwd_ws = torch.full((ops.raster_views_backward_workspace_bytes(n, views, width, height, cap),), fill, dtype=torch.uint8, device="cuda")
    img_f, img_u, radii, count, state = ops.raster_views(*args, cams, width, height, channels=4, want_float=True, want_radii=True,
                                                         want_instances=True, want_state=True, max_instances=cap, workspace=fwd_ws, **kw)
    assert fill is None or (state[0].data_ptr() == fwd_ws.data_ptr() and state[1] == cap)
    grads = ops.raster_views_backward(*args, cams, width, height, torch.from_numpy(np.array(g, np.float32)).cuda(), state, workspace=bwd_ws, **kw)
    return img_f.cpu().numpy(), img_u.cpu().numpy(), radii.cpu().numpy(), count, {k: v.cpu() for k, v in zip(RB.NAMES, grads)}


def _check(ops, c, width, height, what, skip=(), fill=None, **flags):
    """One case (an RB.case / RB.measure dict) against fp64: the float image under RR.bound, the uint8 image within one step, radii on
    the decidable Gaussians, the instance count in the reference's band, the seven gradient arrays under RB.bounds."""
    rr = c["rr"]
    limit = RR.bound(rr["rounding"])
    assert limit <= RR.ERROR_CEILING and rr["undecidable"].mean() <= RR.MAX_UNDECIDABLE_SHARE
    img_f, img_u, radii, count, got = _gpu(ops, c["scene"], c["rows"], width, height, c["g"], fill=fill, **flags)
    TR._compare(img_f, img_u, rr["r64"]["image"], rr["undecidable"], limit, what)
    assert np.array_equal(radii[rr["decidable"]], rr["r64"]["radii"][rr["decidable"]]), f"{what}: radii differ on decidable Gaussians"
    assert rr["r64"]["instances_lo"] <= count <= rr["r64"]["instances_hi"], (what, count, rr["r64"]["instances"])
    for k in RB.NAMES:
        assert got[k].dtype == torch.float32 and got[k].shape == (c["rows"].shape if k == "cams" else c["scene"][k].shape), k
    TB._compare(got, c["g64"], c["bounds"], what, skip=skip)
    return img_f, img_u, radii, count, {k: v.numpy() for k, v in got.items()}


@pytest.mark.parametrize("name,args,kw", RB.PARAM_CASES, ids=[c[0] for c in RB.PARAM_CASES])
def test_parameterisations_against_fp64(ops, syn, name, args, kw):
    """Measured on MI355X, max |gpu - fp64| / bound per case and array: see profiles/raster_views.md and profiles/raster_backward.md.
    With raw arrays d scale and d opacity are by the raw values (the restatement differentiates by what it is given)."""
    c = RB.case(syn, *args, **kw)
    degree = args[6]
    got = _check(ops, c, WIDTH, HEIGHT, name, **_flags(kw))[4]
    nb = (degree + 1) ** 2
    assert not got["f_rest"][:, nb - 1:].any(), "d f_rest past the active degree is not exactly zero"
    assert degree == 0 or np.abs(got["f_rest"][:, :nb - 1]).max(axis=(0, 2)).min() > 0


def test_autograd_function_with_every_switch(ops, syn):
    """6dgs_amd.autograd.raster_views with raw scales, raw opacities, a scale modifier and degree 1 of 16: the bytes of the plain calls."""
    autograd = importlib.import_module("6dgs_amd.autograd")
    flags = dict(scale_is_log=False, opacity_is_logit=False, scale_modifier=1.7)
    scene = RR.raw_scene(syn.make_scene(N, SCENE_SEED), False, False)
    scene["sh_degree"] = 1
    rows = RR.camera_rows(syn.make_cameras(VIEWS, CAM_SEED, width=WIDTH, height=HEIGHT))
    g = np.random.default_rng(2).standard_normal((VIEWS, HEIGHT, WIDTH, 4)).astype(np.float32)
    img_f, _, _, _, plain = _gpu(ops, scene, rows, WIDTH, HEIGHT, g, **flags)
    default = _gpu(ops, scene, rows, WIDTH, HEIGHT, g)[0]
    assert not np.array_equal(img_f, default)
    leaves = [t.clone().requires_grad_(True) for t in TB._dev(scene)[:6] + [torch.from_numpy(rows).cuda()]]
    image = autograd.raster_views(*leaves[:6], 1, leaves[6], WIDTH, HEIGHT, background=RR.BACKGROUND, **flags)
    assert np.array_equal(image.detach().cpu().numpy(), img_f)
    image.backward(torch.from_numpy(g).cuda())
    for t, k in zip(leaves, RB.NAMES):
        assert torch.equal(t.grad.cpu(), plain[k]) and bool(plain[k].any()), k


# ---- more than 65 536 Gaussians through the backward -------------------------------------------------------------------------------------
def test_more_than_65536_gaussians(ops, syn):
    """k_raster_cams_bwd stages 256 blocks' camera partials per round: 66 000 Gaussians are 258 blocks, live ones in blocks 0, 255, 256
    and 257.  The image, the instance count, all gradients under the usual bounds, exact zeros on the filler rows, and d_cams bit for bit
    that of one view at a time."""
    c, filler = PC.check_big_case(syn)
    img_f, _, radii, count, got = _check(ops, c, WIDTH, HEIGHT, f"n={PC.BIG_N}")
    small = RB.case(syn, *RB.PARAM_BASE, 3)["rr"]["r64"]
    assert (c["rr"]["r64"]["instances_lo"], c["rr"]["r64"]["instances_hi"]) == (small["instances_lo"], small["instances_hi"])       # the band _check held it in
    assert not radii[:, filler].any()
    for k in GAUSSIAN_KEYS:
        assert not got[k][filler].any(), f"d {k} is not exactly zero on a culled Gaussian"
        assert np.abs(got[k][PC.BIG_SLOTS]).max() > 0
    for v in range(VIEWS):
        one = _gpu(ops, c["scene"], c["rows"][v:v + 1], WIDTH, HEIGHT, c["g"][v:v + 1])
        assert np.array_equal(one[0][0], img_f[v]) and np.array_equal(one[4]["cams"][0].numpy(), got["cams"][v]), v


# ---- an early stop inside a tile whose list takes several rounds --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("A", "B"))
def test_early_stop_inside_a_multi_round_tile_in_poisoned_workspaces(ops, which):
    """Both workspaces hold 0xFF bytes (NaN as float) before each call: k_raster_blend_bwd has no memset, so every slot no pixel reached
    must get its explicit zero -- whole rounds (base >= hi) and the rest of the round the last pixel stopped in.  Against fp64 under the
    usual rules (d rot of these isotropic Gaussians as in test_gpu_raster_backward._hand_check), exact zeros behind the stop, no NaN,
    and the bytes of the same calls in zero-filled workspaces."""
    c, order, first_unused = PC.early_stop_case(which)
    img_f, _, _, count, got = _check(ops, c, 16, 16, f"early stop {which}", skip=("rot",), fill=0xFF)
    assert count == c["scene"]["xyz"].shape[0]
    assert all(np.isfinite(v).all() for v in got.values()) and np.isfinite(img_f).all()
    assert np.abs(got["rot"]).max() <= 1e-6 * np.abs(c["g64"]["log_scale"]).max()
    for k in GAUSSIAN_KEYS:
        assert not got[k][order[first_unused:]].any(), f"d {k} is not exactly zero behind the stop"
    zeroed = _gpu(ops, c["scene"], c["rows"], 16, 16, c["g"], fill=0)
    assert np.array_equal(zeroed[0], img_f) and all(np.array_equal(zeroed[4][k].numpy(), got[k]) for k in RB.NAMES)
    if which == "A":            # the image is that of the first two Gaussians alone, bit for bit
        two = {k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in c["scene"].items()}
        assert np.array_equal(_gpu(ops, two, c["rows"], 16, 16, c["g"], fill=0xFF)[0], img_f)
        assert (img_f[..., 1] < 1e-3).all() and (img_f[..., 3] > 0.999).all()            # no green but the background's 0.5 T: the third was not added


def test_poisoned_workspaces_give_the_bytes_of_zeroed_ones(ops, syn):
    name, args, kw = RB.PARAM_CASES[np.random.default_rng(4).integers(len(RB.PARAM_CASES))]
    c = RB.case(syn, *args, **kw)
    a = _gpu(ops, c["scene"], c["rows"], WIDTH, HEIGHT, c["g"], fill=0xFF, **_flags(kw))
    b = _gpu(ops, c["scene"], c["rows"], WIDTH, HEIGHT, c["g"], fill=0, **_flags(kw))
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] > 0, name
    for k in RB.NAMES:
        assert torch.equal(a[4][k], b[4][k]) and bool(torch.isfinite(a[4][k]).all()), (name, k)


# ---- the switches through the fused entry points -----------------------------------------------------------------------------------------
FUSED = dict(scale_is_log=False, opacity_is_logit=False, scale_modifier=1.7)       # with degree 1 of the 16 stored coefficients
FUSED_DEGREE, SIZE = 1, TF.SIZE


@pytest.fixture(scope="module")
def fused(pkg, syn):
    """The fixture the four consumer tests share -- make_scene(2000, 0) and three 64 x 64 views drawn by the rasteriser -- with the scene's
    scales and opacities stored raw."""
    render = importlib.import_module("6dgs_amd.render")
    stored = syn.make_scene(2000, 0)
    views = render.render_views(pkg.GaussianScene.from_dict(stored, device="cuda"), syn.make_cameras(3, 21, width=SIZE, height=SIZE), renderer="raster")
    scene = RR.raw_scene(stored, False, False)
    rows = render.camera_rows(views)
    target = torch.stack([torch.from_numpy(np.ascontiguousarray(v.image[..., :3])) for v in views]).cuda().contiguous()
    return dict(scene=scene, arrays=TB._dev(scene)[:6], rows_np=rows, rows=torch.from_numpy(rows).cuda(), target=target)


def test_refine_poses_raw_takes_the_switches(ops, fused):
    f = fused
    delta = torch.tensor([[s * o for o in TP.OFFSET] for s in (1.0, -1.0, 0.5)], dtype=torch.float32, device="cuda")
    start = ops.pose_compose(f["rows"], delta)
    capacity = ops.raster_instances_estimate(2000, 3)
    got = ops.refine_poses_raw(*f["arrays"], FUSED_DEGREE, start, SIZE, SIZE, f["target"], steps=4, max_instances=capacity, retry=False, **FUSED)
    hand = TP.hand_loop(ops, f["arrays"], FUSED_DEGREE, start, SIZE, SIZE, f["target"], 4, capacity, raster=FUSED)
    for k in TP.RAW:
        assert got[k].dtype == hand[k].dtype and torch.equal(got[k], hand[k]), k
    assert got["instances_needed"] == hand["instances_needed"] > 0 and not bool(got["status"].any()) and bool(torch.isfinite(got["history"]).all())
    plain = ops.refine_poses_raw(*f["arrays"], FUSED_DEGREE, start, SIZE, SIZE, f["target"], steps=4)
    assert not torch.equal(plain["history"], got["history"])


def test_fit_scene_raw_takes_the_switches(ops, fused):
    """Without resets: a raw opacity forbids them."""
    f = fused
    views, lrs, degrees, resets = TF.schedule(3, 2)
    degrees[:], resets[:] = FUSED_DEGREE, False
    lrs = 0.1 * lrs                                        # raw scales are some 1e-2: steps of the log-scale's rate would cross zero
    capacity = ops.raster_instances_estimate(2000, 2)
    start = dict(zip(TF.ORDER, f["arrays"]))
    got_p, hand_p = ({k: v.clone() for k, v in start.items()} for _ in range(2))
    got = ops.fit_scene_raw(got_p, f["rows"], SIZE, SIZE, f["target"], views=views, lrs=lrs, sh_degrees=degrees, resets=resets,
                            max_instances=capacity, retry=False, **FUSED)
    hand = TF.hand_loop(ops, hand_p, f["rows"], f["target"], views, lrs, degrees, resets, ops.FIT_GROUPS, capacity, **FUSED)
    for k in ("history", "m", "v", "status"):
        assert TF.same(got[k], hand[k]), k
    for k in ops.FIT_GROUPS:
        assert TF.same(got_p[k], hand_p[k]) and not TF.same(got_p[k], start[k]), k
    assert got["instances_needed"] == hand["instances_needed"] > 0 and int(got["status"]) == 0 and bool(torch.isfinite(got["history"]).all())
    with pytest.raises(ValueError):
        ops.fit_scene_raw({k: v.clone() for k, v in start.items()}, f["rows"], SIZE, SIZE, f["target"], views=views, lrs=lrs, sh_degrees=degrees,
                          resets=np.array([False, True, False]), **FUSED)
    plain_p = {k: v.clone() for k, v in start.items()}
    plain = ops.fit_scene_raw(plain_p, f["rows"], SIZE, SIZE, f["target"], views=views, lrs=lrs, sh_degrees=degrees, resets=resets)
    assert not torch.equal(plain["history"], got["history"])


def test_evaluate_views_raw_takes_the_switches(ops, fused):
    f = fused
    want, want_render = TE.by_hand(ops, f, f["target"], True, sh_degree=FUSED_DEGREE, width=SIZE, height=SIZE, **FUSED)
    got = ops.evaluate_views_raw(*f["arrays"], FUSED_DEGREE, f["rows"], SIZE, SIZE, f["target"], quantise=True, chunk=2, want_render=True, **FUSED)
    assert TE.same(got["metrics"], want) and torch.equal(got["render"], want_render) and int(got["status"]) == 0
    assert bool(torch.isfinite(want).all()) and bool((want[:, 2] > 0).all())
    plain = ops.evaluate_views_raw(*f["arrays"], FUSED_DEGREE, f["rows"], SIZE, SIZE, f["target"], quantise=True, chunk=2)
    assert not torch.equal(plain["metrics"], got["metrics"])


def test_scene_contrib_raw_takes_the_switches(ops, fused):
    f = fused
    keys = TC.ACCS + ("view_weight", "view_pixels")
    want, _, _ = TC._measure(ops, f["scene"], f["rows_np"], SIZE, SIZE, sh_degree=FUSED_DEGREE, **FUSED)
    got = ops.scene_contrib_raw(*f["arrays"], FUSED_DEGREE, f["rows"], SIZE, SIZE, chunk=2, want_views=True, **FUSED)
    assert TC._equal(got, want, keys) and int(got["status"]) == 0 and int((got["pixels"] > 0).sum()) > 0
    plain = ops.scene_contrib_raw(*f["arrays"], FUSED_DEGREE, f["rows"], SIZE, SIZE, chunk=2, want_views=True)
    assert not torch.equal(plain["weight"], got["weight"])
