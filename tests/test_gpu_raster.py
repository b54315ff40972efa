"""sixdgs_raster_views on the GPU against the numpy restatement of its definition (tests/raster_reference.py): the float image against
fp64 within a bound taken from the restatement's own fp32 rounding, radii, the uint8 image, the edges of the definition, determinism,
batching, the instance capacity, and the full size.  Everything runs inside this process."""
import importlib
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C0 = 0.28209479177387814


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def _dev(scene):
    return [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + \
        [int(scene["sh_degree"])]


def _raster(ops, scene, rows, width, height, **kw):
    return ops.raster_views(*_dev(scene), torch.from_numpy(np.ascontiguousarray(rows)).cuda(), width, height, **kw)


def _u8(ref):
    return np.round(255.0 * np.clip(ref, 0.0, 1.0))


def _compare(got_f, got_u, r64, und, limit, what):
    """Float image within `limit` of fp64 on the decidable pixels (rgb and alpha); uint8 within one step.  -> the largest error."""
    ok = ~und
    err = np.abs(got_f.astype(np.float64) - r64)[ok]
    worst = float(err.max()) if err.size else 0.0
    step = np.abs(got_u.astype(np.int64) - _u8(r64)[..., :got_u.shape[-1]].astype(np.int64))[ok]
    print(f"{what}: max |gpu - fp64| {worst:.3e} (bound {limit:.3e}, ratio {worst / limit:.3f}); largest uint8 step {int(step.max()) if step.size else 0}; "
          f"undecidable {und.mean():.5f}")
    assert worst <= limit, f"{what}: {worst:.3e} > {limit:.3e} at {np.argwhere((np.abs(got_f.astype(np.float64) - r64).max(-1) > limit) & ok)[:3]}"
    assert not step.size or step.max() <= 1, f"{what}: a uint8 value is {int(step.max())} steps off"
    return worst


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", RR.CASES)
def test_image_radii_and_uint8_against_the_restatement(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """Measured on MI355X, max |gpu - fp64| / bound per case: see profiles/raster_views.md."""
    c = RR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    limit = RR.bound(c["rounding"])
    assert limit <= RR.ERROR_CEILING and c["undecidable"].mean() <= RR.MAX_UNDECIDABLE_SHARE
    img_f, img_u, radii, count = _raster(ops, c["scene"], c["rows"], width, height, channels=4, background=RR.BACKGROUND, want_float=True,
                                         want_radii=True, want_instances=True)
    assert img_f.shape == (views, height, width, 4) and img_f.dtype == torch.float32
    assert img_u.shape == (views, height, width, 4) and img_u.dtype == torch.uint8 and radii.shape == (views, n) and radii.dtype == torch.int32
    _compare(img_f.cpu().numpy(), img_u.cpu().numpy(), c["r64"]["image"], c["undecidable"], limit, f"n={n} {width}x{height} deg={sh_degree}")
    dec = c["decidable"]
    assert np.array_equal(radii.cpu().numpy()[dec], c["r64"]["radii"][dec]), "radii differ on decidable Gaussians"
    assert c["r64"]["instances_lo"] <= count <= c["r64"]["instances_hi"], (count, c["r64"]["instances"])
    img3 = _raster(ops, c["scene"], c["rows"], width, height, channels=3, background=RR.BACKGROUND)
    assert img3.shape == (views, height, width, 3) and torch.equal(img3, img_u[..., :3])


ROW = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 16.0, 16.0]], np.float32)       # identity pose, f = 20, 32 x 32


def _hand(xyz, sigma, o, colour):
    """A scene of isotropic-or-not Gaussians with given opacities (values in (0, 1)) and flat colours (SH degree 0)."""
    n = len(xyz)
    sigma = np.asarray(sigma, np.float64)
    sigma = np.broadcast_to(sigma.reshape(n, 1) if sigma.ndim == 1 else sigma, (n, 3))
    o = np.asarray(o, np.float64).reshape(n, 1)
    return {"xyz": np.asarray(xyz, np.float32).reshape(n, 3), "log_scale": np.log(sigma).astype(np.float32),
            "rot": np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (n, 1)), "opacity": np.log(o / (1 - o)).astype(np.float32),
            "f_dc": ((np.asarray(colour, np.float64).reshape(n, 1, 3) - 0.5) / C0).astype(np.float32), "f_rest": np.zeros((n, 0, 3), np.float32),
            "sh_degree": 0}


def _hand_check(ops, scene, what, background=(0.0, 0.0, 0.0)):
    """Render the hand-made scene at 32 x 32 and hold it against fp64 under the bound rule of the cases -> (float image, radii, r64)."""
    r64 = RR.reference_view(scene, ROW[0], 32, 32, np.float64, background=background)
    r32 = RR.reference_view(scene, ROW[0], 32, 32, np.float32, background=background)
    und = r64["undecidable"] | r32["undecidable"]
    rounding = np.abs(r32["image"].astype(np.float64) - r64["image"])[~und]
    limit = RR.bound(float(rounding.max()) if rounding.size else 0.0)
    assert limit <= RR.ERROR_CEILING
    img_f, img_u, radii = _raster(ops, scene, ROW, 32, 32, channels=4, background=background, want_float=True, want_radii=True)
    img_f, radii = img_f[0].cpu().numpy(), radii[0].cpu().numpy()
    _compare(img_f, img_u[0].cpu().numpy(), r64["image"], und, limit, what)
    dec = r64["decidable"] & r32["decidable"]
    assert np.array_equal(radii[dec], r64["radii"][dec]), what
    return img_f, radii, r64


def test_edges_of_the_definition(ops):
    red, green, blue, grey = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)
    bg = (0.25, 0.5, 1.0)
    # p.z <= 0.2 and behind the camera: culled, the image is the background bit for bit
    img, radii, _ = _hand_check(ops, _hand([[0, 0, 0.2], [0, 0, 0.1], [0, 0, -1.0]], 0.05, [0.9] * 3, [red] * 3), "near plane", bg)
    assert (radii == 0).all() and (img == np.array(bg + (0.0,), np.float32)).all()
    # two Gaussians at one position, o = 0.6: the smaller index is blended first
    for first, second in ((red, blue), (blue, red)):
        img, _, r64 = _hand_check(ops, _hand([[0, 0, 2.0]] * 2, 0.2, [0.6, 0.6], [first, second]), "equal depth")
        a = 0.6 * math.exp(-0.5 * 0.5 / (4.0 + 0.3))                     # pixel (16, 16): d = (-0.5, -0.5), var = (0.2 * 20 / 2)^2 + 0.3
        want = a * np.array(first) + a * (1 - a) * np.array(second)
        assert np.abs(img[16, 16, :3] - want).max() < 1e-5 and abs(img[16, 16, 3] - (1 - (1 - a) ** 2)) < 1e-5
        assert img[16, 16, 0 if first is red else 2] > img[16, 16, 2 if first is red else 0] + 0.2
    # three near-opaque Gaussians (50-pixel sigma: alpha in [0.97, 0.98] on the middle pixels) in a row and one behind: T <= 0.028, then
    # T in [4e-4, 7.8e-4], then T' <= 2.2e-5 < 1e-4 -- the third is not added, nor the fourth
    four = _hand([[0, 0, 2.0], [0, 0, 2.1], [0, 0, 2.2], [0, 0, 2.3]], 5.0, [0.98] * 4, [red, blue, green, green])
    img4, _, _ = _hand_check(ops, four, "saturation")
    img2, _, _ = _hand_check(ops, {k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in four.items()}, "saturation, first two")
    mid = (slice(12, 20), slice(12, 20))
    assert np.array_equal(img4[mid], img2[mid]) and (img4[mid][..., 1] < 1e-6).all() and (img4[mid][..., 3] > 0.999).all()
    # o < 1/255 adds nothing (it still has a radius)
    img, radii, _ = _hand_check(ops, _hand([[0, 0, 2.0]], 0.2, [0.0035], [red]), "faint", bg)
    assert radii[0] == 7 and (img == np.array(bg + (0.0,), np.float32)).all()
    # one Gaussian over every tile; one whose centre is off-frame but whose rectangle reaches in; one whose rectangle is empty
    img, radii, r64 = _hand_check(ops, _hand([[0, 0, 2.0]], 1.0, [0.9], [grey]), "every tile")
    assert tuple(r64["rect"][0]) == (0, 0, 2, 2) and (img[..., 3] > 0).all()
    img, radii, r64 = _hand_check(ops, _hand([[-2.1, 0, 2.0]], 0.3, [0.9], [grey]), "off-frame centre")
    # u = -5; cov00 = 0.09 (10^2 + 10.4^2) + 0.3 = 19.03 (p.x / p.z = -1.05 is clamped to -1.04): radius ceil(3 sqrt(19.03)) = 14
    assert radii[0] == 14 and tuple(r64["rect"][0]) == (0, 0, 1, 2) and img[16, 0, 3] > 0.3 and (img[:, 16:, 3] == 0).all()
    img, radii, _ = _hand_check(ops, _hand([[-12.0, 0, 2.0], [0, 30.0, 2.0]], 0.05, [0.9] * 2, [grey] * 2), "empty rectangle")
    assert (radii == 0).all() and (img[..., 3] == 0).all()
    # far off-axis: p.x / p.z = 1.6 against 1.3 tanx = 1.04, the clamp acts (without it the footprint would be larger along x)
    img, radii, r64 = _hand_check(ops, _hand([[3.2, 0.4, 2.0]], [[0.3, 0.3, 1.0]], [0.9], [grey]), "1.3 tan clamp")
    unclamped = math.ceil(3 * math.sqrt((20 * 0.3 / 2) ** 2 + (20 * 3.2 / 4 * 1.0) ** 2 + 0.3))
    assert 0 < radii[0] < unclamped and (img[..., 3] > 0).any()
    # n == 0: the background, alpha 0
    empty = {k: v[:0] for k, v in _hand([[0, 0, 2.0]], 0.2, [0.5], [red]).items() if isinstance(v, np.ndarray)}
    empty["sh_degree"] = 0
    img_f, img_u, count = _raster(ops, empty, np.repeat(ROW, 2, 0), 40, 24, channels=4, background=(0.0, 1.0, 0.5), want_float=True, want_instances=True)
    assert count == 0 and bool((img_u == torch.tensor([0, 255, 128, 0], dtype=torch.uint8, device="cuda")).all())
    assert bool((img_f == torch.tensor([0.0, 1.0, 0.5, 0.0], device="cuda")).all())


def test_determinism_batching_and_capacity(pkg, ops, syn):
    lib = importlib.import_module("6dgs_amd._lib").load()
    scene = syn.make_scene(3000, 9)
    cams = syn.make_cameras(5, 10, width=96, height=64)
    rows = RR.camera_rows(cams)
    kw = dict(channels=4, want_float=True, want_radii=True, want_instances=True)
    a_f, a_u, a_r, a_n = _raster(ops, scene, rows, 96, 64, **kw)
    b_f, b_u, b_r, b_n = _raster(ops, scene, rows, 96, 64, **kw)
    assert torch.equal(a_f, b_f) and torch.equal(a_u, b_u) and torch.equal(a_r, b_r) and a_n == b_n > 3000
    total = 0
    for v in range(5):
        s_f, s_u, s_r, s_n = _raster(ops, scene, rows[v:v + 1], 96, 64, **kw)
        assert torch.equal(s_f[0], a_f[v]) and torch.equal(s_u[0], a_u[v]) and torch.equal(s_r[0], a_r[v]), v
        total += s_n
    assert total == a_n
    # the retried call (capacity 1 -> the exact size) equals the roomy one, and so does the exact size given at once
    for cap in (1, a_n):
        c_f, c_u, c_r, c_n = _raster(ops, scene, rows, 96, 64, max_instances=cap, **kw)
        assert torch.equal(c_f, a_f) and torch.equal(c_u, a_u) and torch.equal(c_r, a_r) and c_n == a_n, cap
    # max_instances = 1, the C call itself: the needed count is reported, nothing is written outside the workspace or the outputs
    args = _dev(scene)
    need = ops.raster_views_workspace_bytes(3000, 5, 96, 64, 1)
    guard = 256
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((5 * 64 * 96 * 4 + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    camt, bg = torch.from_numpy(rows).cuda(), torch.ones(3, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    st = lib.sixdgs_raster_views(p(args[0]), p(args[1]), 1, p(args[2]), p(args[3]), 1, p(args[4]), p(args[5]), 3, 16, 3000, p(camt), 5, 96, 64, 1.0,
                                 p(bg), None, p(out, guard), 4, None, 1, p(cnt, 8), p(ws, guard), need, torch.cuda.current_stream().cuda_stream, None)
    torch.cuda.synchronize()
    assert st == 0 and cnt.tolist() == [-7, a_n, -7]
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[-guard:] == 0xA5).all()), "the workspace's guard bytes were written"
    assert bool((out[:guard] == 0x5A).all()) and bool((out[-guard:] == 0x5A).all()), "the image's guard bytes were written"
    # render_views(renderer="raster") does not depend on batch_size; rgba carries round(255 (1 - T)); the disc renderer is as before
    gs = pkg.GaussianScene.from_dict(scene, device="cuda")
    one = pkg.render_views(gs, cams, batch_size=1, renderer="raster")
    both = pkg.render_views(gs, [pkg.CameraInfo(**c) for c in cams], batch_size=5, renderer="raster")
    default = pkg.render_views(gs, cams, rgba=True, renderer="raster")
    white = _raster(ops, scene, rows, 96, 64, channels=4)
    for v in range(5):
        assert isinstance(one[v], pkg.CameraInfo) and one[v].image.dtype == np.uint8 and one[v].image.shape == (64, 96, 3)
        assert np.array_equal(one[v].image, white[v, ..., :3].cpu().numpy()) and np.array_equal(one[v].image, both[v].image)
        assert np.array_equal(default[v].image, white[v].cpu().numpy())
        assert np.array_equal(default[v].image[..., 3], a_u[v, ..., 3].cpu().numpy())
    assert not np.array_equal(one[0].image, one[1].image)
    disc = pkg.render_views(gs, cams)
    explicit = pkg.render_views(gs, cams, renderer="disc")
    splat = ops.splat_views(*[args[i] for i in (0, 1, 4, 5, 6)], camt, 96, 64)
    for v in range(5):
        assert np.array_equal(disc[v].image, splat[v].cpu().numpy()) and np.array_equal(disc[v].image, explicit[v].image)


@pytest.mark.timeout(300)
def test_full_size_samples(ops, syn):
    """500 k Gaussians, 800 x 800, one view: 2048 sampled pixels (32 in each of 64 sampled tiles) against the restatement evaluated on
    those tiles in fp64 and fp32, under the bound rule of the cases."""
    n, side = 500_000, 800
    scene = syn.make_scene(n, 0)
    rows = RR.camera_rows(syn.make_cameras(1, 21, width=side, height=side))
    rng = np.random.default_rng(5)
    tiles = np.sort(rng.choice((side // RR.TILE) ** 2, 64, replace=False))
    inner = np.stack([rng.choice(RR.TILE * RR.TILE, 32, replace=False) for _ in tiles])
    ys = ((tiles // (side // RR.TILE))[:, None] * RR.TILE + inner // RR.TILE).reshape(-1)
    xs = ((tiles % (side // RR.TILE))[:, None] * RR.TILE + inner % RR.TILE).reshape(-1)
    r64 = RR.reference_view(scene, rows[0], side, side, np.float64, background=RR.BACKGROUND, tiles=tiles)
    r32 = RR.reference_view(scene, rows[0], side, side, np.float32, background=RR.BACKGROUND, tiles=tiles)
    assert r64["blended"][ys, xs].all()
    und = (r64["undecidable"] | r32["undecidable"])[ys, xs]
    assert und.mean() <= RR.MAX_UNDECIDABLE_SHARE_FULL, und.mean()
    ref = r64["image"][ys, xs]
    rounding = np.abs(r32["image"][ys, xs].astype(np.float64) - ref)[~und].max()
    limit = RR.bound(float(rounding))
    assert limit <= RR.ERROR_CEILING, rounding
    args, cams = _dev(scene), torch.from_numpy(rows).cuda()
    kw = dict(channels=4, background=RR.BACKGROUND, want_float=True, want_instances=True)
    _, _, count = ops.raster_views(*args, cams, side, side, **kw)           # warm-up (and the capacity the scene needs)
    torch.cuda.synchronize()
    t0 = time.time()
    img_f, img_u, count = ops.raster_views(*args, cams, side, side, max_instances=count, **kw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert r64["instances_lo"] <= count <= r64["instances_hi"]
    print(f"500 k Gaussians at 800 x 800: {count} instances, {1e3 * dt:.1f} ms wall; fp32 rounding of the restatement {rounding:.3e}; "
          f"mean alpha of the samples {ref[:, 3].mean():.3f}")
    _compare(img_f[0].cpu().numpy()[ys, xs], img_u[0].cpu().numpy()[ys, xs], ref, und, limit, "full size")
    assert dt < 10.0, f"{dt:.2f} s for one view"
