"""sixdgs_splat_views on the GPU against the fp64 restatement of its definition (tests/splat_reference.py): winners pixel by pixel,
colours against this build's own SH evaluation, the edges of the definition, determinism and batching, and the full size."""
import importlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def _dev(scene):
    return [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("xyz", "log_scale", "f_dc", "f_rest")] + [int(scene["sh_degree"])]


def _splat(ops, scene, rows, width, height, **kw):
    return ops.splat_views(*_dev(scene), torch.from_numpy(np.ascontiguousarray(rows)).cuda(), width, height, **kw)


def _expected_colours(ops, scene, row):
    """uint8 [n,3]: round(255 min(c, 1)), c = ops.eval_sh_color for the ray that leaves each Gaussian towards the camera."""
    sh = torch.cat([torch.from_numpy(scene["f_dc"]), torch.from_numpy(scene["f_rest"])], dim=1).transpose(1, 2).contiguous().cuda()
    dirs = torch.from_numpy(SR.ray_dirs_to_camera(scene["xyz"], row).astype(np.float32)).cuda()
    c = ops.eval_sh_color(sh, dirs, int(scene["sh_degree"])).cpu().numpy().astype(np.float64)
    return np.round(255.0 * np.minimum(c, 1.0))


def _check_colours(ops, scene, rows, image, winner, background):
    image, winner = image.cpu().numpy(), winner.cpu().numpy()
    bg = np.round(255.0 * np.asarray(background, np.float64))
    worst = 0
    for v, row in enumerate(rows):
        hit = winner[v] >= 0
        want = _expected_colours(ops, scene, row)[winner[v][hit]]
        worst = max(worst, int(np.abs(image[v][hit][:, :3].astype(np.int64) - want).max()) if hit.any() else 0)
        assert (image[v][~hit][:, :3] == bg).all(), "background pixels do not carry the background"
        if image.shape[-1] == 4:
            assert (image[v][hit][:, 3] == 255).all() and (image[v][~hit][:, 3] == 0).all(), "alpha is not the silhouette"
    assert worst <= 1, f"a colour differs from round(255 min(c, 1)) by {worst}"
    return worst


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height", SR.WINNER_CASES)
def test_winners_and_colours_against_the_restatement(ops, syn, n, scene_seed, views, cam_seed, width, height):
    """The winner buffer equals the restatement's on every decidable pixel (and at most 0.1 % are not); every covered pixel has its
    winner's colour within one step of the last place, every other pixel the background; RGBA: alpha = the silhouette."""
    scene = syn.make_scene(n, scene_seed)
    rows = SR.camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height))
    ref, und = SR.reference_views(scene, rows, width, height, extent=1.0, near_z=0.05)
    share = und.mean()
    assert share <= SR.MAX_UNDECIDABLE_SHARE, share
    bg = (0.25, 0.5, 1.0)
    image, winner = _splat(ops, scene, rows, width, height, extent=1.0, near_z=0.05, background=bg, want_winner=True)
    assert image.shape == (views, height, width, 3) and image.dtype == torch.uint8 and winner.dtype == torch.int32
    got = winner.cpu().numpy()
    differ = (got != ref) & ~und
    print(f"n={n} {width}x{height} views={views}: covered {(ref >= 0).mean():.3f}, undecidable {share:.5f}, "
          f"differing decidable pixels {int(differ.sum())}, differing undecidable pixels {int(((got != ref) & und).sum())}")
    assert not differ.any(), f"{int(differ.sum())} decidable pixels have another winner, first at {np.argwhere(differ)[0]}"
    worst = _check_colours(ops, scene, rows, image, winner, bg)
    image4, winner4 = _splat(ops, scene, rows, width, height, channels=4, background=bg, want_winner=True)
    assert torch.equal(winner4, winner) and torch.equal(image4[..., :3], image)
    _check_colours(ops, scene, rows, image4, winner4, bg)
    print(f"  largest colour difference {worst}")


def test_edges_of_the_definition(ops):
    """Behind the camera / nearer than near_z never wins; a disc cut by the frame; a disc entirely outside; two Gaussians at one
    position (same depth bits -> the smaller index); the radius floor."""
    row = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 10.0, 10.0, 8.0, 8.0]], np.float32)       # identity pose, f = 10, 16 x 16
    xyz = np.array([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [0.5, 0.5, 0.01], [0, 0, -1.0], [-0.75, -0.75, 1.0], [30.0, 0, 1.0],
                    [0.9, 0.0, 1.5]], np.float32)
    s = np.log(np.array([[0.8] * 3, [0.2] * 3, [0.2] * 3, [0.5] * 3, [0.5] * 3, [1e-4] * 3, [0.3] * 3, [0.3, 0.1, 0.45]], np.float32))
    rng = np.random.default_rng(1)
    scene = {"xyz": xyz, "log_scale": s, "f_dc": (0.3 * rng.standard_normal((8, 1, 3))).astype(np.float32),
             "f_rest": (0.05 * rng.standard_normal((8, 15, 3))).astype(np.float32), "sh_degree": 3}
    ref, und = SR.reference_view(xyz, s, row[0], 16, 16)
    image, winner = _splat(ops, scene, row, 16, 16, want_winner=True)
    got = winner[0].cpu().numpy()
    assert got[8, 8] == 1, "two Gaussians at one position: the smaller index must win"
    assert not np.isin(got, (2, 3, 4, 6)).any()
    assert got[0, 0] == 5 and got[0, 1] == -1 and got[1, 0] == -1            # the floor of the radius: exactly the centre's pixel
    assert (got[:, 15] == 7).any() and ref[8, 15] == 7                         # Gaussian 7 (u = 14, r = 3) is cut by the right frame edge
    assert ((got == ref) | und).all()
    _check_colours(ops, scene, row, image, winner, (1.0, 1.0, 1.0))
    # the same scene seen from in front of every Gaussian's back: nothing visible
    back = row.copy()
    back[0, 11] = -40.0
    image, winner = _splat(ops, scene, back, 16, 16, want_winner=True)
    assert bool((winner == -1).all()) and bool((image == 255).all())


def test_no_gaussians_and_sh_degrees(ops, syn):
    rows = SR.camera_rows(syn.make_cameras(2, 3, width=40, height=24))
    empty = syn.make_scene(0, 0)
    image, winner = _splat(ops, empty, rows, 40, 24, background=(0.0, 1.0, 0.5), want_winner=True, channels=4)
    assert bool((winner == -1).all())
    assert bool((image == torch.tensor([0, 255, 128, 0], dtype=torch.uint8, device="cuda")).all())
    for deg in (0, 3):
        scene = syn.make_scene(300, 2, sh_degree=deg)
        assert scene["f_rest"].shape[1] == (deg + 1) ** 2 - 1
        ref, und = SR.reference_views(scene, rows, 40, 24)
        image, winner = _splat(ops, scene, rows, 40, 24, want_winner=True)
        assert (((winner.cpu().numpy() == ref) | und)).all() and (ref >= 0).any()
        _check_colours(ops, scene, rows, image, winner, (1.0, 1.0, 1.0))


def test_determinism_and_batching(pkg, ops, syn):
    """Two calls give the same bytes; B views in one call equal the B single-view calls; render_views does not depend on its batch size."""
    scene = syn.make_scene(3000, 9)
    cams = syn.make_cameras(5, 10, width=96, height=64)
    rows = SR.camera_rows(cams)
    a_img, a_win = _splat(ops, scene, rows, 96, 64, want_winner=True)
    b_img, b_win = _splat(ops, scene, rows, 96, 64, want_winner=True)
    assert torch.equal(a_img, b_img) and torch.equal(a_win, b_win)
    for v in range(5):
        s_img, s_win = _splat(ops, scene, rows[v:v + 1], 96, 64, want_winner=True)
        assert torch.equal(s_img[0], a_img[v]) and torch.equal(s_win[0], a_win[v]), v
    gs = pkg.GaussianScene.from_dict(scene, device="cuda")
    one = pkg.render_views(gs, cams, batch_size=1)
    both = pkg.render_views(gs, [pkg.CameraInfo(**c) for c in cams], batch_size=5)
    default = pkg.render_views(gs, cams, rgba=True)
    for v in range(5):
        assert isinstance(one[v], pkg.CameraInfo) and one[v].image.dtype == np.uint8 and one[v].image.shape == (64, 96, 3)
        assert np.array_equal(one[v].image, a_img[v].cpu().numpy()) and np.array_equal(one[v].image, both[v].image)
        assert default[v].image.shape == (64, 96, 4) and np.array_equal(default[v].image[..., :3], one[v].image)
        assert np.array_equal(one[v].R, cams[v]["R"]) and one[v].width == 96 and one[v].image_name == cams[v]["image_name"]
    # two views of the same scene are different images (what the random-byte views could not give: content that follows the camera)
    assert not np.array_equal(one[0].image, one[1].image)


@pytest.mark.timeout(300)
def test_full_size_invariants(ops, syn):
    """500 k Gaussians, 800 x 800, 2 views.  On 4096 sampled pixels per view: the winner's disc contains the pixel in fp64 within the
    edge tolerance scaled to this image size (1e-4 at 160 px -> 5e-4 at 800 px), and no Gaussian that clearly covers the pixel
    (d^2 < 0.99 r^2) is clearly nearer (by more than 1e-6 relative); a pixel without a winner is clearly covered by nothing."""
    n, width, height, views, samples = 500_000, 800, 800, 2, 4096
    edge_tol = SR.EDGE_TOL * width / 160
    scene = syn.make_scene(n, 0)
    rows = SR.camera_rows(syn.make_cameras(views, 21, width=width, height=height))
    args = _dev(scene)
    cams = torch.from_numpy(rows).cuda()
    ops.splat_views(*args, cams, width, height)           # warm-up
    torch.cuda.synchronize()
    t0 = time.time()
    image, winner = ops.splat_views(*args, cams, width, height, want_winner=True)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert dt < 5.0, f"{dt:.2f} s for two views"
    win = winner.cpu().numpy()
    rng = np.random.default_rng(5)
    for v in range(views):
        z, vis, u, vv, r = (torch.from_numpy(a).cuda() for a in SR.project(scene["xyz"], scene["log_scale"], rows[v], 1.0, 0.05))
        pix = rng.choice(width * height, samples, replace=False)
        px = torch.from_numpy((pix % width) + 0.5).cuda()
        py = torch.from_numpy((pix // width) + 0.5).cuda()
        w = torch.from_numpy(win[v].reshape(-1)[pix].astype(np.int64)).cuda()
        has = w >= 0
        ws = w.clamp(min=0)
        d2w = (px - u[ws]) ** 2 + (py - vv[ws]) ** 2
        inside = d2w <= (r[ws] ** 2) * (1 + edge_tol)
        assert bool((inside & vis[ws])[has].all()), f"view {v}: a winner's disc does not contain its pixel"
        zw = torch.where(has, z[ws], torch.full_like(z[ws], float("inf")))
        nearest_clear = torch.full_like(zw, float("inf"))
        for g0 in range(0, n, 32768):
            g = slice(g0, min(g0 + 32768, n))
            d2 = (px[:, None] - u[None, g]) ** 2 + (py[:, None] - vv[None, g]) ** 2
            clear = (d2 < 0.99 * (r[None, g] ** 2)) & vis[None, g]
            zg = torch.where(clear, z[None, g], torch.full_like(d2, float("inf")))
            nearest_clear = torch.minimum(nearest_clear, zg.min(dim=1).values)
        bad = nearest_clear < zw * (1 - SR.DEPTH_TIE)
        assert not bool(bad.any()), f"view {v}: {int(bad.sum())} sampled pixels have a clearly nearer, clearly covering Gaussian"
        print(f"view {v}: {int(has.sum())} of {samples} sampled pixels covered; coverage of the view {(win[v] >= 0).mean():.3f}")
    print(f"two views of 500 k Gaussians at 800 x 800 (with the winner buffer): {1e3 * dt:.1f} ms wall")
