"""CPU tests of the depth feature: the numpy restatement (tests/depth_reference.py) held to account -- its two precisions agree, hand
cases give what their formulas dictate, every case of the GPU tests qualifies and one of them reaches the second LDS round --, the
declaration of the entry points and their argument handling, which is answered without a GPU."""
import importlib
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrib_reference as CR  # noqa: E402
import depth_reference as DR  # noqa: E402
import raster_reference as RR  # noqa: E402

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_raster_depth_workspace_bytes", "sixdgs_raster_depth", "sixdgs_scene_depth_workspace_bytes", "sixdgs_scene_depth")


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", DR.CASES)
def test_the_restatements_agree_and_the_case_qualifies(syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """Every case of the GPU tests: the union of undecidable pixels stays under raster_reference's share; outside it fp32 and fp64 name
    the same median Gaussian; the fp32 form's own deviation from fp64 is inside the ceiling that caps the GPU's tolerance, and 4 x it
    too for the points at the median; and the restatement's alpha is raster_reference's image alpha (the same products in the same
    order: equal in both precisions)."""
    c = DR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    r64, r32, und = c["r64"], c["r32"], c["undecidable"]
    band = r64["median_undecidable"] | r32["median_undecidable"]
    has = r64["median_index"] >= 0
    print(f"n={n} {width}x{height}x{views} deg={sh_degree}: undecidable {und.sum()} of {und.size} ({und.mean():.2e}), in the median band "
          f"{band.sum()}, pixels with a median {has.mean():.2f}, fp32 deviates " + ", ".join(f"{k} {v:.2e}" for k, v in c["deviations"].items())
          + f", bound {DR.bound(c['rounding']):.2e}")
    assert und.mean() <= RR.MAX_UNDECIDABLE_SHARE, "not a fit case: pick other seeds"
    assert np.array_equal(r64["median_index"][~und], r32["median_index"][~und])
    # the GPU is held to min(4 x this deviation, the ceiling) (depth_reference.tolerance): fp32 done in this order must itself fit
    assert c["rounding"] <= RR.ERROR_CEILING and all(DR.tolerance(c, k) <= RR.ERROR_CEILING for k in DR.MEASURED), "not a fit case"
    assert DR.bound(c["deviations"]["points_median"]) <= RR.ERROR_CEILING
    assert 0.1 < has.mean() < 0.9 and (r64["median_index"][has] < n).all() and (r64["median"][~has] == 0).all()
    image = CR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    assert np.abs(r64["alpha"] - image["r64"]["image_alpha"]).max() <= 1e-12 and np.array_equal(r32["alpha"], image["r32"]["image_alpha"])
    for r in (r64, r32):
        # the median is the depth of its Gaussian; it exists only where alpha passed one half; D is a convex sum of depths times alpha
        v, y, x = np.nonzero(r["median_index"] >= 0)
        assert np.array_equal(r["median"][v, y, x], r["z"][v, r["median_index"][v, y, x]]) and (r["alpha"][v, y, x] > 0.5 - 1e-6).all()
        assert (r["expected"] <= r["z"].max() * r["alpha"] * (1 + 1e-5)).all() and (r["expected"] >= RR.NEAR_Z * r["alpha"] * (1 - 1e-5)).all()
        assert not r["points_median"][r["median_index"] < 0].any() and not r["points_expected"][r["alpha"] == 0].any()


def test_one_case_has_a_median_in_the_second_round(syn):
    """The kernel stages a tile's list through LDS 256 entries at a time: a median at position >= 256 is found in a later round."""
    c = DR.case(syn, *DR.ROUNDS)
    pos = c["r64"]["median_pos"]
    print(f"{(pos >= 256).sum()} of {pos.size} pixels have their median at a list position >= 256 (largest {pos.max()})")
    assert (pos[~c["undecidable"]] >= 256).any()


def _one(scene, row=CR.ROW, width=32, height=32):
    und = CR.pair(scene, row, width, height)["undecidable"]
    c = DR.pair(scene, row, width, height, und)
    assert not c["undecidable"].any(), "the hand case has an undecidable pixel"
    assert np.array_equal(c["r64"]["median_index"], c["r32"]["median_index"])
    return c["r64"]


def test_hand_cases_give_the_stated_depths():
    z0, f = 2.0, 20.0
    var = (0.2 * f / z0) ** 2 + 0.3                    # sigma f / z squared, + 0.3
    centre = math.exp(-0.5 * (0.5 ** 2 + 0.5 ** 2) / var)          # the Gaussian's centre is the corner of pixel (16, 16): d = (-0.5, -0.5)
    # one Gaussian facing the camera, opacity 0.9: T' = 1 - alpha < 0.5 at the centre pixel
    r = _one(CR.hand([[0, 0, z0]], 0.2, [0.9]))
    alpha = 0.9 * centre
    assert abs(r["alpha"][0, 16, 16] - alpha) < 1e-6 and abs(r["expected"][0, 16, 16] - z0 * alpha) < 1e-6
    assert r["median"][0, 16, 16] == z0 and r["median_index"][0, 16, 16] == 0
    want = np.array([0.5 / f * z0, 0.5 / f * z0, z0])               # identity pose: X = d r
    assert np.abs(r["points_median"][0, 16, 16] - want).max() < 1e-12 and np.abs(r["points_expected"][0, 16, 16] - want).max() < 1e-6
    far = r["median_index"][0] < 0
    assert far[0, 0] and not r["points_median"][0][far].any() and (r["alpha"][0][far] <= 0.5 + 1e-9).all()
    # the same at opacity 0.4: T never falls below 0.5
    r = _one(CR.hand([[0, 0, z0]], 0.2, [0.4]))
    assert abs(r["alpha"][0, 16, 16] - 0.4 * centre) < 1e-6 and abs(r["expected"][0, 16, 16] - z0 * 0.4 * centre) < 1e-6
    assert not r["median"].any() and (r["median_index"] == -1).all() and not r["points_median"].any() and r["points_expected"][0, 16, 16, 2] > 0
    # two wide Gaussians at z = 1 and 2, both at 0.4: T goes to 0.6, then 0.36 -- the median is the second
    r = _one(CR.hand([[0, 0, 1.0], [0, 0, 2.0]], 5.0, [0.4, 0.4]))
    assert (r["median_index"] == 1).all() and (r["median"] == 2.0).all()
    a1, a2 = (0.4 * math.exp(-0.25 / ((5.0 * f / z) ** 2 + 0.3)) for z in (1.0, 2.0))          # at the centre pixel: nearly flat
    assert abs(r["alpha"][0, 16, 16] - (1 - (1 - a1) * (1 - a2))) < 1e-6 and abs(r["expected"][0, 16, 16] - (1.0 * a1 + 2.0 * a2 * (1 - a1))) < 1e-6
    assert abs(a1 - 0.4) < 1e-4 and abs((1 - a1) * (1 - a2) - 0.36) < 1e-4
    # equal depth bits: the lower index comes first, whichever of the two is the more opaque
    for o, alpha_first in (([0.6, 0.9], 0.6), ([0.9, 0.6], 0.9)):
        r = _one(CR.hand([[0, 0, z0], [0, 0, z0]], 5.0, o))
        assert (r["median_index"] == 0).all() and (r["median"] == z0).all()
        assert abs(r["alpha"][0, 16, 16] - (1 - (1 - o[0]) * (1 - o[1]))) < 1e-3 and alpha_first > 0.5
    r = _one(CR.hand([[0, 0, z0], [0, 0, z0]], 5.0, [0.3, 0.9]))
    assert (r["median_index"] == 1).all()
    # nothing in view: the empty values everywhere
    r = _one(CR.hand_nothing())
    assert not r["expected"].any() and not r["median"].any() and (r["median_index"] == -1).all() and not r["alpha"].any()
    assert not r["points_median"].any() and not r["points_expected"].any()


def test_lift_projects_back_to_the_pixel_centre(syn):
    rows = RR.camera_rows(syn.make_cameras(2, 5, width=33, height=17))
    ys, xs = np.mgrid[0:17, 0:33]
    d = np.random.default_rng(0).uniform(0.5, 6.0, (17, 33))
    for row in rows:
        X = DR.lift(row, xs, ys, d, np.ones((17, 33), bool), np.float64)
        m = row.astype(np.float64)
        p = X @ m[:12].reshape(3, 4)[:, :3].T + m[:12].reshape(3, 4)[:, 3]
        assert np.abs(p[..., 2] - d).max() < 1e-5          # (the rotation of a camera row is orthonormal to fp32)
        assert np.abs(m[12] * p[..., 0] / p[..., 2] + m[14] - (xs + 0.5)).max() < 1e-4
        assert np.abs(m[13] * p[..., 1] / p[..., 2] + m[15] - (ys + 0.5)).max() < 1e-4
    assert not DR.lift(rows[0], xs, ys, d, np.zeros((17, 33), bool), np.float32).any()


def test_entry_points_are_declared_and_bound():
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    pkg = importlib.import_module("6dgs_amd")
    render = importlib.import_module("6dgs_amd.render")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(lib.load(), name), f"{name} is not exported"
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES] == [5, 18, 5, 32]
    assert lib.ABI_VERSION == 10 and "depth.hip" in build.SOURCES
    assert pkg.render_depth is render.render_depth and pkg.surface_points is render.surface_points
    assert {"render_depth", "surface_points"} <= set(pkg.__all__)


def test_workspace_sizes_and_argument_errors_need_no_gpu():
    ops = importlib.import_module("6dgs_amd.ops")
    lib = importlib.import_module("6dgs_amd._lib").load()
    assert ops.raster_depth_workspace_bytes(1000, 2, 40, 24, 1) == 256 == ops.raster_depth_workspace_bytes(0, 0, 40, 24, 1 << 20)
    for bad in ((-1, 2, 40, 24, 10), (1 << 31, 2, 40, 24, 10), (10, 65536, 40, 24, 10), (10, 2, 0, 24, 10), (10, 2, 40, 16385, 10), (10, 2, 40, 24, 0),
                (10, 2, 40, 24, 1 << 31)):
        assert ops.raster_depth_workspace_bytes(*bad) == 0 and ops.scene_depth_workspace_bytes(*bad) == 0, bad
    fwd = ops.raster_views_workspace_bytes(1000, 3, 40, 24, 5000)
    assert ops.scene_depth_workspace_bytes(1000, 3, 40, 24, 5000) == fwd + 256 + 256 and ops.scene_depth_workspace_bytes(1000, 0, 40, 24, 5000) == 0
    # the raw call: every refusal comes back before anything is launched (this process has no GPU to launch on); the pointers are
    # never followed, so aligned made-up addresses stand in for device memory
    A, W = 1 << 20, 2 << 20
    fwd1 = ops.raster_views_workspace_bytes(10, 2, 40, 24, 100)
    call = lambda n=10, views=2, w=40, h=24, cap=100, f=A, fb=fwd1, cams=None, outs=(None,) * 5, kind=0, ws=W, wb=256: lib.sixdgs_raster_depth(  # noqa: E731
        n, views, w, h, cap, f, fb, cams, *outs, kind, ws, wb, None, None)
    assert call(n=-1) == -1 and call(views=65536) == -1 and call(w=0) == -1 and call(h=16385) == -1 and call(cap=0) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1
    assert call(f=None) == -1 and call(fb=fwd1 - 1) == -2 and call(wb=255) == -2 and call(ws=None) == -1 and call(ws=W + 8) == -1 and call(f=A + 8) == -1
    assert call(outs=(None,) * 4 + (A,)) == -1 and call(outs=(None,) * 4 + (A,), f=None, cams=A) == -1          # points without cams; no fwd_ws
    for k in range(5):
        assert call(outs=(None,) * k + (A + 2,) + (None,) * (4 - k), cams=A) == -1, k
    assert call(cams=A + 2) == -1
    assert call(views=0, f=None) == 0 and call() == 0 and call(cams=A) == 0          # nothing to do; every output NULL
    scene = (A, A, 1, A, A, 1, A, None, 0, 1, 10)
    need = ops.scene_depth_workspace_bytes(10, 2, 40, 24, 100)
    drive = lambda views=2, chunk=2, cap=100, cams=A, bg=A, outs=(A,) * 5, kind=0, image=None, ch=3, status=A, needed=A, ws=W, wb=need, sm=1.0, args=scene: \
        lib.sixdgs_scene_depth(*args, cams, views, 40, 24, sm, bg, chunk, cap, *outs, kind, image, ch, status, needed, ws, wb, None)      # noqa: E731
    assert drive(chunk=0) == -1 and drive(cap=0) == -1 and drive(views=-1) == -1 and drive(sm=0.0) == -1 and drive(cams=None) == -1
    assert drive(kind=2) == -1 and drive(ch=5) == -1 and drive(image=A, bg=None) == -1 and drive(image=A + 2, ch=4) == -1
    assert drive(status=None) == -1 and drive(needed=None) == -1 and drive(needed=A + 4) == -1 and drive(wb=need - 1) == -2 and drive(ws=None) == -1
    assert drive(outs=(A + 1,) + (None,) * 4) == -1 and drive(outs=(None,) * 4 + (A + 2,)) == -1
    assert drive(args=(None,) + scene[1:]) == -1 and drive(args=scene[:8] + (1, 1, 10)) == -1
    assert drive(views=0, cams=None, status=None) == 0
    # the Python surface refuses in the style of its neighbours, before it looks for a device
    state = (torch.empty(8, dtype=torch.uint8), 10)
    for bad in (dict(want=("depth",)), dict(want=()), dict(points="mean"), dict(points="median"), dict(points="median", cams=torch.zeros(3, 16))):
        with pytest.raises(ValueError):
            ops.raster_depth(state, 10, 2, 40, 24, **bad)
    for bad_state in ((state[0], 0), (None, 10), state[0]):
        with pytest.raises(ValueError):
            ops.raster_depth(bad_state, 10, 2, 40, 24)
    with pytest.raises(ValueError):
        ops.raster_depth(state, 10, 2, 0, 24)
    with pytest.raises(RuntimeError):
        ops.raster_depth(state, 10, 2, 40, 24)          # a state on the CPU: no fallback


def test_render_depth_refuses_cpu_scenes_and_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(20, 1), device="cpu")
    cams = syn.make_cameras(2, 3, width=40, height=24)
    for bad in (dict(kind="mean"), dict(chunk=0), dict(chunk=1.5), dict(scale_modifier=0.0)):
        with pytest.raises(ValueError):
            pkg.render_depth(scene, cams, **bad)
    for bad in (dict(min_alpha=1.5), dict(stride=0), dict(kind="mode"), dict(background=(1.0, 1.0))):
        with pytest.raises(ValueError):
            pkg.surface_points(scene, cams, **bad)
    with pytest.raises(RuntimeError):
        pkg.render_depth(scene, cams)
    with pytest.raises(RuntimeError):
        pkg.surface_points(scene, cams)
