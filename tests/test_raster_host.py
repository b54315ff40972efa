"""The 3DGS forward rasteriser (sixdgs_raster_views) without a GPU: the entry points in the header, the binding and the library; the
answers that need no device; the refusals of ops.raster_views and render_views(renderer="raster"); and the numpy restatement of the
image definition (tests/raster_reference.py) on the properties the GPU test relies on -- few undecidable pixels, radii and
rectangles that do not depend on fp32 rounding, and a small fp32-against-fp64 difference."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_raster_views", "sixdgs_raster_views_workspace_bytes")


def _call(L, **kw):
    """sixdgs_raster_views with NULL pointers everywhere; kw overrides the scalar arguments."""
    a = dict(scale_is_log=1, opacity_is_logit=1, sh_degree=3, n_coef=16, n=0, views=1, width=8, height=8, scale_modifier=1.0, channels=3,
             max_instances=16, ws_bytes=0)
    a.update(kw)
    nul = None
    return L.sixdgs_raster_views(nul, nul, a["scale_is_log"], nul, nul, a["opacity_is_logit"], nul, nul, a["sh_degree"], a["n_coef"], a["n"],
                                 nul, a["views"], a["width"], a["height"], a["scale_modifier"], nul, nul, nul, a["channels"], nul,
                                 a["max_instances"], nul, nul, a["ws_bytes"], nul, None)


def test_raster_entry_points_in_header_binding_and_library():
    ge = importlib.import_module("__graft_entry__")
    lib = importlib.import_module("6dgs_amd._lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert ge.header_abi_version() == 10 == lib.ABI_VERSION
    assert len(lib.SIGNATURES["sixdgs_raster_views"][1]) == 27 and len(lib.SIGNATURES["sixdgs_raster_views_workspace_bytes"][1]) == 5
    assert "raster.hip" in importlib.import_module("6dgs_amd.build").SOURCES
    if os.path.exists(lib.LIB_PATH):
        so = C.CDLL(lib.LIB_PATH)
        for name in NAMES:
            assert hasattr(so, name), f"{name} is not exported by the library"
        L = lib.load()
        assert L.sixdgs_abi_version() == 10
        # sizes and argument errors are answered without touching the GPU
        ws = L.sixdgs_raster_views_workspace_bytes
        assert ws(1000, 2, 64, 48, 5000) >= 2 * 1000 * 64 + 2 * 5000 * 12 + 16 * 5000
        assert ws(1000, 4, 64, 48, 5000) > ws(1000, 2, 64, 48, 5000) > ws(1000, 2, 64, 48, 50) and ws(0, 1, 8, 8, 1) > 0
        assert ws(1000, 2, 64, 48, 0) == 0 and ws(-1, 2, 64, 48, 10) == 0 and ws(10, 2, 0, 48, 10) == 0 and ws(10, 2, 64, 48, 1 << 31) == 0
        assert ws(10, 65535, 16384, 16384, 10) == 0                         # views gx gy >= 2^31
        for bad in (dict(channels=5), dict(width=0), dict(height=20000), dict(n_coef=9), dict(sh_degree=4), dict(scale_modifier=0.0),
                    dict(scale_modifier=float("inf")), dict(max_instances=0), dict(max_instances=1 << 31), dict(n=-1), dict(views=-1),
                    dict(views=65535, width=16384, height=16384), dict()):   # the last: NULL cams / background
            assert _call(L, **bad) == -1, bad
        assert _call(L, views=0) == 0                                       # no views: nothing to do


def _scene_tensors(syn, n=10):
    sc = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_scene(n, 0).items()}
    return (sc["xyz"], sc["log_scale"], sc["rot"], sc["opacity"], sc["f_dc"], sc["f_rest"], 3)


def test_raster_views_refuses_cpu_tensors_and_bad_arguments(syn):
    ops = importlib.import_module("6dgs_amd.ops")
    args = _scene_tensors(syn)
    cams = torch.from_numpy(RR.camera_rows(syn.make_cameras(2, 0, width=16, height=16)))
    with pytest.raises(RuntimeError):
        ops.raster_views(*args, cams, 16, 16)
    for kw in (dict(channels=2), dict(channels=5), dict(scale_modifier=0.0), dict(scale_modifier=-1.0), dict(scale_modifier=float("nan")),
               dict(background=(1.0, 1.0)), dict(max_instances=0), dict(max_instances=1 << 31), dict(want_u8=False)):
        with pytest.raises(ValueError):
            ops.raster_views(*args, cams, 16, 16, **kw)
    for bad in (cams[:, :12], cams.reshape(-1), cams[None]):
        with pytest.raises(ValueError):
            ops.raster_views(*args, bad, 16, 16)
    with pytest.raises(ValueError):
        ops.raster_views(*args, cams, 0, 16)
    for k in (1, 2, 3):                                                     # scale, rot, opacity of another length
        short = list(args)
        short[k] = short[k][:5]
        with pytest.raises(ValueError):
            ops.raster_views(*short, cams, 16, 16)
    if os.path.exists(importlib.import_module("6dgs_amd._lib").LIB_PATH):
        assert ops.raster_views_workspace_bytes(1000, 2, 64, 48, 5000) > ops.raster_views_workspace_bytes(1000, 1, 64, 48, 5000) > 0
    assert ops.raster_instances_estimate(0, 1) >= 1 and ops.raster_instances_estimate(1 << 30, 64) < 1 << 31


def test_render_views_raster_refuses_cpu_scenes_and_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    cams = syn.make_cameras(2, 0, width=16, height=16)
    with pytest.raises(RuntimeError):
        pkg.render_views(scene, cams, renderer="raster")
    with pytest.raises(RuntimeError):
        pkg.render_views(scene, [pkg.CameraInfo(**c) for c in cams], rgba=True, renderer="raster")
    for kw in (dict(renderer="bogus"), dict(renderer=None), dict(renderer="raster", batch_size=0), dict(renderer="raster", scale_modifier=0.0)):
        with pytest.raises(ValueError):
            pkg.render_views(scene, cams, **kw)
    with pytest.raises(ValueError):
        pkg.render_views(scene, [dict(cams[0], R=np.eye(4))], renderer="raster")
    assert "--renderer" in open(os.path.join(ROOT, "tools", "train_standin.py")).read()


def test_restatement_on_a_hand_made_scene():
    """Values that can be worked out by hand: one isotropic Gaussian in front of an identity camera."""
    row = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 16.0, 16.0], np.float32)       # identity pose, f = 20, 32 x 32
    scene = {"xyz": np.array([[0.0, 0.0, 2.0]], np.float32), "log_scale": np.log(np.full((1, 3), 0.2, np.float32)),
             "rot": np.array([[1.0, 0, 0, 0]], np.float32), "opacity": np.array([[0.0]], np.float32),
             "f_dc": np.zeros((1, 1, 3), np.float32), "f_rest": np.zeros((1, 15, 3), np.float32), "sh_degree": 3}
    r = RR.reference_view(scene, row, 32, 32, np.float64, background=(0.0, 0.0, 0.0))
    var = (0.2 * 20.0 / 2.0) ** 2 + 0.3                                   # (sigma f / z)^2 + the 0.3 of step 3
    assert r["radii"][0] == int(np.ceil(3 * np.sqrt(var))) == 7
    assert tuple(r["rect"][0]) == (0, 0, 2, 2) and r["instances"] == 4 and r["decidable"][0]
    img = r["image"]
    a = lambda d2: 0.5 * np.exp(-0.5 * d2 / var)                          # noqa: E731  (sigmoid(0) = 0.5)
    for (y, x) in ((16, 16), (15, 16), (10, 20), (3, 3)):
        d2 = (16 - x - 0.5) ** 2 + (16 - y - 0.5) ** 2
        want = a(d2) if a(d2) >= 1 / 255 else 0.0
        # colour = 0 + 0.5; 1e-7: log(0.2) reaches the restatement rounded to fp32, which moves var by 1e-7 relative
        assert abs(img[y, x, 3] - want) < 1e-7 and abs(img[y, x, 0] - 0.5 * want) < 1e-7, (y, x)
    assert img[0, 0, 3] == 0.0 and not r["undecidable"].all()
    r32 = RR.reference_view(scene, row, 32, 32, np.float32, background=(0.0, 0.0, 0.0))
    assert r32["image"].dtype == np.float32 and np.abs(r32["image"] - img).max() < 1e-6


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", RR.CASES)
def test_the_cases_are_decidable_and_fp32_is_close(syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """The cases of tests/test_gpu_raster.py, from the restatement alone: at most 0.2 % of a case's pixels are undecidable; fp32 and
    fp64 give the same radii and rectangles for every decidable Gaussian; the case's bound stays under the ceiling."""
    c = RR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    share = c["undecidable"].mean()
    dec = c["decidable"]
    covered = (c["r64"]["image"][..., 3] > 0.5).mean()
    print(f"n={n} {width}x{height} views={views} deg={sh_degree}: undecidable pixels {share:.5f}, undecidable Gaussians {(~dec).mean():.5f}, "
          f"instances {c['r64']['instances']}, alpha > 0.5 on {covered:.3f} of the pixels, max |fp32 - fp64| {c['rounding']:.3e}")
    assert share <= RR.MAX_UNDECIDABLE_SHARE, share
    assert np.array_equal(c["r32"]["radii"][dec], c["r64"]["radii"][dec])
    assert np.array_equal(c["r32"]["rect"][dec], c["r64"]["rect"][dec])
    assert dec.mean() > 0.9 and (c["r64"]["radii"] > 0).mean() > 0.5
    assert RR.bound(c["rounding"]) <= RR.ERROR_CEILING, c["rounding"]
    assert c["r64"]["instances_lo"] <= c["r64"]["instances"] <= c["r64"]["instances_hi"]
    assert covered > 0.05
