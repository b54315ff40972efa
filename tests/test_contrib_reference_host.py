"""CPU tests of the contribution feature: the numpy restatement (tests/contrib_reference.py) held to account -- a pixel's summed w is
the reference image's 1 - T, the hand cases give the counts their geometry dictates, the fit cases qualify for an equality test --, the
declaration of the entry points, their argument handling (answered without a GPU), GaussianScene.subset and prune_by_contribution."""
import importlib
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrib_reference as CR  # noqa: E402
import raster_reference as RR  # noqa: E402

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_raster_contrib_workspace_bytes", "sixdgs_raster_contrib", "sixdgs_scene_contrib_workspace_bytes", "sixdgs_scene_contrib")


def test_tile_tree_is_the_stated_tree():
    rng = np.random.default_rng(0)
    w = rng.random((3, 256)).astype(np.float32)
    for g in range(3):
        groups = []
        for k in range(4):
            x = w[g, 64 * k:64 * k + 64].copy()
            for s in (32, 16, 8, 4, 2, 1):
                x = np.array([np.float32(x[lane] + x[lane ^ s]) for lane in range(64)], np.float32)
            groups.append(x[0])
        want = np.float32(np.float32(np.float32(groups[0] + groups[1]) + groups[2]) + groups[3])
        assert CR.tile_tree(w[g:g + 1])[0] == want
    assert CR.tile_tree(np.zeros((2, 256), np.float32)).tolist() == [0.0, 0.0]
    assert abs(float(CR.tile_tree(w.astype(np.float64))[0]) - float(w[0].astype(np.float64).sum())) < 1e-12


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", CR.CASES)
def test_cases_qualify_and_sum_to_the_image_alpha(syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """Every fit case: no undecidable pixel in either restatement, every Gaussian decidable, a bound under the ceiling -- and, per
    pixel, the w of the Gaussians it added sum to 1 - T of raster_reference's image, in both precisions."""
    c = CR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    assert not c["undecidable"].any() and c["decidable"].all()
    b = CR.bound(c["rounding"])
    print(f"n={n} {width}x{height} deg={sh_degree}: fp32 restatement deviates {c['rounding']:.3e}, bound {b:.3e}")
    assert b <= RR.ERROR_CEILING
    r64, r32 = c["r64"], c["r32"]
    assert np.abs(r64["pixel_sum"] - r64["image_alpha"]).max() <= 1e-12
    # fp32, per Gaussian a pixel adds: 1 - alpha, T', w and the running sum are each rounded once, and T + sum <= 1, T' + w <= 1
    adds = r32["view_pixels"].sum()
    assert (np.abs(r32["pixel_sum"].astype(np.float64) - r32["image_alpha"]) <= 2.0 ** -23 * (r32["pixel_adds"] + 1)).all()
    for k in ("view_pixels", "view_stops", "pixels", "stops", "seen", "inert"):
        assert np.array_equal(r64[k], r32[k]), k
    assert adds > 0 and r64["stops"].sum() >= 0 and r64["inert"].any() and not r64["inert"].all()
    assert np.array_equal(r64["seen"], (r64["view_weight"] > 0).sum(0)) and (r64["peak"] <= r64["weight"] + 1e-15).all()
    assert abs(r64["view_weight"].sum() - r64["image_alpha"].sum()) <= 1e-9 * adds


def _one(scene, row=CR.ROW, width=32, height=32):
    c = CR.pair(scene, row, width, height)
    assert not c["undecidable"].any(), "the hand case has an undecidable pixel"
    for k in ("pixels", "stops", "seen", "inert"):
        assert np.array_equal(c["r64"][k], c["r32"][k]), k
    return c


def test_hand_cases_give_the_stated_counts():
    # one isotropic Gaussian: weight is the sum of its alphas (T = 1), peak the alpha of the pixels next to the centre
    c = _one(CR.hand_one())
    r = c["r64"]
    var = (0.2 * 20 / 2.0) ** 2 + 0.3          # sigma f / z squared, + 0.3
    o = 1.0 / (1.0 + math.exp(-float(CR.hand_one()["opacity"][0, 0])))
    ys, xs = np.mgrid[0:32, 0:32]
    alpha = o * np.exp(-0.5 * ((16 - xs - 0.5) ** 2 + (16 - ys - 0.5) ** 2) / var)
    on = alpha >= 1.0 / 255.0
    assert r["pixels"][0] == on.sum() and r["stops"][0] == 0 and r["seen"][0] == 1 and not r["inert"][0]
    assert abs(r["weight"][0] - alpha[on].sum()) < 1e-5 * alpha[on].sum() and abs(r["peak"][0] - alpha[16, 16]) < 1e-6
    # saturation: on the middle pixels the third stops and adds nothing, the fourth is not reached
    scene = CR.hand_saturation()
    r = _one(scene)["r64"]
    mid = {k: v[:, 12:20, 12:20] for k, v in (("pixel_sum", r["pixel_sum"]),)}
    assert (mid["pixel_sum"] > 0.999).all()
    sub = {k: (v[2:] if isinstance(v, np.ndarray) else v) for k, v in scene.items()}       # the third and fourth alone do add
    assert (_one(sub)["r64"]["pixels"] > 0).all()
    P = RR.project(scene, CR.ROW[0], 32, 32, np.float64)
    ys, xs = np.mgrid[12:20, 12:20]
    w, adds, stops = CR._walk_tile(P, np.arange(4), xs.reshape(-1), ys.reshape(-1), np.float64)
    assert adds[:2].all() and not adds[2:].any() and stops[2].all() and not stops[[0, 1, 3]].any() and (w[2:] == 0).all()
    assert r["stops"][2] >= 64 and r["stops"][[0, 1]].sum() == 0
    # nothing: culled, empty rectangle, too faint
    r = _one(CR.hand_nothing())["r64"]
    assert r["inert"].all() and not r["weight"].any() and not r["peak"].any() and not r["pixels"].any() and not r["stops"].any() and not r["seen"].any()
    # the corner: only the pixels inside the image count -- a quarter of the footprint
    shifted = CR.ROW.copy()
    shifted[0, 14:] = 32.0                      # the same footprint, whole, in the middle of a 64 x 64 image
    whole, corner = _one(CR.hand_corner(), shifted, 64, 64)["r64"], _one(CR.hand_corner())["r64"]
    assert whole["pixels"][0] / 5 < corner["pixels"][0] < whole["pixels"][0] / 3 and corner["pixels"][0] == (corner["pixel_sum"][0] > 0).sum()
    assert (corner["pixel_sum"][0, 16:, :] == 0).all() and (corner["pixel_sum"][0, :, 16:] == 0).all()


def test_a_list_longer_than_one_round():
    c = _one(CR.hand_long(), CR.ROW_LONG, 24, 16)
    r = c["r64"]
    k = CR.LONG_ADDS
    assert (r["pixels"][:k] == 384).all() and (r["stops"][:k] == 0).all()          # 256 + 128: the right tile is half outside
    assert r["pixels"][k] == 0 and r["stops"][k] == 384 and r["weight"][k] == 0
    assert not r["pixels"][k + 1:].any() and not r["stops"][k + 1:].any() and not r["weight"][k + 1:].any() and r["inert"][k + 1:].all()
    P = RR.project(CR.hand_long(), CR.ROW_LONG[0], 24, 16, np.float64)
    ys, xs = np.mgrid[0:16, 0:24]
    _, a = RR._alpha(P, np.arange(1), xs.reshape(-1), ys.reshape(-1), np.float64)
    want = (a[0][None, :] * (1 - a[0][None, :]) ** np.arange(k)[:, None]).sum(axis=1)
    assert np.abs(r["weight"][:k] - want).max() <= 1e-12 * want.max()
    assert CR.bound(c["rounding"]) <= RR.ERROR_CEILING


def test_entry_points_are_declared_and_bound():
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(lib.load(), name), f"{name} is not exported"
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES] == [5, 18, 5, 30]
    assert lib.ABI_VERSION == 10 and "contrib.hip" in build.SOURCES


def test_workspace_sizes_and_argument_errors_need_no_gpu():
    ops = importlib.import_module("6dgs_amd.ops")
    lib = importlib.import_module("6dgs_amd._lib").load()
    assert ops.raster_contrib_workspace_bytes(1000, 2, 40, 24, 1) == 256 and ops.raster_contrib_workspace_bytes(1000, 2, 40, 24, 17) == 512
    assert ops.raster_contrib_workspace_bytes(1000, 2, 40, 24, 1 << 20) == 16 << 20
    for bad in ((-1, 2, 40, 24, 10), (1 << 31, 2, 40, 24, 10), (10, 65536, 40, 24, 10), (10, 2, 0, 24, 10), (10, 2, 40, 16385, 10), (10, 2, 40, 24, 0),
                (10, 2, 40, 24, 1 << 31)):
        assert ops.raster_contrib_workspace_bytes(*bad) == 0, bad
    fwd, walk = ops.raster_views_workspace_bytes(1000, 3, 40, 24, 5000), ops.raster_contrib_workspace_bytes(1000, 3, 40, 24, 5000)
    assert ops.scene_contrib_workspace_bytes(1000, 3, 40, 24, 5000) == fwd + walk + 256 and fwd % 256 == 0 and walk % 256 == 0
    assert ops.scene_contrib_workspace_bytes(1000, 0, 40, 24, 5000) == 0 and ops.scene_contrib_workspace_bytes(1000, 3, 40, 24, 0) == 0
    # the raw call: every refusal comes back before anything is launched (this process has no GPU to launch on); the pointers are
    # never followed, so aligned made-up addresses stand in for device memory
    A, W = 1 << 20, 2 << 20
    fwd1 = ops.raster_views_workspace_bytes(10, 2, 40, 24, 100)
    walk1 = ops.raster_contrib_workspace_bytes(10, 2, 40, 24, 100)
    call = lambda n=10, views=2, w=40, h=24, cap=100, f=A, fb=fwd1, outs=(None,) * 7, ws=W, wb=walk1: lib.sixdgs_raster_contrib(  # noqa: E731
        n, views, w, h, cap, f, fb, *outs, ws, wb, None, None)
    assert call(n=-1) == -1 and call(views=65536) == -1 and call(w=0) == -1 and call(h=16385) == -1 and call(cap=0) == -1
    assert call(f=None) == -1 and call(fb=fwd1 - 1) == -2 and call(wb=walk1 - 1) == -2 and call(ws=None) == -1 and call(ws=W + 8) == -1 and call(f=A + 8) == -1
    assert call(outs=(A + 2,) + (None,) * 6) == -1 and call(outs=(None, None, A + 4) + (None,) * 4) == -1
    assert call(views=0, f=None) == 0 and call(n=0, f=None) == 0 and call() == 0          # nothing to do; every output NULL
    scene = (A, A, 1, A, A, 1, A, None, 0, 1, 10)
    need = ops.scene_contrib_workspace_bytes(10, 2, 40, 24, 100)
    drive = lambda views=2, chunk=2, cap=100, cams=A, status=A, needed=A, ws=W, wb=need, sm=1.0, args=scene: lib.sixdgs_scene_contrib(  # noqa: E731
        *args, cams, views, 40, 24, sm, chunk, cap, *(None,) * 7, status, needed, ws, wb, None)
    assert drive(chunk=0) == -1 and drive(cap=0) == -1 and drive(views=-1) == -1 and drive(sm=0.0) == -1 and drive(cams=None) == -1
    assert drive(status=None) == -1 and drive(needed=None) == -1 and drive(needed=A + 4) == -1 and drive(wb=need - 1) == -2 and drive(ws=None) == -1
    assert drive(args=(None,) + scene[1:]) == -1 and drive(args=scene[:8] + (1, 1, 10)) == -1
    assert drive(views=0, cams=None, status=None) == 0


def _scene(n=12, sh_degree=2, seed=0):
    pkg = importlib.import_module("6dgs_amd")
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    s = pkg.GaussianScene.from_arrays(r(n, 3), r(n, 3), r(n, 4), r(n, 1, 3), r(n, (sh_degree + 1) ** 2 - 1, 3), r(n, 1), sh_degree, device="cpu")
    s.active_sh_degree = 1
    return pkg, s


FIELDS = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")


def test_subset():
    pkg, s = _scene()
    before = [getattr(s, k).clone() for k in FIELDS]
    mask = torch.tensor([True, False] * 6)
    a, b = s.subset(mask), s.subset(torch.arange(0, 12, 2))
    for sub in (a, b):
        assert isinstance(sub, pkg.GaussianScene) and len(sub) == 6 and sub.active_sh_degree == 1 and sub.max_sh_degree == 2
        for k, t in zip(FIELDS, before):
            assert torch.equal(getattr(sub, k), t[::2]) and getattr(sub, k).is_contiguous() and torch.equal(getattr(s, k), t)
            assert getattr(sub, k).data_ptr() != getattr(s, k).data_ptr()
    assert len(s.subset(torch.zeros(12, dtype=torch.bool))) == 0 and len(s.subset(np.ones(12, bool))) == 12
    for bad in (torch.ones(11, dtype=torch.bool), torch.tensor([3, 2]), torch.tensor([1, 1]), torch.tensor([12]), torch.tensor([-1]), torch.ones(12)):
        with pytest.raises(ValueError):
            s.subset(bad)


def _contrib(weight, peak, pixels, stops, seen):
    return {"weight": torch.tensor(weight, dtype=torch.float32), "peak": torch.tensor(peak, dtype=torch.float32),
            "pixels": torch.tensor(pixels, dtype=torch.int64), "stops": torch.tensor(stops, dtype=torch.int64),
            "seen": torch.tensor(seen, dtype=torch.int32)}


def test_prune_by_contribution():
    pkg, s = _scene(6)
    before = [getattr(s, k).clone() for k in FIELDS]
    c = _contrib([5.0, 0.0, 2.0, 2.0, 0.0, 2.0], [0.9, 0.0, 0.5, 0.05, 0.0, 0.2], [40, 0, 9, 30, 0, 7], [0, 0, 0, 0, 3, 0], [3, 0, 1, 2, 0, 2])
    frozen = {k: v.clone() for k, v in c.items()}
    keep = lambda **kw: pkg.prune_by_contribution(s, c, **kw)[1].tolist()      # noqa: E731
    assert keep() == [True, False, True, True, True, True]                     # index 4 stops pixels: not inert
    assert keep(drop_inert=False) == [True] * 6
    assert keep(min_peak=0.2) == [True, False, True, False, False, True]
    assert keep(min_seen=2) == [True, False, False, True, False, True]
    assert keep(drop_inert=False, min_seen=0, min_peak=0.0) == [True] * 6
    # the largest weights, ties to the smaller index: 5, then 2 = 2 = 2 at indices 2, 3, 5
    assert keep(drop_inert=False, keep_fraction=0.5) == [True, False, True, True, False, False]
    assert keep(drop_inert=False, keep_fraction=1 / 3) == [True, False, True, False, False, False]
    assert keep(keep_fraction=1.0) == keep() and keep(keep_fraction=0.0) == [False] * 6
    assert keep(keep_fraction=0.5, min_peak=0.2) == [True, False, True, False, False, False]      # AND
    new, k = pkg.prune_by_contribution(s, c, min_seen=2)
    assert len(new) == 3 and k.dtype == torch.bool and new.active_sh_degree == s.active_sh_degree
    for f, t in zip(FIELDS, before):
        assert torch.equal(getattr(new, f), t[k]) and torch.equal(getattr(s, f), t)
    assert all(torch.equal(c[f], frozen[f]) for f in c)
    for bad in (dict(min_peak=-1.0), dict(min_seen=-1), dict(min_seen=1.5), dict(keep_fraction=1.5)):
        with pytest.raises(ValueError):
            pkg.prune_by_contribution(s, c, **bad)
    with pytest.raises(ValueError):
        pkg.prune_by_contribution(_scene(5)[1], c)
    with pytest.raises(ValueError):
        pkg.prune_by_contribution(s, {"weight": c["weight"]})
