"""A coarse-to-fine refinement schedule, without a GPU: csrc/pyramid_rules.h -- a level's geometry, the value of a target pixel and
the keep-the-input rule -- through its host instantiation (libsixdgs_hostcheck.so) against the restatements of
tests/pyramid_reference.py, refine.prepare_target and refine.scaled_intrinsics; refine.level_plan's refusals; what the new entry points
answer and refuse without a device."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_reference as R  # noqa: E402

torch = pytest.importorskip("torch")

F = np.float32
BADARG, WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def hc():
    return C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())


@pytest.fixture(scope="module")
def refine():
    return importlib.import_module("6dgs_amd.refine")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_target(hc, images, d, composite=False, background=(1.0, 1.0, 1.0)):
    images = np.ascontiguousarray(images, np.uint8)
    V, H, W, Cn = images.shape
    w, h, _, _ = R.geometry(W, H, d)
    out = np.full((V, h, w, 3), np.nan, F)
    bg = np.asarray(background, F)
    assert hc.hc_pyr_target(_ptr(images), V, H, W, Cn, int(composite), _ptr(bg), d, _ptr(out)) == 0
    return out


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def test_geometry_is_the_reference_and_prepare_targets_and_scaled_intrinsics(hc, refine):
    assert hc.hc_pyr_max_levels() == R.MAX_LEVELS == refine.MAX_LEVELS and hc.hc_pyr_max_downscale() == R.MAX_DOWNSCALE == refine.MAX_DOWNSCALE
    k4 = np.asarray([311.7, 298.3, 19.61, 21.37], F)
    K = torch.tensor([[k4[0], 0.0, k4[2]], [0.0, k4[1], k4[3]], [0.0, 0.0, 1.0]], dtype=torch.float32)
    geo, kout = np.zeros(4, np.int32), np.zeros(4, F)
    checked = 0
    for W in range(1, 41):
        for H in range(1, 41):
            image = torch.zeros(1, H, W, 3, dtype=torch.uint8)
            for d in range(1, 10):
                hc.hc_pyr_geometry(W, H, d, _ptr(k4), _ptr(geo), _ptr(kout))
                w, h, ox, oy = R.geometry(W, H, d)
                assert geo.tolist() == [w, h, ox, oy], (W, H, d)
                assert np.array_equal(R.bits(kout), R.bits(R.intrinsics(k4, d, ox, oy))), (W, H, d)
                assert np.array_equal(R.bits(kout), R.bits(refine.scaled_intrinsics(K, d, ox, oy).numpy())), (W, H, d)
                if w < 1 or h < 1:
                    with pytest.raises(ValueError):
                        refine.prepare_target(image, d, "composite")
                    with pytest.raises(ValueError):
                        refine.level_plan([(d, 1, 1e-3)], W, H)
                    continue
                target, px, py = refine.prepare_target(image, d)
                assert (px, py) == (ox, oy) and tuple(target.shape) == (1, h, w, 3), (W, H, d)
                plan = refine.level_plan([(d, 3, 1e-3)], W, H)[0]
                assert (plan["width"], plan["height"], plan["crop_x"], plan["crop_y"]) == (w, h, ox, oy)
                checked += 1
    assert checked > 10000


# ---- the target expression ----------------------------------------------------------------------------------------------------------
def _images(kind, V, H, W, Cn, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        im = np.zeros((V, H, W, Cn), np.uint8)
    elif kind == "full":
        im = np.full((V, H, W, Cn), 255, np.uint8)
    else:
        im = rng.integers(0, 256, (V, H, W, Cn), dtype=np.uint8)
    if Cn == 4 and kind in ("alpha0", "alpha255"):
        im[..., 3] = 0 if kind == "alpha0" else 255
    return im


SHAPES = {1: (7, 5), 2: (9, 6), 3: (10, 7), 16: (37, 33), 256: (513, 258)}       # d -> (W, H): a crop on both axes where d > 1


@pytest.mark.parametrize("d", sorted(SHAPES))
@pytest.mark.parametrize("kind", ("random", "zeros", "full", "alpha0", "alpha255"))
def test_target_value_is_the_fp32_restatement_and_within_its_bound_of_fp64(hc, refine, d, kind):
    W, H = SHAPES[d]
    worst = 0.0
    for Cn, composite, bg in ((3, False, None), (4, False, None), (4, True, (1.0, 1.0, 1.0)), (4, True, (0.0, 0.25, 0.7))):
        if Cn == 3 and kind.startswith("alpha"):
            continue
        im = _images(kind, 2 if d < 256 else 1, H, W, Cn, 100 * d + Cn)
        kw = dict(composite=composite, background=bg or (1.0, 1.0, 1.0))
        got, r32, r64 = host_target(hc, im, d, **kw), R.target_f32(im, d, **kw), R.target_f64(im, d, **kw)
        assert got.shape == r32.shape and np.array_equal(R.bits(got), R.bits(r32)), (Cn, composite, bg)
        limit = R.bound_f32(r64, composite)
        err = np.abs(got.astype(np.float64) - r64)
        assert np.isfinite(got).all() and (err <= limit).all(), (Cn, composite, bg, float((err / limit).max()))
        worst = max(worst, float((err / limit).max()))
        if kind in ("zeros", "full") and not composite:
            assert np.all(got == F(0.0 if kind == "zeros" else 1.0))
        # prepare_target on the CPU: the same mean by another route
        tt, _, _ = refine.prepare_target(torch.from_numpy(im), d, "composite" if composite else "ignore", kw["background"])
        t = tt.numpy().astype(np.float64) / (255.0 if tt.dtype == torch.uint8 else 1.0)
        assert t.shape == r64.shape
        assert (np.abs(t - r64) <= R.bound_prepare(d, composite)).all() and (np.abs(t - got) <= R.bound_prepare(d, composite) + limit).all()
    print(f"d {d}, {kind}: worst measured / bound {worst:.3f}")


def test_composite_with_opaque_alpha_is_the_plain_value_to_its_bound(hc):
    im = _images("alpha255", 1, 12, 14, 4, 5)
    a, b = host_target(hc, im, 4, composite=True, background=(0.2, 0.4, 0.6)), R.target_f64(im, 4)
    assert (np.abs(a - b) <= R.bound_f32(b, True)).all()
    clear = host_target(hc, _images("alpha0", 1, 12, 14, 4, 6), 4, composite=True, background=(0.25, 0.5, 1.0))
    assert np.all(clear == np.asarray([0.25, 0.5, 1.0], F))


def test_host_target_refuses_what_the_entry_point_refuses(hc):
    im = np.zeros((1, 8, 8, 3), np.uint8)
    out, bg = np.zeros((1, 8, 8, 3), F), np.ones(3, F)
    for d, Cn, composite in ((0, 3, 0), (257, 3, 0), (9, 3, 0), (2, 3, 1), (2, 5, 0)):
        assert hc.hc_pyr_target(_ptr(im), 1, 8, 8, Cn, composite, _ptr(bg), d, _ptr(out)) == -1, (d, Cn, composite)


# ---- the keep-the-input rule --------------------------------------------------------------------------------------------------------
def test_keep_input_rule_on_planted_values(hc):
    nan, inf = np.nan, np.inf
    cases = [(0.5, 1.0, 0), (1.0, 1.0, 1), (1.5, 1.0, 1), (nan, 1.0, 1), (0.5, nan, 1), (nan, nan, 1), (inf, 1.0, 1), (0.5, inf, 0), (inf, inf, 1),
             (0.0, 1e-45, 0), (-0.0, 0.0, 1)]
    best, inp = np.asarray([c[0] for c in cases], F), np.asarray([c[1] for c in cases], F)
    keep = np.full(len(cases), -1, np.int32)
    hc.hc_pyr_keep_input(_ptr(best), _ptr(inp), C.c_longlong(len(cases)), _ptr(keep))
    assert keep.tolist() == [c[2] for c in cases]
    assert R.keep_input(best, inp).astype(np.int32).tolist() == keep.tolist()


# ---- level_plan and refine_poses' refusals --------------------------------------------------------------------------------------------
def test_level_plan_normalises_and_refuses(refine):
    plan = refine.level_plan([(8, 30, 4e-3), [4, np.int64(30), 2e-3], (2, 40, 1)], 70, 66)
    assert [(p["downscale"], p["steps"], p["lr"]) for p in plan] == [(8, 30, 4e-3), (4, 30, 2e-3), (2, 40, 1.0)]
    assert [(p["width"], p["height"], p["crop_x"], p["crop_y"]) for p in plan] == [(8, 8, 3, 1), (17, 16, 1, 1), (35, 33, 0, 0)]
    assert all(type(p["downscale"]) is int and type(p["steps"]) is int and type(p["lr"]) is float for p in plan)
    assert refine.parse_levels("8:30:4e-3, 4:30:2e-3,2:40:1e-3") == [(8, 30, 4e-3), (4, 30, 2e-3), (2, 40, 1e-3)]
    ok = (2, 5, 1e-3)
    bad = ([], [ok] * 9, [(0, 5, 1e-3)], [(-2, 5, 1e-3)], [(2.5, 5, 1e-3)], [(True, 5, 1e-3)], [(2, 0, 1e-3)], [(2, 1.5, 1e-3)], [(2, True, 1e-3)],
           [(2, 5, 0.0)], [(2, 5, -1e-3)], [(2, 5, float("inf"))], [(2, 5, float("nan"))], [(2, 5, "1e-3")], [(2, 5)], [(257, 5, 1e-3)], [(71, 5, 1e-3)],
           [(67, 5, 1e-3)], [ok, (2, 5, 1e-3, 4)], 5)
    for levels in bad:
        with pytest.raises(ValueError):
            refine.level_plan(levels, 70, 66)
    assert len(refine.level_plan([ok] * 8, 70, 66)) == 8 and refine.level_plan([(66, 1, 1e-3)], 70, 66)[0]["height"] == 1
    assert refine.level_plan([(256, 1, 1e-3)], 600, 300)[0]["width"] == 2
    for text in ("8:30", "8:30:x", "a:30:1e-3", ""):
        with pytest.raises(ValueError):
            refine.parse_levels(text)


def test_refine_poses_refuses_levels_beside_a_downscale_before_any_gpu_is_touched(refine):
    class NoScene:                       # any attribute access would be a use of the scene
        def __getattr__(self, name):
            raise AssertionError(f"the scene was touched ({name})")

    images = [np.zeros((16, 16, 3), np.uint8)]
    pose, K = np.eye(4, dtype=F)[None], np.eye(3, dtype=F)
    for d in (3, 4):                     # any downscale beside levels, the single-level default's value included
        with pytest.raises(ValueError, match="exclude"):
            refine.refine_poses(NoScene(), images, pose, K, levels=[(2, 5, 1e-3)], downscale=d)
    with pytest.raises(ValueError, match="nothing"):          # steps and lr are ignored with levels, not checked: the plan is what fails
        refine.refine_poses(NoScene(), images, pose, K, levels=[(32, 5, 1e-3)], steps=0, lr=-1.0)
    with pytest.raises(ValueError):
        refine.refine_poses(NoScene(), images, pose, K, levels=[(32, 5, 1e-3)])          # nothing left of a 16 x 16 image
    with pytest.raises(ValueError):
        refine.refine_poses(NoScene(), images, pose, K, levels=[(2, 5, 1e-3)] * 9)


def test_refine_levels_flag_of_the_evaluation_script():
    pea = importlib.import_module("6dgs_amd.pretrain_eval_attention")
    base = ["--exp_path", "e", "--out_path", "o"]
    off, _ = pea.parse_args(base)
    assert not hasattr(off, "refine_levels")                  # off by default: the namespace is what it was
    on, rest = pea.parse_args(base + ["--refine_levels", "8:30:4e-3,4:30:2e-3,2:40:1e-3", "--refine_backend", "fused"])
    assert on.refine_levels == [(8, 30, 4e-3), (4, 30, 2e-3), (2, 40, 1e-3)] and rest == [] and on.refine_steps == 0
    for bad in (["--refine_levels", "8:30"], ["--refine_levels", "0:30:1e-3"], ["--refine_levels", "2:30:1e-3", "--refine_downscale", "2"], ["--refine_downscale", "4", "--refine_levels", "2:30:1e-3"],
                ["--refine_levels", ",".join(["2:5:1e-3"] * 9)]):
        with pytest.raises(SystemExit):
            pea.parse_args(base + bad)


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_refuse_without_a_device():
    L = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    names = ("sixdgs_target_pyramid", "sixdgs_pose_rebase", "sixdgs_refine_poses_levels_workspace_bytes", "sixdgs_refine_poses_levels")
    for name in names:
        assert name in L.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert [len(L.SIGNATURES[n][1]) for n in names] == [11, 5, 6, 38]
    assert "pyramid.hip" in build.SOURCES and "pyramid_rules.h" in build.HEADERS and L.ABI_VERSION == 10
    lib = L.load()
    fake = C.c_void_p(4096)                                  # never dereferenced: every call below is refused before a launch
    bg = (C.c_float * 3)(1.0, 1.0, 1.0)
    outs = (C.c_void_p * 9)(*[4096] * 9)

    def pyramid(ds, views=1, H=16, W=16, Cn=3, composite=0, background=bg, out=outs):
        h_d = (C.c_int32 * max(len(ds), 1))(*ds)
        return lib.sixdgs_target_pyramid(fake, views, H, W, Cn, composite, C.cast(background, C.c_void_p) if background is not None else None,
                                         len(ds), C.cast(h_d, C.c_void_p), C.cast(out, C.c_void_p), None)

    assert pyramid([]) == BADARG and pyramid([2] * 9) == BADARG                     # 0 and 9 levels
    assert pyramid([257]) == BADARG and pyramid([0]) == BADARG and pyramid([17]) == BADARG      # d outside 1 .. 256; nothing left of 16 x 16
    assert pyramid([8, 4, 17, 1]) == BADARG                                         # one bad level refuses the whole call
    assert pyramid([2], Cn=5) == BADARG and pyramid([2], Cn=3, composite=1) == BADARG and pyramid([2], Cn=4, composite=1, background=None) == BADARG
    assert pyramid([2], views=-1) == BADARG and pyramid([2], views=65536) == BADARG and pyramid([2], W=32769) == BADARG
    assert pyramid([2], out=(C.c_void_p * 9)(*[4097] * 9)) == BADARG and pyramid([2], out=(C.c_void_p * 9)()) == BADARG
    assert pyramid([2], views=0) == 0                                               # nothing to do
    assert lib.sixdgs_pose_rebase(None, fake, 2, fake, None) == BADARG and lib.sixdgs_pose_rebase(fake, fake, 2, fake, None) == BADARG
    assert lib.sixdgs_pose_rebase(fake, C.c_void_p(8192), -1, C.c_void_p(12288), None) == BADARG
    assert lib.sixdgs_pose_rebase(None, None, 0, None, None) == 0
    # the workspace: the largest level's, plus two sets of rows
    ops = importlib.import_module("6dgs_amd.ops")
    one = [ops.refine_poses_workspace_bytes(2000, 2, s, s, 50000) for s in (16, 32, 64)]
    both = ops.refine_poses_levels_workspace_bytes(2000, 2, [(16, 16), (32, 32), (64, 64)], [50000] * 3)
    assert both == max(one) + 2 * 256 and max(one) == one[2] > one[0]
    assert ops.refine_poses_levels_workspace_bytes(2000, 2, [(64, 64), (16, 16)], [50000, 50000]) == both
    assert ops.refine_poses_levels_workspace_bytes(2000, 2, [(16, 16)] * 9, [50000] * 9) == 0
    assert ops.refine_poses_levels_workspace_bytes(2000, 2, [(16, 16), (0, 16)], [50000] * 2) == 0
    assert ops.refine_poses_levels_workspace_bytes(2000, 2, [(16, 16)], [0]) == 0
