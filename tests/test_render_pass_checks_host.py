"""The argument checks of the render-and-compare family without a GPU, stated once for every member.

Python: a table of malformed scenes, view arguments and targets, each applied to every function of the family that takes the argument
(ops.splat_views, raster_views, raster_views_backward, photometric_loss, refine_poses_raw, fit_scene_raw and _fit_params).  The tensors
are CPU tensors, so a call that got past its checks would raise the "must live on the GPU" RuntimeError: every case must raise
ValueError instead.  Sizes: 5 Gaussians, 2 views, 16 x 16.

C, through ctypes: for sixdgs_raster_views, sixdgs_raster_views_backward, sixdgs_refine_poses and sixdgs_fit_scene a table of calls
that are refused before the first HIP call, with the status each must return.  The device pointers are 256-aligned dummy integers:
every row is refused first, so none is dereferenced, and no row would pass validation."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as RR  # noqa: E402

torch = pytest.importorskip("torch")

N, V, W, H = 5, 2, 16, 16
SCENE = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")
BADARG, WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def good(syn):
    sc = {k: torch.from_numpy(np.asarray(v)).float().contiguous() for k, v in syn.make_scene(N, 0).items() if k != "sh_degree"}
    scene = {"xyz": sc["xyz"], "scale": sc["log_scale"], "rot": sc["rot"], "opacity": sc["opacity"], "f_dc": sc["f_dc"], "f_rest": sc["f_rest"]}
    assert scene["xyz"].shape == (N, 3) and scene["rot"].shape == (N, 4) and scene["f_rest"].shape == (N, 15, 3)
    cams = torch.from_numpy(RR.camera_rows(syn.make_cameras(V, 0, width=W, height=H))).float().contiguous()
    assert cams.shape == (V, 16)
    return dict(scene=scene, cams=cams, width=W, height=H, background=(1.0, 1.0, 1.0), scale_modifier=1.0,
                target=torch.zeros(V, H, W, 3), image=torch.zeros(V, H, W, 4))


# name -> (the arguments of `good` it reads, the call)
def _family(ops):
    def scene6(a):
        return [a["scene"][k] for k in SCENE]

    state = (torch.zeros(1 << 16, dtype=torch.uint8), 4096)
    return {
        "splat_views": ({"xyz", "scale", "f_dc", "f_rest", "cams", "width", "background"},
                        lambda a: ops.splat_views(a["scene"]["xyz"], a["scene"]["scale"], a["scene"]["f_dc"], a["scene"]["f_rest"], 3, a["cams"],
                                                  a["width"], a["height"], background=a["background"])),
        "raster_views": ({*SCENE, "cams", "width", "background", "scale_modifier"},
                         lambda a: ops.raster_views(*scene6(a), 3, a["cams"], a["width"], a["height"], background=a["background"],
                                                    scale_modifier=a["scale_modifier"])),
        "raster_views_backward": ({*SCENE, "cams", "width", "background", "scale_modifier"},
                                  lambda a: ops.raster_views_backward(*scene6(a), 3, a["cams"], a["width"], a["height"], a["image"], state,
                                                                      background=a["background"], scale_modifier=a["scale_modifier"])),
        "photometric_loss": ({"target"}, lambda a: ops.photometric_loss(a["image"], a["target"])),
        "refine_poses_raw": ({*SCENE, "cams", "width", "background", "scale_modifier", "target"},
                             lambda a: ops.refine_poses_raw(*scene6(a), 3, a["cams"], a["width"], a["height"], a["target"], steps=2,
                                                            background=a["background"], scale_modifier=a["scale_modifier"])),
        "fit_scene_raw": ({*SCENE, "cams", "width", "background", "scale_modifier", "target"},
                          lambda a: ops.fit_scene_raw(a["scene"], a["cams"], a["width"], a["height"], a["target"], views=[[0], [1]],
                                                      lrs=[[1e-3] * 6] * 2, sh_degrees=[0, 3], background=a["background"],
                                                      scale_modifier=a["scale_modifier"])),
        "_fit_params": ({*SCENE}, lambda a: ops._fit_params(a["scene"])),
    }


def _bad_inputs(good):
    """(label, the argument it spoils, the spoilt arguments)"""
    def with_scene(k, t):
        return dict(good, scene=dict(good["scene"], **{k: t}))

    sc = good["scene"]
    out = [(f"{k} short by a row", k, with_scene(k, sc[k][:N - 1].contiguous())) for k in SCENE]
    out += [("rot of width 3", "rot", with_scene("rot", sc["rot"][:, :3].contiguous())),
            ("f_rest of two channels", "f_rest", with_scene("f_rest", sc["f_rest"][..., :2].contiguous())),
            ("f_rest without its coefficient axis", "f_rest", with_scene("f_rest", sc["f_rest"].reshape(N, 45))),
            ("cams [V,12]", "cams", dict(good, cams=good["cams"][:, :12].contiguous())),
            ("cams 1-D", "cams", dict(good, cams=good["cams"].reshape(-1))),
            ("width 0", "width", dict(good, width=0, target=torch.zeros(V, H, 0, 3), image=torch.zeros(V, H, 0, 4))),
            ("background of 2 entries", "background", dict(good, background=(1.0, 1.0))),
            ("scale_modifier 0", "scale_modifier", dict(good, scale_modifier=0.0)),
            ("scale_modifier NaN", "scale_modifier", dict(good, scale_modifier=float("nan"))),
            ("uint8 target of 4 channels", "target", dict(good, target=torch.zeros(V, H, W, 4, dtype=torch.uint8))),
            ("float target of 2 channels", "target", dict(good, target=torch.zeros(V, H, W, 2))),
            ("target not contiguous", "target", dict(good, target=torch.zeros(V, H, W, 4)[..., :3])),
            ("target of the wrong V", "target", dict(good, target=torch.zeros(V + 1, H, W, 3))),
            ("target of the wrong H", "target", dict(good, target=torch.zeros(V, H - 1, W, 3))),
            ("target of the wrong W", "target", dict(good, target=torch.zeros(V, H, W + 1, 3)))]
    return out


def test_good_arguments_get_as_far_as_the_device(ops, good):
    """The table below means something only if the unspoilt call passes every check: it must stop at the tensors' device."""
    for name, (_, call) in _family(ops).items():
        if name == "_fit_params":
            assert call(good) == (N, 16)
            continue
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(good)


def test_malformed_inputs_are_value_errors_in_every_family_function(ops, good):
    family = _family(ops)
    seen = set()
    for label, spoils, args in _bad_inputs(good):
        for name, (takes, call) in family.items():
            if spoils not in takes:
                continue
            seen.add(name)
            try:
                call(args)
            except ValueError:
                continue
            except Exception as e:      # noqa: BLE001
                pytest.fail(f"{name}, {label}: {type(e).__name__} ({e}) where ValueError was due")
            pytest.fail(f"{name} accepted: {label}")
    assert seen == set(family)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
P = 256                     # a 256-aligned address that is never dereferenced
SH3 = dict(sh_degree=3, n_coef=16)


def _scene_args(a):
    return (a["xyz"], a["scale"], 1, a["rot"], a["opacity"], 1, a["f_dc"], a["f_rest"])


def _base():
    return dict(xyz=P, scale=P, rot=P, opacity=P, f_dc=P, f_rest=P, n=N, cams=P, views=V, width=W, height=H, scale_modifier=1.0, background=P,
                max_instances=4096, ws=P, ws_bytes=None, **SH3)


def _raster(L, **kw):
    a = {**_base(), **kw}
    need = L.sixdgs_raster_views_workspace_bytes(a["n"], a["views"], a["width"], a["height"], a["max_instances"])
    ws_bytes = need + (a["ws_bytes"] or 0)
    return L.sixdgs_raster_views(*_scene_args(a), a["sh_degree"], a["n_coef"], a["n"], a["cams"], a["views"], a["width"], a["height"],
                                 a["scale_modifier"], a["background"], P, None, 3, None, a["max_instances"], P, a["ws"], ws_bytes, None, None)


def _backward(L, **kw):
    a = {**_base(), "fwd_ws_bytes": 0, **kw}
    size = (a["n"], a["views"], a["width"], a["height"], a["max_instances"])
    fwd = L.sixdgs_raster_views_workspace_bytes(*size) + a["fwd_ws_bytes"]
    ws_bytes = L.sixdgs_raster_views_backward_workspace_bytes(*size) + (a["ws_bytes"] or 0)
    return L.sixdgs_raster_views_backward(*_scene_args(a), a["sh_degree"], a["n_coef"], a["n"], a["cams"], a["views"], a["width"], a["height"],
                                          a["scale_modifier"], a["background"], P, a["max_instances"], P, fwd, P, P, P, P, P, P, P, a["ws"], ws_bytes,
                                          None, None)


def _refine(L, **kw):
    a = {**_base(), "is_u8": 0, "stride": 3, "lam": 0.2, "steps": 2, **kw}
    need = L.sixdgs_refine_poses_workspace_bytes(a["n"], a["views"], a["width"], a["height"], a["max_instances"])
    ws_bytes = need + (a["ws_bytes"] or 0)
    return L.sixdgs_refine_poses(*_scene_args(a), a["sh_degree"], a["n_coef"], a["n"], a["cams"], a["views"], a["width"], a["height"],
                                 a["scale_modifier"], a["background"], P, a["is_u8"], a["stride"], a["lam"], a["steps"], 2e-3, 0.9, 0.999, 1e-8,
                                 a["max_instances"], P, P, P, P, P, P, P, a["ws"], ws_bytes, None)


def _fit(L, **kw):
    a = {**_base(), "is_u8": 0, "stride": 3, "lam": 0.2, "steps": 2, **kw}
    steps = max(a["steps"], 1)
    view = np.zeros((steps, 1), np.int32)
    lr = np.full((steps, 6), 1e-3, np.float32)
    degree = np.full(steps, a["sh_degree"], np.int32)
    reset = np.zeros(steps, np.uint8)
    need = L.sixdgs_fit_scene_workspace_bytes(a["n"], a["n_coef"], 1, a["width"], a["height"], a["max_instances"])
    ws_bytes = need + (a["ws_bytes"] or 0)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    return L.sixdgs_fit_scene(*_scene_args(a), a["n_coef"], a["n"], a["cams"], a["views"], a["width"], a["height"], a["scale_modifier"],
                              a["background"], P, a["is_u8"], a["stride"], a["lam"], a["steps"], 1, ptr(view), ptr(lr), ptr(degree), ptr(reset), 63,
                              0.9, 0.999, 1e-15, 0.01, a["max_instances"], 1024, 2048, P, P, P, a["ws"], ws_bytes, None)


# rows every entry point refuses: the scene's rules and the workspace's.  ws_bytes is relative to what the entry point asks for.
SHARED_ROWS = [
    (dict(sh_degree=4), BADARG),
    (dict(sh_degree=2, n_coef=8), BADARG),                  # n_coef below (sh_degree + 1)^2
    (dict(sh_degree=3, n_coef=17), BADARG),
    (dict(scale_modifier=0.0), BADARG),
    *[({k: None}, BADARG) for k in SCENE],                  # a NULL scene pointer with n > 0
    (dict(ws_bytes=-1), WORKSPACE),                         # one byte short
    (dict(ws=P + 128), BADARG),                             # large enough, misaligned
]
# the target's, the loss's and the loop's, where the entry point has them
LOOP_ROWS = [
    (dict(is_u8=1, stride=4), BADARG),
    (dict(lam=1.5), BADARG),
    (dict(steps=0), BADARG),
]


@pytest.mark.parametrize("name,call,rows", [("sixdgs_raster_views", _raster, SHARED_ROWS),
                                            ("sixdgs_raster_views_backward", _backward, SHARED_ROWS + [(dict(fwd_ws_bytes=-1), WORKSPACE)]),
                                            ("sixdgs_refine_poses", _refine, SHARED_ROWS + LOOP_ROWS),
                                            ("sixdgs_fit_scene", _fit, SHARED_ROWS + LOOP_ROWS)])
def test_entry_points_refuse_before_any_device_work(name, call, rows):
    L = importlib.import_module("6dgs_amd._lib").load()
    for kw, status in rows:
        assert call(L, **kw) == status, (name, kw)
    # a bad argument wins over a short workspace; the ws pointer is looked at after the size
    assert call(L, scale_modifier=0.0, ws_bytes=-1) == BADARG
    assert call(L, ws=P + 128, ws_bytes=-1) == WORKSPACE
    assert call(L, ws=None, ws_bytes=-1) == WORKSPACE
