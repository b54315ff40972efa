"""The rasteriser's backward (sixdgs_raster_views_backward) without a GPU: the entry points in the header, the binding and the library;
the answers that need no device; the refusals of ops.raster_views_backward and autograd.raster_views; and the torch restatement
(tests/raster_backward_reference.py) on the properties the GPU test relies on -- its fp64 image is raster_reference's, few pixels lose
their loss weight, every gradient array's bound stays under the ceiling -- and on values worked out by hand."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_raster_views_backward", "sixdgs_raster_views_backward_workspace_bytes")


def _call(L, **kw):
    """sixdgs_raster_views_backward with NULL scene and output pointers; kw overrides the scalar arguments.  cams, background, grad_image
    and fwd_ws are given as (never dereferenced) non-NULL addresses unless kw names them."""
    a = dict(scale_is_log=1, opacity_is_logit=1, sh_degree=3, n_coef=16, n=0, views=1, width=8, height=8, scale_modifier=1.0,
             max_instances=16, fwd_ws_bytes=0, ws_bytes=0, cams=256, background=256, grad_image=256, fwd_ws=256, ws=None)
    a.update(kw)
    nul = None
    return L.sixdgs_raster_views_backward(nul, nul, a["scale_is_log"], nul, nul, a["opacity_is_logit"], nul, nul, a["sh_degree"], a["n_coef"],
                                          a["n"], a["cams"], a["views"], a["width"], a["height"], a["scale_modifier"], a["background"],
                                          a["grad_image"], a["max_instances"], a["fwd_ws"], a["fwd_ws_bytes"], nul, nul, nul, nul, nul, nul, nul,
                                          a["ws"], a["ws_bytes"], nul, None)


def test_backward_entry_points_in_header_binding_and_library():
    ge = importlib.import_module("__graft_entry__")
    lib = importlib.import_module("6dgs_amd._lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert ge.header_abi_version() == 10 == lib.ABI_VERSION
    assert len(lib.SIGNATURES["sixdgs_raster_views_backward"][1]) == 32 and len(lib.SIGNATURES["sixdgs_raster_views_backward_workspace_bytes"][1]) == 5
    if os.path.exists(lib.LIB_PATH):
        so = C.CDLL(lib.LIB_PATH)
        for name in NAMES:
            assert hasattr(so, name), f"{name} is not exported by the library"
        L = lib.load()
        assert L.sixdgs_abi_version() == 10
        # sizes and argument errors are answered without touching the GPU
        ws = L.sixdgs_raster_views_backward_workspace_bytes
        assert ws(1000, 2, 64, 48, 5000) >= 36 * 5000 + 2 * 4 * 64
        assert ws(1000, 4, 64, 48, 5000) > ws(1000, 2, 64, 48, 5000) > ws(1000, 2, 64, 48, 50) and ws(0, 1, 8, 8, 1) > 0
        assert ws(100000, 2, 64, 48, 5000) > ws(1000, 2, 64, 48, 5000)
        assert ws(1000, 2, 64, 48, 0) == 0 and ws(-1, 2, 64, 48, 10) == 0 and ws(10, 2, 0, 48, 10) == 0 and ws(10, 2, 64, 48, 1 << 31) == 0
        assert ws(10, 65535, 16384, 16384, 10) == 0                         # views gx gy >= 2^31
        for bad in (dict(width=0), dict(height=20000), dict(n_coef=9), dict(sh_degree=4), dict(scale_modifier=0.0),
                    dict(scale_modifier=float("inf")), dict(max_instances=0), dict(max_instances=1 << 31), dict(n=-1), dict(views=-1),
                    dict(views=65535, width=16384, height=16384), dict(cams=None), dict(background=None), dict(grad_image=None),
                    dict(fwd_ws=None), dict(n=5)):                           # the last: NULL scene arrays
            assert _call(L, **bad) == -1, bad
        assert _call(L, views=0) == 0                                       # no views: nothing to do
        fwd = L.sixdgs_raster_views_workspace_bytes(0, 1, 8, 8, 16)
        need = ws(0, 1, 8, 8, 16)
        assert _call(L, fwd_ws_bytes=fwd - 1, ws_bytes=need) == -2          # SIXDGS_E_WORKSPACE: too small a forward workspace
        assert _call(L, fwd_ws_bytes=fwd, ws_bytes=need - 1) == -2
        assert _call(L, fwd_ws_bytes=fwd, ws_bytes=need) == -1              # NULL ws
        assert _call(L, fwd_ws_bytes=fwd, ws_bytes=need, ws=128) == -1      # misaligned ws


def _scene_tensors(syn, n=10):
    sc = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_scene(n, 0).items()}
    return (sc["xyz"], sc["log_scale"], sc["rot"], sc["opacity"], sc["f_dc"], sc["f_rest"], 3)


def test_backward_ops_refuse_cpu_tensors_and_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    ops = importlib.import_module("6dgs_amd.ops")
    autograd = importlib.import_module("6dgs_amd.autograd")
    assert pkg.raster_views is autograd.raster_views and "raster_views" in pkg.__all__
    args = _scene_tensors(syn)
    cams = torch.from_numpy(RR.camera_rows(syn.make_cameras(2, 0, width=16, height=16)))
    g = torch.zeros(2, 16, 16, 4)
    state = (torch.zeros(1 << 20, dtype=torch.uint8), 4096)
    with pytest.raises(RuntimeError):
        ops.raster_views_backward(*args, cams, 16, 16, g, state)
    with pytest.raises(RuntimeError):
        autograd.raster_views(*args, cams, 16, 16, background=(1.0, 1.0, 1.0))
    with pytest.raises(RuntimeError):
        ops.raster_views(*args, cams, 16, 16, want_u8=False, want_state=True)
    for kw in (dict(scale_modifier=0.0), dict(scale_modifier=float("nan")), dict(background=(1.0, 1.0)), dict(want=()), dict(want=("xyz", "bogus"))):
        with pytest.raises(ValueError):
            ops.raster_views_backward(*args, cams, 16, 16, g, state, **kw)
    for bad in (None, (state[0],), (state[0], 0), (state[0], 1 << 31), (None, 16)):
        with pytest.raises(ValueError):
            ops.raster_views_backward(*args, cams, 16, 16, g, bad)
    for bad in (cams[:, :12], cams.reshape(-1)):
        with pytest.raises(ValueError):
            ops.raster_views_backward(*args, bad, 16, 16, g, state)
    for bad in (g[:1], g[..., :3], g.reshape(-1)):
        with pytest.raises(ValueError):
            ops.raster_views_backward(*args, cams, 16, 16, bad, state)
    with pytest.raises(ValueError):
        ops.raster_views_backward(*args, cams, 0, 16, g, state)
    for k in (1, 2, 3):
        short = list(args)
        short[k] = short[k][:5]
        with pytest.raises(ValueError):
            ops.raster_views_backward(*short, cams, 16, 16, g, state)
    with pytest.raises(ValueError):
        autograd.raster_views(*args, cams, 16, 16, background=(1.0, 1.0))
    with pytest.raises(TypeError):
        autograd.raster_views(*args, cams, 16, 16)                          # background is required
    if os.path.exists(importlib.import_module("6dgs_amd._lib").LIB_PATH):
        assert ops.raster_views_backward_workspace_bytes(1000, 2, 64, 48, 5000) > ops.raster_views_backward_workspace_bytes(1000, 1, 64, 48, 5000) > 0


def test_hand_worked_gradients():
    """One isotropic Gaussian (sigma 0.2 at z = 2) in front of an identity camera with f = 20, opacity logit 0: at pixel (16, 16)
    d = (-0.5, -0.5), the variance is (0.2 * 20 / 2)^2 + 0.3 = 4.3 and alpha = 0.5 exp(-0.25 / 4.3).  The alpha channel there is alpha,
    so d / d opacity = sigmoid'(0) exp(-0.25 / 4.3); the red channel is (C0 f_dc + 0.5) alpha, so d / d f_dc = C0 alpha."""
    row = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 16.0, 16.0]], np.float32)
    scene = {"xyz": np.array([[0.0, 0.0, 2.0]], np.float32), "log_scale": np.log(np.full((1, 3), 0.2, np.float32)),
             "rot": np.array([[1.0, 0, 0, 0]], np.float32), "opacity": np.array([[0.0]], np.float32),
             "f_dc": np.zeros((1, 1, 3), np.float32), "f_rest": np.zeros((1, 15, 3), np.float32), "sh_degree": 3}
    e = np.exp(-0.25 / 4.3)
    g = np.zeros((1, 32, 32, 4), np.float32)
    g[0, 16, 16, 3] = 1
    r = RB.gradients(scene, row, 32, 32, np.float64, g, background=(0.0, 0.0, 0.0))
    # 1e-7: log(0.2) reaches the restatement rounded to fp32, which moves the variance by 1e-7 relative
    assert abs(r["opacity"][0, 0] - 0.25 * e) < 1e-7 and not r["f_dc"].any() and not r["f_rest"].any()
    # d alpha / d u = alpha d power / d u = alpha (-(1 / 4.3) (-0.5)), and cx, cy enter through u, v alone
    assert abs(r["cams"][0, 14] - 0.5 * e * 0.5 / 4.3) < 1e-7 and abs(r["cams"][0, 15] - 0.5 * e * 0.5 / 4.3) < 1e-7
    g[:] = 0
    g[0, 16, 16, 0] = 1
    r = RB.gradients(scene, row, 32, 32, np.float64, g, background=(0.0, 0.0, 0.0))
    assert abs(r["f_dc"][0, 0, 0] - 0.28209479177387814 * 0.5 * e) < 1e-7 and not r["f_dc"][0, 0, 1:].any()
    assert abs(r["opacity"][0, 0] - 0.5 * 0.25 * e) < 1e-7                  # the red channel is 0.5 alpha


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", RB.CASES)
def test_the_restatement_is_the_image_and_the_bounds_stay_under_the_ceiling(syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """From the restatement alone: its fp64 image is raster_reference's to 1e-12; at most 0.2 % of the pixels lose their loss weight;
    per gradient array max(8 y, 1e-6 scale) <= 1e-4 scale, y = max |fp32 - fp64|, scale = max |fp64|."""
    assert (n, scene_seed, views, cam_seed, width, height, sh_degree) in RR.CASES
    c = RB.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    assert np.abs(c["g64"]["image"] - c["rr"]["r64"]["image"]).max() <= 1e-12
    share = c["rr"]["undecidable"].mean()
    assert share <= RR.MAX_UNDECIDABLE_SHARE and not c["g"][c["rr"]["undecidable"]].any() and c["g"].dtype == np.float32
    for k, (scale, y, limit) in c["bounds"].items():
        print(f"n={n} {width}x{height} deg={sh_degree} {k}: scale {scale:.3e}, y / scale {y / scale if scale else 0:.2e}, "
              f"bound / scale {limit / scale if scale else 0:.2e}; zeroed pixels {share:.5f}")
        if k == "f_rest" and sh_degree == 0:
            assert c["g64"][k].size == 0
            continue
        assert scale > 0 and limit == max(RB.FACTOR * y, RB.FLOOR * scale) and limit <= RB.CEILING * scale, k
    assert RB.FACTOR == 8.0 and RB.FLOOR == 1e-6 and RB.CEILING == 1e-4
