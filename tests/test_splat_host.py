"""Synthetic query views (sixdgs_splat_views, ABI 10) without a GPU: the entry points in the header, the binding and the library;
the refusals of ops.splat_views and render_views; and the fp64 restatement of the image definition (tests/splat_reference.py) on the
property the GPU test relies on -- that fp32 rounding can change the winner of at most 0.1 % of the pixels of its cases."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_reference as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_splat_views", "sixdgs_splat_views_workspace_bytes")


def test_splat_entry_points_in_header_binding_and_library():
    ge = importlib.import_module("__graft_entry__")
    lib = importlib.import_module("6dgs_amd._lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert ge.header_abi_version() == 10 == lib.ABI_VERSION
    assert len(lib.SIGNATURES["sixdgs_splat_views"][1]) == 21
    if os.path.exists(lib.LIB_PATH):
        so = C.CDLL(lib.LIB_PATH)
        for name in NAMES:
            assert hasattr(so, name), f"{name} is not exported by the library"
        L = lib.load()
        assert L.sixdgs_abi_version() == 10
        # sizes and argument errors are answered without touching the GPU
        ws = L.sixdgs_splat_views_workspace_bytes
        assert ws(1000, 2, 64, 48) >= 2 * 64 * 48 * 8 + 2 * 1000 * 4
        assert ws(1000, 4, 64, 48) >= ws(1000, 2, 64, 48) and ws(0, 1, 8, 8) >= 8 * 8 * 8
        call = L.sixdgs_splat_views
        nul = None
        assert call(nul, nul, 1, nul, nul, 3, 16, 0, nul, 1, 8, 8, 5, 1.0, 0.05, nul, nul, nul, nul, 0, nul) == -1      # channels
        assert call(nul, nul, 1, nul, nul, 3, 16, 0, nul, 1, 8, 8, 3, 0.0, 0.05, nul, nul, nul, nul, 0, nul) == -1      # extent
        assert call(nul, nul, 1, nul, nul, 3, 16, 0, nul, 1, 0, 8, 3, 1.0, 0.05, nul, nul, nul, nul, 0, nul) == -1      # width
        assert call(nul, nul, 1, nul, nul, 3, 9, 0, nul, 1, 8, 8, 3, 1.0, 0.05, nul, nul, nul, nul, 0, nul) == -1       # n_coef < (deg + 1)^2
        assert call(nul, nul, 1, nul, nul, 3, 16, 0, nul, 1, 8, 8, 3, 1.0, 0.05, nul, nul, nul, nul, 0, nul) == -1      # NULL cams / image
        assert call(nul, nul, 1, nul, nul, 3, 16, 0, nul, 0, 8, 8, 3, 1.0, 0.05, nul, nul, nul, nul, 0, nul) == 0       # no views: nothing to do


def test_splat_views_refuses_cpu_tensors_and_bad_arguments(syn):
    ops = importlib.import_module("6dgs_amd.ops")
    sc = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_scene(10, 0).items()}
    cams = torch.from_numpy(SR.camera_rows(syn.make_cameras(2, 0, width=16, height=16)))
    args = (sc["xyz"], sc["log_scale"], sc["f_dc"], sc["f_rest"], 3)
    with pytest.raises(RuntimeError):
        ops.splat_views(*args, cams, 16, 16)
    for kw in (dict(channels=2), dict(channels=5), dict(extent=0.0), dict(extent=-1.0), dict(extent=float("nan")), dict(near_z=-0.1),
               dict(background=(1.0, 1.0))):
        with pytest.raises(ValueError):
            ops.splat_views(*args, cams, 16, 16, **kw)
    for bad in (cams[:, :12], cams.reshape(-1), cams[None]):
        with pytest.raises(ValueError):
            ops.splat_views(*args, bad, 16, 16)
    with pytest.raises(ValueError):
        ops.splat_views(*args, cams, 0, 16)
    with pytest.raises(ValueError):
        ops.splat_views(sc["xyz"], sc["log_scale"][:5], sc["f_dc"], sc["f_rest"], 3, cams, 16, 16)


def test_render_views_refuses_cpu_scenes_and_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    assert pkg.render_views is importlib.import_module("6dgs_amd.render").render_views
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    cams = syn.make_cameras(2, 0, width=16, height=16)
    with pytest.raises(RuntimeError):
        pkg.render_views(scene, cams)
    with pytest.raises(RuntimeError):
        pkg.render_views(scene, [pkg.CameraInfo(**c) for c in cams], rgba=True)
    for kw in (dict(extent=0.0), dict(extent=-2.0), dict(near_z=-1.0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            pkg.render_views(scene, cams, **kw)
    with pytest.raises(ValueError):
        pkg.render_views(scene, [dict(cams[0], R=np.eye(4))])


def test_camera_rows_are_the_camera_of_gt_pose_and_intrinsics(syn):
    """render.camera_rows against test.gt_pose_and_intrinsics (the pose the loss and the error metrics use) and against the test tree's own."""
    pkg = importlib.import_module("6dgs_amd")
    render = importlib.import_module("6dgs_amd.render")
    T = importlib.import_module("6dgs_amd.test")
    cams = syn.make_cameras(3, 11, width=160, height=120)
    for c, t in zip(cams, (np.array([0.3, -0.2, 4.0]), np.array([0.0, 0.0, 3.0]), np.array([-1.0, 0.5, 5.0]))):
        c["T"] = t
    rows = render.camera_rows(cams)
    assert rows.dtype == np.float32 and rows.shape == (3, 16)
    assert np.array_equal(rows, SR.camera_rows(cams))
    assert np.array_equal(rows, render.camera_rows([pkg.CameraInfo(**c) for c in cams]))
    for c, row in zip(cams, rows):
        c2w, K = T.gt_pose_and_intrinsics(pkg.CameraInfo(**c), "cpu")
        w2c = np.linalg.inv(c2w.double().numpy())
        assert np.abs(w2c[:3] - row[:12].reshape(3, 4)).max() < 1e-6
        assert np.allclose([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], row[12:], rtol=1e-6)
        assert np.abs(SR.camera_centre(row) - c2w[:3, 3].double().numpy()).max() < 1e-5


def test_restatement_on_a_hand_made_scene():
    """Winners that can be worked out by hand: depth order, the index rule at equal depth, near_z, the radius floor, the frame."""
    row = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 10.0, 10.0, 8.0, 8.0], np.float32)       # identity pose, f = 10, 16 x 16
    xyz = np.array([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [0.5, 0.5, 0.01], [0, 0, -1.0], [-0.75, -0.75, 1.0], [30.0, 0, 1.0]], np.float32)
    s = np.log(np.array([[0.8] * 3, [0.2] * 3, [0.2] * 3, [0.5] * 3, [0.5] * 3, [1e-4] * 3, [0.3] * 3], np.float32))
    win, und = SR.reference_view(xyz, s, row, 16, 16)
    assert win[8, 8] == 1 and und[8, 8]                       # 1 and 2 coincide: the smaller index; the depth tie makes it undecidable
    assert win[8, 10] == 0 and win[8, 12] == -1               # r(1) = 2, r(0) = 4: pixel 10 (centre 10.5) is outside disc 1 and inside disc 0
    assert win[0, 0] == 5 and win[0, 1] == -1 and win[1, 0] == -1   # a tiny Gaussian owns exactly the pixel of its centre (u = v = 0.5)
    assert not np.isin(win, (3, 4, 6)).any()                  # nearer than near_z, behind the camera, outside the frame
    assert (win >= 0).sum() == (win == 0).sum() + (win == 1).sum() + 1


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height", SR.WINNER_CASES)
def test_undecidable_pixels_stay_under_the_cap(syn, n, scene_seed, views, cam_seed, width, height):
    """The cases of tests/test_gpu_splat.py: at most 0.1 % of the pixels may be undecidable, or 'identical on the decidable pixels'
    would say little.  Also: the scenes fill a good part of the frame."""
    sc = syn.make_scene(n, scene_seed)
    rows = SR.camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height))
    win, und = SR.reference_views(sc, rows, width, height)
    share, covered = und.mean(), (win >= 0).mean()
    print(f"n={n} {width}x{height} views={views}: covered {covered:.3f}, undecidable {share:.5f}")
    assert share <= SR.MAX_UNDECIDABLE_SHARE, share
    assert covered > 0.4, covered
