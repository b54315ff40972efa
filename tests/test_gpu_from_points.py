"""Points -> scene -> fit on the GPU: GaussianScene.from_points with the scales from the HIP search equals the restatement of
tests/knn_reference.py (scale within its derived bound, everything else exact, the distances themselves the brute force's bits); the
scene renders; fit_scene(backend="fused") on views of the stand-in the points were drawn from lowers the loss.  Everything runs inside
this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as K  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
N, SIZE, VIEWS, STEPS = 2000, 64, 4, 30


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def fixture(pkg, syn):
    """The stand-in, its centres with their DC colours, the scene made from them, and the brute-force distances."""
    d = syn.make_scene(N, 0)
    points = d["xyz"]
    colors = np.clip(d["f_dc"][:, 0, :] * F(K.C0) + F(0.5), 0.0, 1.0).astype(F)
    standin = pkg.GaussianScene.from_dict(d, device="cuda")
    scene = pkg.GaussianScene.from_points(points, colors)
    return dict(standin=standin, points=points, colors=colors, scene=scene, d2=K.brute_np(points))


def test_from_points_equals_the_restatement(pkg, fixture):
    f = fixture
    ops = importlib.import_module("6dgs_amd.ops")
    d2 = ops.knn_mean_dist2(f["scene"]._xyz).cpu().numpy()
    assert np.array_equal(d2.view(np.int32), f["d2"].view(np.int32))
    assert f["scene"]._xyz.is_cuda
    got, want = K.check_from_points(f["scene"], f["points"], f["colors"], f["d2"])
    cpu = pkg.GaussianScene.from_points(f["points"], f["colors"], mean_dist2=f["d2"], device="cpu")
    for k, a in (("f_dc", "_features_dc"), ("opacity", "_opacity")):             # the same elementwise fp32 arithmetic on either device
        assert np.array_equal(got[k].view(np.int32), getattr(cpu, a).numpy().view(np.int32)), k
    # the reference-named method fills an instance and keeps the rate scale
    D = importlib.import_module("6dgs_amd.datasets")
    s = pkg.GaussianScene(2).create_from_pcd(D.BasicPointCloud(f["points"].astype(np.float64), f["colors"].astype(np.float64), np.zeros((N, 3))), 2.5)
    assert s.spatial_lr_scale == 2.5 and s.active_sh_degree == 0 and s._features_rest.shape == (N, 8, 3)
    assert torch.equal(s._scaling, f["scene"]._scaling) and torch.equal(s._xyz, f["scene"]._xyz) and torch.equal(s._features_dc, f["scene"]._features_dc)


def test_scene_from_points_renders_and_fits(pkg, fixture, syn):
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    fit = importlib.import_module("6dgs_amd.fit")
    f = fixture
    cams = syn.make_cameras(VIEWS, 21, width=SIZE, height=SIZE)
    mine = render.render_views(f["scene"], cams, renderer="raster")
    for v in mine:
        im = np.asarray(v.image)
        assert im.shape[:2] == (SIZE, SIZE) and np.isfinite(im.astype(np.float64)).all()
    assert len({np.asarray(v.image).tobytes() for v in mine}) == VIEWS and np.asarray(mine[0].image).std() > 0      # something was drawn
    views = render.render_views(f["standin"], cams, renderer="raster")
    c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
    before = {k: getattr(f["scene"], k).clone() for k in ("_xyz", "_scaling", "_opacity", "_features_dc")}
    new, rep = fit.fit_scene(f["scene"], [v.image for v in views], torch.stack(c2w), torch.stack(Ks), steps=STEPS, backend="fused")
    h = rep["loss_history"].cpu().numpy()
    assert h.shape == (STEPS, 1) and np.isfinite(h).all() and int(rep["status"]) == 0 and len(new) == N
    print(f"loss: first pass over the views {h[:VIEWS].mean():.5f}, last {h[-VIEWS:].mean():.5f}")
    assert h[-VIEWS:].mean() < h[:VIEWS].mean()
    assert all(torch.equal(getattr(f["scene"], k), v) for k, v in before.items())                                   # the input is not written
