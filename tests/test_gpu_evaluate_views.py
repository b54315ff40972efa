"""sixdgs_evaluate_views and what stands on it, on a scene of 300 Gaussians with 5 views of 40 x 24: the chunked call against the
rasteriser followed by sixdgs_image_metrics, bit for bit and for every chunk size; a capacity too small for one chunk; evaluate_views
on a scene's own renders; fit_scene(evaluate=...) for both backends with and without densification, which must leave the fit's every
bit alone; and tools/evaluate_scene.py's two files.  Everything runs inside this process."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ATTR = {"xyz": "_xyz", "scale": "_scaling", "rot": "_rotation", "opacity": "_opacity", "f_dc": "_features_dc", "f_rest": "_features_rest"}
N, VIEWS, WIDTH, HEIGHT = 300, 5, 40, 24
STEPS, AT = 12, (0, 5, 12)
DENSIFY = dict(from_iter=2, interval=4, grad_threshold=1e-3)          # rounds at iterations 4, 8 and 12: inside the run, one on a cut's eve
KEYS = ("l1", "ssim", "psnr", "psnr_channels")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def fixture(pkg, syn):
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(N, 0), device="cuda")
    views = render.render_views(scene, syn.make_cameras(VIEWS, 21, width=WIDTH, height=HEIGHT), renderer="raster")
    c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
    rows = torch.from_numpy(render.camera_rows(views)).cuda()
    images = [np.ascontiguousarray(v.image[..., :3]) for v in views]
    moved = pkg.GaussianScene(scene.max_sh_degree)
    gen = torch.Generator().manual_seed(3)
    for k, a in ATTR.items():
        t = getattr(scene, a).clone()
        if k in ("f_dc", "opacity"):
            t += (0.3 * torch.randn(t.shape, generator=gen)).cuda()
        setattr(moved, a, t)
    arrays = [getattr(moved, a).detach().float().contiguous() for a in ATTR.values()]
    x = MR.inputs(VIEWS, HEIGHT, WIDTH)
    return dict(scene=scene, moved=moved, arrays=arrays, images=images, c2w=torch.stack(c2w), K=torch.stack(Ks), rows=rows,
                targets={"u8": torch.from_numpy(np.stack(images)).cuda().contiguous(), "f4": torch.from_numpy(x["target_f"]).cuda(),
                         "f3": torch.from_numpy(np.ascontiguousarray(x["target_f"][..., :3])).cuda()})


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def by_hand(ops, f, target, quantise, sh_degree=3, width=WIDTH, height=HEIGHT, **raster):
    """ops.raster_views followed by ops.image_metrics, one view at a time; raster: scale_modifier, scale_is_log and opacity_is_logit."""
    rows, renders = [], []
    for v in range(f["rows"].shape[0]):
        image = ops.raster_views(*f["arrays"], sh_degree, f["rows"][v:v + 1].contiguous(), width, height, want_float=True, want_u8=False, **raster)
        m, r = ops.image_metrics(image, target[v:v + 1].contiguous(), quantise=quantise, want_render=True)
        rows.append(m)
        renders.append(r)
    return torch.cat(rows), torch.cat(renders)


def test_every_chunk_size_gives_the_parts_bytes(ops, fixture):
    f = fixture
    for kind, target in f["targets"].items():
        for quantise in (False, True):
            want, want_render = by_hand(ops, f, target, quantise)
            assert bool(torch.isfinite(want).all()) and bool((want[:, 2] > 0).all())
            for chunk in (1, 2, 5, 8):
                out = ops.evaluate_views_raw(*f["arrays"], 3, f["rows"], WIDTH, HEIGHT, target, quantise=quantise, chunk=chunk, want_render=True)
                assert same(out["metrics"], want) and torch.equal(out["render"], want_render), (kind, quantise, chunk)
                assert int(out["status"]) == 0 and 0 < out["instances_needed"] <= out["max_instances"]
    empty = ops.evaluate_views_raw(*f["arrays"], 3, f["rows"][:0], WIDTH, HEIGHT, f["targets"]["u8"][:0], quantise=True)
    assert empty["metrics"].shape == (0, 6) and int(empty["status"]) == 0


def test_a_capacity_too_small_for_one_chunk(ops, fixture):
    f = fixture
    target = f["targets"]["u8"]
    want, _ = by_hand(ops, f, target, True)
    chunks = [(0, 2), (2, 4), (4, 5)]
    needs = [ops.raster_views(*f["arrays"], 3, f["rows"][a:b].contiguous(), WIDTH, HEIGHT, want_u8=False, want_instances=True) for a, b in chunks]
    cap = sorted(needs)[1]
    over = [n > cap for n in needs]
    print(f"instances per chunk {needs}, capacity {cap}")
    assert any(over) and not all(over)
    out = ops.evaluate_views_raw(*f["arrays"], 3, f["rows"], WIDTH, HEIGHT, target, quantise=True, chunk=2, max_instances=cap, retry=False)
    assert int(out["status"]) == ops.EVALUATE_STATUS_CAPACITY and out["instances_needed"] == max(needs) and out["max_instances"] == cap
    for (a, b), o in zip(chunks, over):
        assert bool(torch.isnan(out["metrics"][a:b]).all()) if o else same(out["metrics"][a:b], want[a:b]), (a, b)
    # the wrapper's one retry, with exactly what was needed
    full = ops.evaluate_views_raw(*f["arrays"], 3, f["rows"], WIDTH, HEIGHT, target, quantise=True, chunk=2, max_instances=cap)
    assert same(full["metrics"], want) and int(full["status"]) == 0 and full["max_instances"] == full["instances_needed"] == max(needs)


def test_evaluate_views_and_a_scenes_own_renders(pkg, ops, fixture):
    f = fixture
    r = pkg.evaluate_views(f["moved"], f["images"], f["c2w"], f["K"], quantise=True, chunk=2, return_renders=True)
    assert set(r) == {"l1", "ssim", "mse", "psnr", "psnr_channels", "mean_l1", "mean_ssim", "mean_mse", "mean_psnr", "mean_psnr_channels",
                      "status", "renders"}
    assert all(r[k].shape == (VIEWS,) and r[k].dtype == np.float32 for k in ("l1", "ssim", "mse", "psnr", "psnr_channels")) and r["status"] == 0
    assert r["renders"].shape == (VIEWS, HEIGHT, WIDTH, 3) and r["renders"].dtype == torch.uint8 and r["renders"].is_cuda
    # the numbers are the raw call's on the prepared views, the PSNRs derived as the restatement derives them
    refine = importlib.import_module("6dgs_amd.refine")
    target, rows, width, height = refine.posed_views(f["images"], *refine.check_poses(f["images"], f["c2w"], f["K"], min_views=1), "cuda", 1, "ignore",
                                                     (1.0, 1.0, 1.0))
    raw = ops.evaluate_views_raw(*f["arrays"], 3, rows, width, height, target, quantise=True, chunk=5)["metrics"].cpu().numpy()
    assert np.array_equal(r["l1"], raw[:, 0]) and np.array_equal(r["ssim"], raw[:, 1]) and np.array_equal(r["mse"], raw[:, 2])
    assert np.array_equal(r["psnr"], MR.psnr(raw[:, 2])) and np.array_equal(r["psnr_channels"], MR.psnr_channels(raw[:, 3:6]))
    assert r["mean_psnr"] == np.float32(torch.tensor(r["psnr"]).mean().item()) and bool((r["mse"] > 0).all())
    # against its own renders the 8-bit comparison is exact: mse 0, PSNR +inf; every SSIM term is x / x, so SSIM is 1 within the
    # bound rule's floor of 1e-6
    own = pkg.evaluate_views(f["moved"], list(r["renders"].cpu().numpy()), f["c2w"], f["K"], quantise=True)
    print(f"own renders: ssim - 1 {(own['ssim'].astype(np.float64) - 1.0).tolist()}")
    assert not own["mse"].any() and not own["l1"].any() and np.isposinf(own["psnr"]).all() and np.isposinf(own["psnr_channels"]).all()
    assert np.isposinf(own["mean_psnr"]) and np.abs(own["ssim"].astype(np.float64) - 1.0).max() <= 1e-6
    # training_report's definition on the same views: other numbers, and no view scores above the 8-bit comparison's perfect
    clamp = pkg.evaluate_views(f["moved"], f["images"], f["c2w"], f["K"], quantise=False)
    assert np.isfinite(clamp["psnr"]).all() and not np.array_equal(clamp["mse"], r["mse"])
    with pytest.raises(ValueError):
        pkg.evaluate_views(f["moved"], f["images"], f["c2w"], f["K"], chunk=0)
    with pytest.raises(ValueError):
        pkg.evaluate_views(f["moved"], f["images"], f["c2w"], f["K"], sh_degree=4)


@pytest.fixture(scope="module")
def fits(pkg, fixture):
    """Every run of fit_scene with and without evaluate=: train on views 0 .. 2, measure on views 3 and 4."""
    f = fixture
    held = dict(images=f["images"][3:], c2w=f["c2w"][3:], intrinsics=f["K"][3:], at=AT)
    out = {}
    for backend in ("torch", "fused"):
        for densify in (None, DENSIFY):
            kw = dict(steps=STEPS, backend=backend, densify=densify)
            plain = pkg.fit_scene(f["moved"], f["images"][:3], f["c2w"][:3], f["K"][:3], **kw)
            watched = pkg.fit_scene(f["moved"], f["images"][:3], f["c2w"][:3], f["K"][:3], evaluate=held, **kw)
            out[backend, densify is not None] = (plain, watched)
    return out, held


@pytest.mark.parametrize("backend", ("torch", "fused"))
@pytest.mark.parametrize("densify", (False, True))
def test_evaluating_never_changes_the_fit(pkg, fixture, fits, backend, densify):
    f = fixture
    (scene_p, rep_p), (scene_w, rep_w) = fits[0][backend, densify]
    held = fits[1]
    assert "evaluations" not in rep_p and set(rep_w) == set(rep_p) | {"evaluations"}
    for k in rep_p:
        a, b = rep_p[k], rep_w[k]
        assert (same(a, b) if torch.is_tensor(a) and a.dtype == torch.float32 else (torch.equal(a, b) if torch.is_tensor(a) else a == b)), k
    for a in ATTR.values():
        assert same(getattr(scene_p, a), getattr(scene_w, a)), a
    assert bool(torch.isfinite(rep_w["loss_history"]).all()) and int(rep_w["status"]) == 0
    if densify:
        print(f"{backend}: rounds {rep_w['rounds'].tolist()}")
        assert rep_w["rounds"][:, 0].tolist() == [4, 8, 12]
    ev = rep_w["evaluations"]
    assert [e["step"] for e in ev] == list(AT) and all(set(e) == {"step", "n", *KEYS} for e in ev)
    assert ev[0]["n"] == N and ev[-1]["n"] == len(scene_w)
    views = dict(images=held["images"], c2w=held["c2w"], intrinsics=held["intrinsics"])
    for e, scene in ((ev[0], f["moved"]), (ev[-1], scene_w)):
        r = pkg.evaluate_views(scene, views["images"], views["c2w"], views["intrinsics"], quantise=False)
        assert all(np.float32(e[k]).view(np.int32) == np.float32(r["mean_" + k]).view(np.int32) for k in KEYS), (e, r)
    assert all(np.isfinite(e[k]) for e in ev for k in KEYS) and ev[-1]["l1"] != ev[0]["l1"]


def test_backends_agree_where_their_scenes_do(fits):
    """The two backends hold the same scene, bit for bit, only before the first update: Adam's rounding order differs from there on
    (fit.py's docstring), so only the evaluation at step 0 is asserted equal; the later ones are printed."""
    for densify in (False, True):
        t, u = fits[0]["torch", densify][1][1]["evaluations"], fits[0]["fused", densify][1][1]["evaluations"]
        assert t[0] == u[0]
        print(f"densify={densify}: psnr torch {[e['psnr'] for e in t]}, fused {[e['psnr'] for e in u]}")


def test_evaluate_argument_is_checked(pkg, fixture):
    f = fixture
    good = dict(images=f["images"][3:], c2w=f["c2w"][3:], intrinsics=f["K"][3:], at=(0,))
    for bad in (dict(good, at=(13,)), dict(good, at=()), dict(good, at=(-1,)), dict(good, extra=1), {k: v for k, v in good.items() if k != "at"},
                dict(good, c2w=f["c2w"][:1]), dict(good, chunk=0), "views"):
        with pytest.raises(ValueError):
            pkg.fit_scene(f["moved"], f["images"][:3], f["c2w"][:3], f["K"][:3], steps=STEPS, evaluate=bad)


def test_tool_writes_the_references_two_files(pkg, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    tool = importlib.import_module("evaluate_scene")
    argv = ["--standin", "--gaussians", "300", "--views", "3", "--size", "32", "--out", str(tmp_path), "--iteration", "7", "--chunk", "2",
            "--write-images", str(tmp_path / "png")]
    results, per_view = tool.main(argv)
    scene, cams = tool.standin_views(300, 3, 32, 11, 0.05)
    r = pkg.evaluate_views(scene, *tool.posed(cams), quantise=True)
    with open(tmp_path / "results.json") as fp:
        on_disk = json.load(fp)
    with open(tmp_path / "per_view.json") as fp:
        per_disk = json.load(fp)
    assert on_disk == results == {"ours_7": {"SSIM": float(r["mean_ssim"]), "PSNR": float(r["mean_psnr"])}}
    names = ["00000.png", "00001.png", "00002.png"]
    assert per_disk == per_view == {"ours_7": {"SSIM": dict(zip(names, map(float, r["ssim"]))), "PSNR": dict(zip(names, map(float, r["psnr"])))}}
    assert np.isfinite(r["psnr"]).all() and 10.0 < results["ours_7"]["PSNR"] < 60.0
    from PIL import Image
    renders = pkg.evaluate_views(scene, *tool.posed(cams), return_renders=True)["renders"].cpu().numpy()
    for i, name in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "png" / "renders" / name)), renders[i])
        assert np.array_equal(np.asarray(Image.open(tmp_path / "png" / "gt" / name)), np.asarray(cams[i].image)[..., :3])
