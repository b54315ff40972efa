"""The photometric loss (sixdgs_photometric_loss) and the pose refiner without a GPU: the entry points in the header, the binding and
the library; the answers that need no device; the torch restatement (tests/photometric_reference.py) against the reference's stored
values (tests/golden/g14_photometric.npz), on closed forms and on the properties the GPU test relies on; refine.compose and the
target's downscaling on values worked by hand; the refusals of ops.photometric_loss and refine_poses; the sweep's flags."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photometric_reference as PR  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_photometric_loss", "sixdgs_photometric_loss_workspace_bytes")
# max |fp64 restatement - reference| / scale over the four pairs, as tools/gen_photometric_golden.py printed it: l1 0, ssim 1.54e-6,
# loss 8.06e-8, gradient 2.89e-7 (the reference's window is normalised and multiplied out in fp32).  The bound is 8 x that; where
# the two agreed to the last bit, 1e-12 of the scale for the fp64 sums' own rounding.
GOLDEN_MEASURED = {"l1": 0.0, "ssim": 1.54e-6, "loss": 8.06e-8, "grad": 2.89e-7}
GOLDEN_BOUND = {k: max(8.0 * v, 1e-12) for k, v in GOLDEN_MEASURED.items()}


def _call(L, **kw):
    """sixdgs_photometric_loss on (never dereferenced) non-NULL addresses; kw overrides.  Every call made here ends in a refusal or
    has nothing to do, so nothing is launched."""
    a = dict(image=256, image_stride=4, target=256, is_u8=0, target_stride=3, views=1, width=8, height=8, lam=0.2, grad_loss=None,
             loss=256, parts=None, grad_image=None, ws=None, ws_bytes=0)
    a.update(kw)
    return L.sixdgs_photometric_loss(a["image"], a["image_stride"], a["target"], a["is_u8"], a["target_stride"], a["views"], a["width"],
                                     a["height"], a["lam"], a["grad_loss"], a["loss"], a["parts"], a["grad_image"], a["ws"], a["ws_bytes"],
                                     None, None)


def test_entry_points_in_header_binding_and_library():
    ge = importlib.import_module("__graft_entry__")
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "photometric.hip" in build.SOURCES
    assert ge.header_abi_version() == 10 == lib.ABI_VERSION
    assert len(lib.SIGNATURES["sixdgs_photometric_loss"][1]) == 17 and len(lib.SIGNATURES["sixdgs_photometric_loss_workspace_bytes"][1]) == 4
    so = C.CDLL(lib.LIB_PATH)                                              # a missing build fails here, it does not pass
    for name in NAMES:
        assert hasattr(so, name), f"{name} is not exported by the library"
    L = lib.load()
    assert L.sixdgs_abi_version() == 10
    ws = L.sixdgs_photometric_loss_workspace_bytes
    # positive, monotone in every size and in want_grad; 8 B per tile, 36 B per pixel with the gradient
    assert ws(1, 1, 1, 0) > 0 and ws(1, 1, 1, 1) > ws(1, 1, 1, 0)
    assert ws(2, 64, 48, 0) >= 2 * 4 * 3 * 8 and ws(2, 64, 48, 1) >= ws(2, 64, 48, 0) + 36 * 2 * 64 * 48
    assert ws(4, 640, 480, 0) > ws(2, 640, 480, 0) > ws(2, 320, 480, 0) > ws(2, 320, 240, 0)
    assert ws(4, 64, 48, 1) > ws(2, 64, 48, 1) > ws(2, 32, 48, 1) > ws(2, 32, 24, 1)
    assert ws(0, 8, 8, 1) >= 0
    for bad in ((-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385), (65535, 16384, 16384)):   # the last: views gx gy >= 2^31
        assert ws(*bad, 0) == 0 and ws(*bad, 1) == 0, bad
    assert ws(1, 16384, 16384, 1) > 36 * 16384 * 16384
    for bad in (dict(image_stride=2), dict(image_stride=5), dict(target_stride=2), dict(target_stride=5), dict(is_u8=1, target_stride=4),
                dict(is_u8=2), dict(views=-1), dict(views=65536), dict(width=0), dict(height=0), dict(width=16385), dict(height=20000),
                dict(views=65535, width=16384, height=16384), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(image=None), dict(target=None), dict(image=258), dict(target=257), dict(loss=130), dict(parts=129), dict(grad_image=2),
                dict(grad_loss=1)):
        assert _call(L, **bad) == -1, bad
    assert _call(L, is_u8=1, target=257, ws_bytes=0) == -2                 # a byte target needs no alignment; then the workspace is too small
    assert _call(L, views=0) == 0 and _call(L, views=0, image=None, target=None) == 0      # no views: nothing to do
    assert _call(L, loss=None) == 0                                        # nothing asked for
    small, big = ws(1, 8, 8, 0), ws(1, 8, 8, 1)
    assert _call(L, ws_bytes=small - 1, ws=256) == -2                      # SIXDGS_E_WORKSPACE
    assert _call(L, ws_bytes=small, grad_image=256, ws=256) == -2          # the gradient needs the larger one
    assert _call(L, ws_bytes=big - 1, grad_image=256, ws=256) == -2
    assert _call(L, ws_bytes=small) == -1 and _call(L, ws_bytes=big, grad_image=256) == -1          # NULL ws
    assert _call(L, ws_bytes=small, ws=128) == -1 and _call(L, ws_bytes=big, grad_image=256, ws=128) == -1        # misaligned ws


def test_the_header_window_is_the_fp32_rounding_of_the_fp64_gaussian():
    text = open(os.path.join(ROOT, "include", "sixdgs.h")).read()
    body = re.search(r"#define\s+SIXDGS_SSIM_WINDOW(.*?)\}", text, re.S).group(1)
    taps = np.array([np.float32(t) for t in re.findall(r"([0-9.eE+-]+)f", body)], np.float32)
    assert taps.shape == (11,) and np.array_equal(taps, PR.WINDOW) and np.array_equal(taps, taps[::-1])
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    assert np.array_equal(PR.WINDOW, (g / g.sum()).astype(np.float32)) and abs(float(PR.WINDOW64.sum()) - 1.0) < 1e-15


def test_the_restatement_agrees_with_the_reference(golden):
    g = golden("g14_photometric")
    assert list(g["names"]) == ["r5x7", "r16x16", "r33x17", "shift24x40"]
    for name in g["names"]:
        image, target = g[f"{name}_image"], g[f"{name}_target"]
        assert image.dtype == np.float32 and image.shape == target.shape and image.shape[2] == 3
        r = PR.evaluate(image[None], target[None], 0.2, np.float64)
        got = {"l1": r["parts"][0, 0], "ssim": r["parts"][0, 1], "loss": r["loss"][0], "grad": r["grad"][0]}
        for k, v in got.items():
            ref = g[f"{name}_{k}"]
            err, scale = float(np.abs(v - ref).max()), float(np.abs(ref).max())
            print(f"{name} {k}: {err / scale:.2e} of the scale (bound {GOLDEN_BOUND[k]:.2e})")
            assert err <= GOLDEN_BOUND[k] * scale, (name, k)
    assert max(GOLDEN_BOUND.values()) <= 1e-5 * 8                          # more than 1e-5 measured would mean a wrong restatement
    assert max(GOLDEN_MEASURED.values()) <= 1e-5
    big = g["shift24x40_image"]
    assert np.array_equal(big[:-2, :-3], g["shift24x40_target"][2:, 3:])   # the target is the image moved by (2, 3)


def test_the_two_pass_gradient_is_the_derivative():
    x = PR.inputs(2, 17, 33)
    for lam in PR.LAMBDAS:
        lam32 = float(np.float32(lam))
        auto = PR.autograd_gradient(x["image"], x["target_f"], lam32)
        two = PR.evaluate(x["image"], x["target_f"], lam, np.float64)["grad"]
        assert np.abs(auto - two).max() <= 1e-12 * max(np.abs(auto).max(), 1e-30), lam


def test_a_single_pixel_has_a_closed_form():
    """1 x 1: every blur is w[5]^2 times the value."""
    a, b = np.float32(0.3), np.float32(0.85)
    k = float(PR.WINDOW[5]) ** 2
    mu1, mu2 = k * float(a), k * float(b)
    s1, s2, s12 = k * float(a) ** 2 - mu1 ** 2, k * float(b) ** 2 - mu2 ** 2, k * float(a) * float(b) - mu1 * mu2
    c1, c2 = float(np.float32(1e-4)), float(np.float32(9e-4))
    m = (2 * mu1 * mu2 + c1) * (2 * s12 + c2) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))
    image, target = np.full((1, 1, 1, 3), a, np.float32), np.full((1, 1, 1, 3), b, np.float32)
    r = PR.evaluate(image, target, 0.2, np.float64)
    lam = float(np.float32(0.2))
    assert abs(r["parts"][0, 1] - m) < 1e-13 and abs(r["parts"][0, 0] - (float(b) - float(a))) < 1e-13
    assert abs(r["loss"][0] - ((1 - lam) * (float(b) - float(a)) + lam * (1 - m))) < 1e-13
    # d m / d a by a central difference of the closed form
    def m_of(t):
        u1 = k * t
        v1, v12 = k * t * t - u1 * u1, k * t * float(b) - u1 * mu2
        return (2 * u1 * mu2 + c1) * (2 * v12 + c2) / ((u1 * u1 + mu2 ** 2 + c1) * (v1 + s2 + c2))
    h = 1e-6
    dm = (m_of(float(a) + h) - m_of(float(a) - h)) / (2 * h)
    assert np.allclose(r["grad"][0, 0, 0], ((1 - lam) * -1.0 - lam * dm) / 3.0, rtol=0, atol=1e-8)


def test_equal_images_at_lambda_zero_give_exact_zeros():
    x = PR.inputs(2, 17, 33)
    for dtype in (np.float64, np.float32):
        r = PR.evaluate(x["image"], x["image"], 0.0, dtype)
        assert not r["loss"].any() and not r["grad"].any() and not r["parts"][:, 0].any()
        assert np.abs(r["parts"][:, 1] - 1).max() < 1e-5


@pytest.mark.parametrize("views,height,width", PR.CASES)
def test_every_parity_case_is_fit_under_the_ceiling(views, height, width):
    for lam in PR.LAMBDAS:
        for u8 in (False, True):
            for with_gl in (False, True):
                c = PR.case(views, height, width, lam, u8, with_gl)
                for k, (scale, y, limit) in c["bounds"].items():
                    if k == "grad" and lam == 0.0:            # +-(1 / n): the fp32 restatement has it to the last bit or nearly
                        assert y <= 1e-7 * scale
                    assert scale > 0 and limit == max(PR.FACTOR * y, PR.FLOOR * scale) and limit <= PR.CEILING * scale, (lam, u8, with_gl, k)
    assert PR.FACTOR == 8.0 and PR.FLOOR == 1e-6 and PR.CEILING == 1e-4


def test_compose_on_values_worked_by_hand():
    refine = importlib.import_module("6dgs_amd.refine")
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    row = torch.from_numpy(np.concatenate([np.concatenate([q, rng.standard_normal((3, 1))], 1).reshape(-1), [50.0, 60.0, 16.0, 12.0]]).astype(np.float32))
    assert torch.equal(refine.compose(row, torch.zeros(6)), row)                           # delta = 0 is the row itself
    moved = refine.compose(row, torch.tensor([0.5, -0.25, 2.0, 0, 0, 0]))
    want = row.clone()
    want[3], want[7], want[11] = row[3] + 0.5, row[7] - 0.25, row[11] + 2.0                # a pure translation adds to t alone
    assert torch.equal(moved, want)
    # 90 degrees about z after the identity camera with t = (1, 2, 3): dR = [[0, -1, 0], [1, 0, 0], [0, 0, 1]], so R' = dR, t' = (-2, 1, 3)
    ident = torch.tensor([1.0, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3, 7, 8, 9, 10])
    turned = refine.compose(ident, torch.tensor([0, 0, 0, 0, 0, np.pi / 2], dtype=torch.float32))
    want = torch.tensor([0.0, -1, 0, -2, 1, 0, 0, 1, 0, 0, 1, 3, 7, 8, 9, 10])
    assert (turned - want).abs().max() < 1e-6
    # batched: each row as alone
    rows, deltas = torch.stack([row, ident]), torch.tensor([[0.1, 0.2, 0.3, 0.02, -0.01, 0.03], [0, 0, 0, 0, 0, np.pi / 2]], dtype=torch.float32)
    both = refine.compose(rows, deltas)
    assert torch.equal(both[0], refine.compose(row, deltas[0])) and torch.equal(both[1], turned)
    r = refine.rodrigues(deltas[0, 3:]).double()
    assert (r @ r.T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6 and abs(float(torch.linalg.det(r)) - 1) < 1e-6
    # differentiable at 0
    d = torch.zeros(6, requires_grad=True)
    refine.compose(row, d).sum().backward()
    assert bool(torch.isfinite(d.grad).all()) and bool(d.grad.abs().sum() > 0)


def test_downscaling_of_image_and_intrinsics():
    refine = importlib.import_module("6dgs_amd.refine")
    img = torch.arange(2 * 5 * 7 * 4, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 5, 7, 4)
    same, ox, oy = refine.prepare_target(img, 1)
    assert same.dtype == torch.uint8 and torch.equal(same, img[..., :3]) and same.is_contiguous() and (ox, oy) == (0, 0)
    # 5 x 7 by 2: a 4 x 6 crop that starts at (x, y) = (0, 0) ((7 mod 2) // 2 = 0), 2 x 3 blocks of 2 x 2
    t, ox, oy = refine.prepare_target(img, 2)
    assert t.shape == (2, 2, 3, 3) and t.dtype == torch.float32 and (ox, oy) == (0, 0)
    f = img.float() / 255.0
    want = (f[1, 2, 4, 1] + f[1, 2, 5, 1] + f[1, 3, 4, 1] + f[1, 3, 5, 1]) / 4
    assert abs(float(t[1, 1, 2, 1]) - float(want)) < 1e-6
    # 5 x 7 by 3: a 3 x 6 crop that starts at (0, 1) -> one row of two 3 x 3 blocks
    t, ox, oy = refine.prepare_target(img, 3)
    assert t.shape == (2, 1, 2, 3) and (ox, oy) == (0, 1)
    assert abs(float(t[0, 0, 1, 2]) - float(f[0, 1:4, 3:6, 2].mean())) < 1e-6
    t, ox, oy = refine.prepare_target(img[:, :, :5], 3)                  # 5 x 5 by 3: the crop starts at (1, 1)
    assert t.shape == (2, 1, 1, 3) and (ox, oy) == (1, 1) and abs(float(t[0, 0, 0, 0]) - float(f[0, 1:4, 1:4, 0].mean())) < 1e-6
    with pytest.raises(ValueError):
        refine.prepare_target(img, 6)
    K = torch.tensor([[100.0, 0, 3.5], [0, 120.0, 2.5], [0, 0, 1]])
    assert torch.equal(refine.scaled_intrinsics(K, 1, 0, 0), torch.tensor([100.0, 120.0, 3.5, 2.5]))
    assert torch.allclose(refine.scaled_intrinsics(K, 2, 0, 0), torch.tensor([50.0, 60.0, 1.75, 1.25]))
    assert torch.allclose(refine.scaled_intrinsics(K[None], 3, 1, 1), torch.tensor([[100 / 3, 40.0, 2.5 / 3, 0.5]]))


def test_pose_errors_of_the_refiner_are_the_kernel_formulas():
    refine = importlib.import_module("6dgs_amd.refine")
    gt = torch.eye(4)[None].repeat(2, 1, 1)
    pred = gt.clone()
    pred[0, :3, 3] = torch.tensor([3.0, 4.0, 0.0])
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    pred[1, :3, :3] = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float32)
    t, a = refine.pose_errors(gt, pred)
    assert abs(float(t[0]) - 5) < 1e-6 and abs(float(a[0])) < 1e-3 and abs(float(t[1])) < 1e-6 and abs(float(a[1]) - 30) < 1e-3
    pred[1, :3, :3] = 0
    assert bool(torch.isnan(refine.pose_errors(gt, pred)[1][1]))


def test_ops_and_refiner_refuse_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    ops = importlib.import_module("6dgs_amd.ops")
    autograd = importlib.import_module("6dgs_amd.autograd")
    refine = importlib.import_module("6dgs_amd.refine")
    assert pkg.photometric_loss is autograd.photometric_loss and pkg.refine_poses is refine.refine_poses
    assert {"photometric_loss", "refine_poses", "refine_results"} <= set(pkg.__all__)
    image, target = torch.zeros(2, 8, 9, 4), torch.zeros(2, 8, 9, 3)
    with pytest.raises(RuntimeError):                                     # CPU tensors: no fallback
        ops.photometric_loss(image, target)
    with pytest.raises(RuntimeError):
        autograd.photometric_loss(image, target)
    for bad in (dict(lambda_dssim=-0.1), dict(lambda_dssim=1.1), dict(lambda_dssim=float("nan")), dict(grad_loss=torch.ones(2)),
                dict(grad_loss=torch.ones(3), want_grad=True)):
        with pytest.raises(ValueError):
            ops.photometric_loss(image, target, **bad)
    for bad_image in (image.double(), image[..., :2], image[0], image.permute(0, 2, 1, 3), image[:, :, ::2], "image"):
        with pytest.raises(ValueError):
            ops.photometric_loss(bad_image, target)
    for bad_target in (target.double(), target[:1], target[:, :4], torch.zeros(2, 8, 9, 4, dtype=torch.uint8), torch.zeros(2, 8, 9, 5),
                       torch.zeros(2, 8, 9, 3, dtype=torch.int32), torch.zeros(2, 8, 9, 4)[..., :3], None):
        with pytest.raises(ValueError):
            ops.photometric_loss(image, bad_target)
    if os.path.exists(importlib.import_module("6dgs_amd._lib").LIB_PATH):
        assert ops.photometric_loss_workspace_bytes(2, 64, 48, True) > ops.photometric_loss_workspace_bytes(2, 64, 48) > 0
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    images, c2w, K = [np.zeros((8, 8, 3), np.uint8)] * 2, torch.eye(4)[None].repeat(2, 1, 1), torch.tensor([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    with pytest.raises(RuntimeError):                                     # the scene is not on the GPU
        refine.refine_poses(scene, images, c2w, K)
    for bad in (dict(steps=0), dict(steps=-3), dict(steps=2.5), dict(lr=0.0), dict(lr=float("inf")), dict(lr=float("nan")), dict(downscale=0),
                dict(downscale=1.5), dict(lambda_dssim=2.0), dict(background=(1.0, 1.0))):
        with pytest.raises(ValueError):
            refine.refine_poses(scene, images, c2w, K, **bad)
    nan_pose = c2w.clone()
    nan_pose[1, 0, 3] = float("nan")
    for bad_args in ((images, c2w[0], K), (images, c2w[:, :3], K), (images[:1], c2w, K), (images, c2w, K[:2]), (images, c2w, K[None].repeat(3, 1, 1)),
                     (images, nan_pose, K)):
        with pytest.raises(ValueError):
            refine.refine_poses(scene, *bad_args)
    with pytest.raises(ValueError):
        refine.refine_results(scene, [], [{"pred_c2w": np.eye(4).tolist()}])
    resized = type("Cam", (), {"image": np.zeros((8, 8, 3), np.uint8), "width": 16, "height": 16})()
    with pytest.raises(ValueError):                                       # the stored image is not of the camera's size
        refine.refine_results(scene, [resized], [{"pred_c2w": np.eye(4).tolist(), "gt_c2w": np.eye(4).tolist()}])


def test_refine_steps_zero_changes_nothing_in_the_sweep():
    pea = importlib.import_module("6dgs_amd.pretrain_eval_attention")
    refine = importlib.import_module("6dgs_amd.refine")
    args, rest = pea.parse_args(["--exp_path", "e", "--out_path", "o.json"])
    fields = dict(vars(args))
    new = {k: fields.pop(k) for k in list(fields) if k.startswith("refine_")}
    assert new == {"refine_steps": 0, "refine_downscale": 4, "refine_lr": 2e-3, "refine_lambda": 0.2} and rest == []
    assert fields == dict(exp_path="e", out_path="o.json", data_type="all", emitter="quadricell", max_ellipsoids=1000, rays_per_ellipsoid=64,
                          n_iterations=1500, batched_window=False, data_parallel_train=False, backward_ray_groups=1, skip_train=False,
                          batch_size=16, pose_solver="ls", inlier_scale=None, rays_to_output=100, arena_gb=0.0)
    on, _ = pea.parse_args(["--exp_path", "e", "--out_path", "o", "--refine_steps", "30", "--refine_downscale", "2", "--refine_lr", "1e-3",
                            "--refine_lambda", "0.5"])
    assert (on.refine_steps, on.refine_downscale, on.refine_lr, on.refine_lambda) == (30, 2, 1e-3, 0.5)
    for bad in (["--refine_steps", "-1"], ["--refine_downscale", "0"], ["--refine_lr", "0"], ["--refine_lambda", "1.5"]):
        with pytest.raises(SystemExit):
            pea.parse_args(["--exp_path", "e", "--out_path", "o"] + bad)
    assert inspect.signature(pea.pretrain_single_object).parameters["refine"].default is None        # off unless asked for
    # an entry without a finite pose is left exactly as it is (and nothing here needs a GPU)
    entry = {"sequence_id": "s", "category_name": "c", "frame_id": 0, "loss": 0.5, "scores_loss": 0.0, "recall": 0.0,
             "total_optimization_time_in_ms": 0.0, "pred_c2w": np.full((4, 4), np.nan).tolist(), "gt_c2w": np.eye(4).tolist()}
    cam = type("Cam", (), {"image": np.zeros((8, 8, 3), np.uint8), "width": 8, "height": 8})()
    before = {k: (v if not isinstance(v, list) else [list(r) for r in v]) for k, v in entry.items()}
    out = refine.refine_results(None, [cam], [entry])
    assert list(out[0]) == list(before) and str(out[0]) == str(before)
    # the summary's key names are new ones beside the unrefined errors
    done = dict(entry, pred_c2w=np.eye(4).tolist(), refined_c2w=np.eye(4).tolist(), refined_translation_error=0.25, refined_angular_error=0.5,
                photometric_loss_before=0.3, photometric_loss_after=0.1)
    s = pea.refine_summary([entry, done])
    assert s["views"] == 2 and s["refined_views"] == 1 and s["mean_refined_translation_error"] == 0.25 and s["median_translation_error"] == 0.0
    assert s["median_photometric_loss_after"] == 0.1 and pea.refine_summary([entry]) == {"refined_views": 0, "views": 1}
