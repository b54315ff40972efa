"""sixdgs_photometric_loss on the GPU: loss, parts and gradient against the fp64 restatement (tests/photometric_reference.py) under a
bound taken from the restatement's own fp32 rounding, and against the reference's stored values; the exact facts of the definition;
determinism and batching bit for bit; guard bytes through the raw C call; the autograd function alone and chained after the
rasteriser; and the pose refiner built from the two.  Everything runs inside this process.

Measured on MI355X (profiles/photometric_loss.md): parity worst |gpu - fp64| / bound 0.31 (the 289-tile case; 0.19 below it); the chain's camera gradient 0.13 of its bound;
refinement from 0.054 units / 1.54 degrees to 0.0014 - 0.0017 units / 0.00 - 0.04 degrees in 60 steps."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photometric_reference as PR  # noqa: E402
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402
from test_photometric_host import GOLDEN_BOUND  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, c, what):
    """loss, parts, grad within their bounds of fp64 -> the largest measured / bound."""
    worst = 0.0
    for k, v in got.items():
        scale, y, limit = c["bounds"][k]
        ref = c["r64"][k]
        a = v.cpu().numpy().astype(np.float64)[..., :3] if k == "grad" else v.cpu().numpy().astype(np.float64)
        err = float(np.abs(a - ref).max())
        assert limit <= PR.CEILING * scale, f"{what} {k}: the case is unfit"
        print(f"{what} {k}: max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
        assert np.isfinite(a).all() and err <= limit, f"{what} {k}: {err:.3e} > {limit:.3e}"
        worst = max(worst, err / limit)
    return worst


@pytest.mark.parametrize("views,height,width", PR.CASES)
def test_parity_against_fp64(ops, views, height, width):
    worst = 0.0
    for lam in PR.LAMBDAS:
        for kind in ("f3", "f4", "u8"):
            for with_gl in (False, True):
                c = PR.case(views, height, width, lam, kind == "u8", with_gl)
                x = c["x"]
                target = G(x["target_u8"]) if kind == "u8" else G(x["target_f"] if kind == "f4" else x["target_f"][..., :3])
                gl = G(x["grad_loss"]) if with_gl else None
                for stride in (3, 4):
                    image = G(x["image"][..., :stride])
                    loss, grad, parts = ops.photometric_loss(image, target, lambda_dssim=lam, grad_loss=gl, want_grad=True, want_parts=True)
                    assert loss.shape == (views,) and parts.shape == (views, 2) and grad.shape == image.shape and grad.dtype == torch.float32
                    worst = max(worst, _check({"loss": loss, "parts": parts, "grad": grad}, c,
                                              f"{views}x{height}x{width} lambda={lam} {kind} stride={stride} gl={with_gl}"))
                    if stride == 4:
                        assert not bool(grad[..., 3].any())
                    # the loss alone, from the smaller workspace: the same bits
                    assert torch.equal(ops.photometric_loss(image, target, lambda_dssim=lam), loss)
    print(f"{views}x{height}x{width}: worst measured / bound {worst:.3f}")


def test_hard_images_are_held_to_eight_y(ops):
    """The smooth and the nearly flat image, where blur(a a) - mu1 mu1 cancels: no ceiling, FACTOR y alone (reported in the profile)."""
    for kind in ("smooth", "flat"):
        image, target = PR.hard_case(kind)
        r64, r32 = PR.evaluate(image, target, 0.2, np.float64), PR.evaluate(image, target, 0.2, np.float32)
        loss, grad, parts = ops.photometric_loss(G(image), G(target), want_grad=True, want_parts=True)
        for k, v in (("loss", loss), ("parts", parts), ("grad", grad)):
            scale, y, limit = PR.bounds(r64, r32)[k]
            err = float(np.abs(v.cpu().numpy().astype(np.float64) - r64[k]).max())
            print(f"{kind} {k}: |gpu - fp64| {err / scale:.2e} of the scale, restatement y {y / scale:.2e}, bound {limit / scale:.2e}")
            assert err <= limit, (kind, k)


def test_golden_against_the_reference(ops, golden):
    """|gpu - reference| within the golden bound (8 x the measured |fp64 restatement - reference|).  l1 alone gets the pair's parity
    bound added: there the restatement and the reference agreed to the last bit, the golden bound is 1e-12 of the scale, and no fp32
    sum can meet that."""
    g = golden("g14_photometric")
    for name in g["names"]:
        image, target = g[f"{name}_image"][None], g[f"{name}_target"][None]
        r64, r32 = PR.evaluate(image, target, 0.2, np.float64), PR.evaluate(image, target, 0.2, np.float32)
        loss, grad, parts = ops.photometric_loss(G(image), G(target), lambda_dssim=0.2, want_grad=True, want_parts=True)
        got = {"l1": (float(parts[0, 0]), PR.bounds(r64, r32)["parts"][2]), "ssim": (float(parts[0, 1]), 0.0), "loss": (float(loss[0]), 0.0),
               "grad": (grad[0].cpu().numpy().astype(np.float64), 0.0)}
        for k, (v, own) in got.items():
            ref = g[f"{name}_{k}"]
            err, scale = float(np.abs(v - ref).max()), float(np.abs(ref).max())
            print(f"{name} {k}: |gpu - reference| {err / scale:.2e} of the scale (bound {GOLDEN_BOUND[k] + own / scale:.2e})")
            assert err <= GOLDEN_BOUND[k] * scale + own, (name, k)


def test_exact_facts(ops):
    x = PR.inputs(3, 17, 33)
    image4, image3 = G(x["image"]), G(x["image"][..., :3])
    # lambda = 0, image == target: loss and gradient exactly 0
    for image, target in ((image4, image4.clone()), (image3, image3.clone()), (image4, image3)):
        loss, grad = ops.photometric_loss(image, target, lambda_dssim=0.0, want_grad=True)
        assert not bool(loss.any()) and not bool(grad.any())
    # a uint8 target and its fp32 u / 255 copy: the same bits
    u = G(x["target_u8"])
    f = G(PR.u8_value(x["target_u8"]))               # the correctly rounded quotient (torch's own division on the GPU is not)
    a = ops.photometric_loss(image4, u, want_grad=True, want_parts=True)
    b = ops.photometric_loss(image4, f.contiguous(), want_grad=True, want_parts=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and bool(a[1].any())
    assert not bool(a[1][..., 3].any())                                   # the stride-4 gradient's fourth channel: exact zeros
    # NaN in the alpha channel of a stride-4 image and target changes nothing
    target4 = G(x["target_f"])
    clean = ops.photometric_loss(image4, target4, want_grad=True, want_parts=True)
    dirty_i, dirty_t = image4.clone(), target4.clone()
    dirty_i[..., 3] = float("nan")
    dirty_t[..., 3] = float("nan")
    dirty = ops.photometric_loss(dirty_i, dirty_t, want_grad=True, want_parts=True)
    assert all(torch.equal(p, q) for p, q in zip(clean, dirty)) and bool(torch.isfinite(dirty[1]).all())
    # the same bytes on two calls; each view alone is its rows of the batch
    again = ops.photometric_loss(image4, target4, want_grad=True, want_parts=True)
    assert all(torch.equal(p, q) for p, q in zip(clean, again))
    gl = G(x["grad_loss"])
    batch = ops.photometric_loss(image4, u, lambda_dssim=0.2, grad_loss=gl, want_grad=True, want_parts=True)
    for v in range(3):
        one = ops.photometric_loss(image4[v:v + 1].contiguous(), u[v:v + 1].contiguous(), lambda_dssim=0.2, grad_loss=gl[v:v + 1], want_grad=True,
                                   want_parts=True)
        assert all(torch.equal(p[0], q[v]) for p, q in zip(one, batch)), v
    assert ops.photometric_loss(image4[:0], u[:0]).shape == (0,)          # no views


def test_guard_bytes_through_the_c_call(ops):
    lib = importlib.import_module("6dgs_amd._lib").load()
    views, height, width = 2, 40, 24
    x = PR.inputs(views, height, width)
    image, target, gl = G(x["image"]), G(x["target_u8"]), G(x["grad_loss"])
    want = ops.photometric_loss(image, target, grad_loss=gl, want_grad=True, want_parts=True)
    guard = 256
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    for want_grad in (1, 0):
        need = ops.photometric_loss_workspace_bytes(views, width, height, bool(want_grad))
        assert need > 0 and (want_grad or need < ops.photometric_loss_workspace_bytes(views, width, height, True))
        ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")       # exactly workspace_bytes between the guards
        sizes = [views, 2 * views, image.numel()]
        outs = [torch.full((4 * s + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes]
        st = lib.sixdgs_photometric_loss(p(image), 4, p(target), 1, 3, views, width, height, 0.2, p(gl), p(outs[0], guard), p(outs[1], guard),
                                         p(outs[2], guard) if want_grad else None, p(ws, guard), need, stream, None)
        torch.cuda.synchronize()
        assert st == 0
        assert bool((ws[:guard] == 0xA5).all()) and bool((ws[-guard:] == 0xA5).all()), "the workspace's guard bytes were written"
        for o, k, w in zip(outs, ("loss", "parts", "grad"), (want[0], want[2], want[1])):
            assert bool((o[:guard] == 0x5A).all()) and bool((o[-guard:] == 0x5A).all()), f"the guard bytes of {k} were written"
            if k == "grad" and not want_grad:
                assert bool((o == 0x5A).all()), "a gradient was written without being asked for"
            else:
                assert torch.equal(o[guard:-guard].view(torch.float32), w.reshape(-1)), k
    assert lib.sixdgs_photometric_loss(p(image), 4, p(target), 1, 3, views, width, height, 0.2, None, p(outs[0], guard), None, p(outs[2], guard),
                                       p(ws, guard), need, stream, None) == -2            # the gradient does not fit the smaller workspace


def test_autograd_function(pkg, ops):
    autograd = importlib.import_module("6dgs_amd.autograd")
    x = PR.inputs(3, 17, 33)
    image, target, g = G(x["image"]), G(x["target_u8"]), G(x["grad_loss"])
    loss, grad = ops.photometric_loss(image, target, lambda_dssim=0.3, grad_loss=g, want_grad=True)
    leaf = image.clone().requires_grad_(True)
    out = autograd.photometric_loss(leaf, target, 0.3)
    assert out.requires_grad and torch.equal(out.detach(), loss)
    out.backward(g)
    assert bool((g < 0).any()) and torch.equal(leaf.grad.view(torch.int32), grad.view(torch.int32))      # the bits, +0 in the fourth channel included
    frozen = autograd.photometric_loss(image, target, 0.3)
    assert not frozen.requires_grad and torch.equal(frozen, loss)


def test_camera_gradient_through_rasteriser_and_loss(pkg, ops, syn):
    """d sum_v loss_v / d cams on a 300-Gaussian 40 x 24 scene: the GPU chain against fp64 autograd through both restatements, under
    the raster-backward bound rule (the bound from the fp32 chain of the same restatements)."""
    autograd = importlib.import_module("6dgs_amd.autograd")
    n, scene_seed, views, cam_seed, width, height, sh_degree = RB.CASES[2]
    assert (n, width, height) == (300, 40, 24)
    # the few pixels whose discrete outcome fp32 and fp64 decide differently (they carry no loss weight in the raster-backward tests
    # either) are given the target's value, without a gradient, in all three chains
    und = RB.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)["rr"]["undecidable"]
    assert und.shape == (views, height, width) and und.mean() <= RR.MAX_UNDECIDABLE_SHARE
    scene = syn.make_scene(n, scene_seed)
    rows = RR.camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height))
    target = PR.inputs(views, height, width)["target_f"][..., :3]
    ref = {}
    for dtype, td in ((np.float64, torch.float64), (np.float32, torch.float32)):
        t = {k: torch.from_numpy(np.asarray(scene[k], np.float32)).to(td) for k in KEYS}
        cams = torch.from_numpy(rows).to(td).requires_grad_(True)
        # the image each restatement differentiates: raster_backward_reference.render is differentiable torch
        b = torch.from_numpy(target).to(td)
        image = torch.where(torch.from_numpy(np.array(und))[..., None], b, RB.render(t, cams, width, height, sh_degree)[..., :3])
        m = PR.ssim_map(image, b)[0]
        nn = float(np.float32(3 * height * width))
        lam = float(np.float32(0.2))
        loss = (1 - lam) * (image - b).abs().reshape(views, -1).sum(1) / nn + lam * (1 - m.reshape(views, -1).sum(1) / nn)
        loss.sum().backward()
        ref[dtype] = {"cams": cams.grad.numpy(), "loss": loss.detach().numpy()}
    bounds = PR.bounds(ref[np.float64], ref[np.float32])
    args = [G(np.asarray(scene[k], np.float32)) for k in KEYS]
    cams = G(rows).requires_grad_(True)
    image = autograd.raster_views(*args, sh_degree, cams, width, height, background=RR.BACKGROUND)
    image = torch.where(G(np.array(und))[..., None], torch.nn.functional.pad(G(target), (0, 1)), image)
    loss = autograd.photometric_loss(image, G(target), 0.2)
    loss.sum().backward()
    for k, v in (("cams", cams.grad), ("loss", loss.detach())):
        scale, y, limit = bounds[k]
        err = float(np.abs(v.cpu().numpy().astype(np.float64) - ref[np.float64][k]).max())
        print(f"chain {k}: max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
        assert limit <= RB.CEILING * scale and err <= limit, k


OFFSET = (0.03, -0.02, 0.04, 0.02, -0.015, 0.01)          # tools/raster_fit.py's: about 0.054 scene units and 1.5 degrees


@pytest.fixture(scope="module")
def refinement(pkg, ops, syn):
    """make_scene(2000, 0), two 64 x 64 views drawn by the rasteriser as the query images; each start is the true camera moved by
    OFFSET, the second view's with opposite signs."""
    refine = importlib.import_module("6dgs_amd.refine")
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 0), device="cuda")
    views = render.render_views(scene, syn.make_cameras(2, 21, width=64, height=64), renderer="raster")
    gt, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
    gt = torch.stack(gt)
    rows = torch.from_numpy(render.camera_rows(views))
    off = torch.tensor([OFFSET, [-o for o in OFFSET]], dtype=torch.float32)
    moved = refine.compose(rows, off)
    w2c = torch.eye(4).repeat(2, 1, 1)
    w2c[:, :3, :] = moved[:, :12].reshape(2, 3, 4)
    start = torch.linalg.inv(w2c)
    return dict(refine=refine, scene=scene, cams=views, images=[v.image for v in views], gt=gt, K=torch.stack(Ks), start=start)


def test_refinement_halves_both_errors(refinement):
    r = refinement
    refine = r["refine"]
    out = refine.refine_poses(r["scene"], r["images"], r["start"], r["K"], steps=60, downscale=1)
    t0, a0 = refine.pose_errors(r["gt"], r["start"])
    t1, a1 = refine.pose_errors(r["gt"], out["c2w"])
    print(f"refinement, 60 steps at 64 x 64: centre error {t0.tolist()} -> {t1.tolist()}, rotation error {a0.tolist()} -> {a1.tolist()} deg, "
          f"loss {out['loss_start'].tolist()} -> {out['loss_best'].tolist()} at steps {out['best_step'].tolist()}")
    assert out["loss_history"].shape == (61, 2) and out["c2w"].shape == (2, 4, 4)
    assert bool((out["loss_best"] <= out["loss_start"]).all()) and torch.equal(out["loss_start"], out["loss_history"][0])
    assert torch.equal(out["loss_best"], out["loss_history"].min(dim=0).values)
    assert bool((t0 > 0.04).all()) and bool((a0 > 1.0).all())
    assert bool((t1 <= 0.5 * t0).all()) and bool((a1 <= 0.5 * a0).all())
    # views refined together and each alone: the same loss history, bit for bit
    for v in range(2):
        one = refine.refine_poses(r["scene"], r["images"][v:v + 1], r["start"][v:v + 1], r["K"][v:v + 1], steps=60, downscale=1)
        assert torch.equal(one["loss_history"][:, 0], out["loss_history"][:, v]), v
        assert torch.equal(one["c2w"][0], out["c2w"][v])


def test_refinement_at_half_resolution_lowers_the_loss(refinement):
    r = refinement
    out = r["refine"].refine_poses(r["scene"], r["images"], r["start"], r["K"][0], steps=20, downscale=2)
    print(f"downscale 2: loss {out['loss_start'].tolist()} -> {out['loss_best'].tolist()}")
    assert out["loss_history"].shape == (21, 2) and bool((out["loss_best"] < out["loss_start"]).all())


def test_refine_results_adds_its_keys_and_keeps_the_rest(refinement):
    r = refinement
    cams = r["cams"]
    results = [{"frame_id": i, "pred_c2w": r["start"][i].tolist(), "gt_c2w": r["gt"][i].tolist()} for i in range(2)]
    results.append({"frame_id": 2, "pred_c2w": np.full((4, 4), np.nan).tolist(), "gt_c2w": r["gt"][0].tolist()})
    before = [dict(x) for x in results]
    out = r["refine"].refine_results(r["scene"], list(cams) + [cams[0]], results, steps=10, downscale=2)
    for i in range(2):
        assert {k: out[i][k] for k in before[i]} == before[i]
        assert set(out[i]) - set(before[i]) == {"refined_c2w", "refined_translation_error", "refined_angular_error", "photometric_loss_before",
                                                "photometric_loss_after"}
        assert out[i]["photometric_loss_after"] <= out[i]["photometric_loss_before"] and np.isfinite(out[i]["refined_translation_error"])
    assert out[2] == before[2] or str(out[2]) == str(before[2])


def test_pose_errors_of_the_refiner_are_the_pose_kernels(ops, refinement):
    """refine.pose_errors restates the formulas the pose kernel reports test_pose_estimation's errors with; the sweep puts the two side
    by side, so they must agree on the same poses: 1e-5 max(1, t) in translation and 1e-2 degrees in angle (fp32 acos of a trace
    summed in another order; the tolerances of tests/test_gpu_cfg1.py against the CPU checker)."""
    import pose_tail_reference as PT
    cs, _ = PT.reference_cases(100)
    ori, dr, idx, val, up, gt = PT.stack(cs)
    out = ops.solve_pose(*[G(np.asarray(a)) for a in (ori, dr, idx, val, up, gt)])
    errors, c2w = out["errors"].cpu(), out["c2w"].cpu()
    t, a = refinement["refine"].pose_errors(torch.from_numpy(np.asarray(gt, np.float32)).reshape(-1, 4, 4), c2w)
    ok = torch.isfinite(errors).all(dim=1)
    assert int(ok.sum()) >= len(cs) // 2
    dt, da = (t - errors[:, 0]).abs()[ok], (a - errors[:, 1]).abs()[ok]
    print(f"pose_errors against the kernel on {int(ok.sum())} poses: translation {float(dt.max()):.2e}, angle {float(da.max()):.2e} deg")
    assert bool((dt <= 1e-5 * errors[ok, 0].clamp(min=1.0)).all()) and bool((da <= 1e-2).all())
