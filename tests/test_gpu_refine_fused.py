"""Pose refinement below the C ABI on the GPU: the step kernels (sixdgs_pose_compose, sixdgs_pose_step) against the fp64 restatement
(tests/pose_step_reference.py) under its own fp32 bound, with guard bytes around every output; sixdgs_refine_poses against the same
loop composed in Python from the parts, bit for bit; determinism and batching bit for bit; the refiner with backend="fused" on the
fixture of test_gpu_photometric.py; the capacity protocol; refine_results.  Everything runs inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_step_reference as P  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")
OFFSET = (0.03, -0.02, 0.04, 0.02, -0.015, 0.01)          # tools/raster_fit.py's: about 0.054 scene units and 1.5 degrees
GUARD = 256
RAW = ("best_rows", "best_loss", "best_step", "history", "delta", "status")


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


def guarded(shape, dtype, value=None):
    """(buffer, view): a tensor of `shape` between two runs of GUARD bytes of 0x5A."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(dtype).reshape(shape)
    if value is not None:
        view.copy_(value)
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == 0x5A).all()) and bool((buf[-GUARD:] == 0x5A).all())


def within(got, r64, r32, what):
    scale, y, limit = P.bounds({"x": r64}, {"x": r32})["x"]
    a = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(a - r64).max())
    assert limit <= P.CEILING * scale, f"{what}: the case is unfit"
    assert np.isfinite(a).all() and err <= limit, f"{what}: {err:.3e} > {limit:.3e} (scale {scale:.3e}, y {y:.3e})"
    return err / limit


@pytest.mark.parametrize("views", (1, 3, 64, 65, 257))
def test_step_kernels_against_fp64(ops, views):
    lib = importlib.import_module("6dgs_amd._lib").load()
    stream = torch.cuda.current_stream().cuda_stream
    worst = 0.0
    for ti, theta in enumerate(P.THETAS):
        start_h, delta_h, d_rows_h = P.random_views(views, theta, 10 * views + ti)
        start, delta, d_rows = G(start_h), G(delta_h), G(d_rows_h)
        # compose through the raw call, into guarded memory
        buf, rows = guarded((views, 16), torch.float32)
        assert lib.sixdgs_pose_compose(start.data_ptr(), delta.data_ptr(), views, rows.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert guards_intact(buf) and torch.equal(rows, ops.pose_compose(start, delta))
        worst = max(worst, within(rows, P.compose(start_h, delta_h, np.float64), P.compose(start_h, delta_h, np.float32), f"rows at {theta}"))
        assert torch.equal(ops.pose_compose(start, torch.zeros_like(delta)).view(torch.int32), start.view(torch.int32))      # delta = 0: the start's bits
        # two steps and the evaluate-only step from this delta, every state array and the history between guards
        state = ops.pose_state(start)
        state["delta"], state["rows"] = delta.clone(), rows.clone()
        bufs = {}
        for k in list(state):
            bufs[k], state[k] = guarded(tuple(state[k].shape), state[k].dtype, state[k])
        bufs["history"], history = guarded((3, views), torch.float32)
        s64, s32 = P.new_state(start_h, np.float64), P.new_state(start_h, np.float32)
        for s in (s64, s32):
            s["delta"], s["rows"] = delta_h.astype(s["delta"].dtype), P.compose(start_h, delta_h, s["rows"].dtype.type)
        rng = np.random.default_rng(ti)
        for step in range(3):
            last = step == 2
            g = (d_rows_h * rng.uniform(0.5, 2.0, (views, 1)) * rng.choice([-1.0, 1.0], (views, 16))).astype(np.float32)
            loss = rng.random(views).astype(np.float32)
            before = {k: v.clone() for k, v in state.items()}
            ops.pose_step(start, G(loss), None if last else G(g), state, history[step], step, evaluate_only=last)
            P.step(s64, start_h, loss, g, step, np.float64, evaluate_only=last)
            P.step(s32, start_h, loss, g, step, np.float32, evaluate_only=last)
            assert torch.equal(history[step], G(loss))
            for k in ("delta", "m", "v", "rows"):
                if last:
                    assert torch.equal(state[k], before[k]), k
                else:
                    worst = max(worst, within(state[k], s64[k], s32[k], f"{k} after step {step + 1} at {theta}"))
            assert np.array_equal(state["best_step"].cpu().numpy(), s32["best_step"]) and not bool(state["status"].any())
            assert np.array_equal(state["best_loss"].cpu().numpy(), s32["best_loss"])
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in bufs.values()), "guard bytes were written"
    print(f"{views} views: worst measured / bound {worst:.3f}")


def test_step_kernel_freezes_and_reports_capacity(ops):
    """The bookkeeping's rules on the device (tests/test_pose_step_host.py checks the same function on the host)."""
    start_h, _, d_rows_h = P.random_views(3, 0.0, 9)
    start, d_rows = G(start_h), G(d_rows_h)
    state, history = ops.pose_state(start), torch.zeros(4, 3, device="cuda")
    count = torch.tensor([90], dtype=torch.int64, device="cuda")
    ops.pose_step(start, G(np.float32([0.5, 0.5, 0.5])), d_rows, state, history[0], 0, instances=count, max_instances=100)
    g = d_rows.clone()
    g[2, 7] = float("inf")
    g[1, 13] = float("nan")                                   # an intrinsics entry: ignored
    frozen = {k: state[k].clone() for k in ("delta", "m", "v", "rows")}
    ops.pose_step(start, G(np.float32([np.nan, 0.4, 0.3])), g, state, history[1], 1, instances=count, max_instances=100)
    assert state["status"].tolist() == [1, 0, 1] and state["best_step"].tolist() == [0, 1, 1]
    for k in frozen:
        assert torch.equal(state[k][[0, 2]], frozen[k][[0, 2]]) and not torch.equal(state[k][1], frozen[k][1]), k
    kept = {k: v.clone() for k, v in state.items()}
    count.fill_(101)
    ops.pose_step(start, G(np.float32([0.1, 0.1, 0.1])), d_rows, state, history[2], 2, instances=count, max_instances=100)
    count.fill_(95)
    ops.pose_step(start, G(np.float32([0.1, 0.1, 0.1])), None, state, history[3], 3, instances=count, max_instances=100, evaluate_only=True)
    assert state["status"].tolist() == [3, 2, 3] and int(state["instances_needed"]) == 101 and bool(torch.isnan(history[2:]).all())
    assert all(torch.equal(kept[k], state[k]) for k in kept if k not in ("status", "instances_needed"))


def hand_loop(ops, tensors, sh_degree, start, width, height, target, steps, capacity, lam=0.2, raster=None, **hyper):
    """sixdgs_refine_poses composed in Python from its parts; raster: scale_modifier, scale_is_log and opacity_is_logit of both rasteriser
    calls."""
    raster = raster or {}
    views = start.shape[0]
    state = ops.pose_state(start)
    history = torch.empty(steps + 1, views, device="cuda")
    for step in range(steps + 1):
        last = step == steps
        image, needed, fwd = ops.raster_views(*tensors, sh_degree, state["rows"], width, height, want_float=True, want_u8=False, want_instances=True,
                                              want_state=True, max_instances=capacity, **raster)
        assert needed <= capacity and fwd[1] == capacity
        if last:
            loss, d_rows = ops.photometric_loss(image, target, lambda_dssim=lam), None
        else:
            loss, grad = ops.photometric_loss(image, target, lambda_dssim=lam, want_grad=True)
            d_rows = ops.raster_views_backward(*tensors, sh_degree, state["rows"], width, height, grad, fwd, want=("cams",), **raster)[6]
        ops.pose_step(start, loss, d_rows, state, history[step], step, instances=torch.tensor([needed], dtype=torch.int64, device="cuda"),
                      max_instances=capacity, evaluate_only=last, **hyper)
    return dict(state, history=history, instances_needed=int(state["instances_needed"]))


OFFSET_SIGNS = (1.0, -1.0)


@pytest.fixture(scope="module")
def refinement(pkg, ops, syn):
    """The fixture of test_gpu_photometric.py: make_scene(2000, 0), two 64 x 64 views drawn by the rasteriser as the query images; each
    start is the true camera moved by OFFSET, the second view's with opposite signs.  Plus the camera rows and the target the refiner
    forms from them at downscale 1."""
    refine = importlib.import_module("6dgs_amd.refine")
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 0), device="cuda")
    views = render.render_views(scene, syn.make_cameras(2, 21, width=64, height=64), renderer="raster")
    gt, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
    gt, K = torch.stack(gt), torch.stack(Ks)
    rows = torch.from_numpy(render.camera_rows(views))
    off = torch.tensor([[s * o for o in OFFSET] for s in OFFSET_SIGNS], dtype=torch.float32)
    moved = refine.compose(rows, off)
    w2c = torch.eye(4).repeat(2, 1, 1)
    w2c[:, :3, :] = moved[:, :12].reshape(2, 3, 4)
    start = torch.linalg.inv(w2c)
    images = [v.image for v in views]
    target, ox, oy = refine.prepare_target(refine._stack_images(images, "cuda"), 1)
    start_rows = torch.cat([torch.linalg.inv(start)[:, :3, :].reshape(2, 12), refine.scaled_intrinsics(K, 1, ox, oy)], dim=1).cuda().contiguous()
    tensors, sh_degree = refine._scene_tensors(scene)
    return dict(refine=refine, scene=scene, cams=views, images=images, gt=gt, K=K, start=start, target=target, start_rows=start_rows,
                tensors=tuple(t.detach() for t in tensors), sh_degree=sh_degree)


@pytest.mark.parametrize("steps,kind", ((12, "u8"), (1, "f32")))
def test_loop_is_the_hand_composition_bit_for_bit(ops, refinement, steps, kind):
    r = refinement
    target = r["target"] if kind == "u8" else (r["target"].float() / 255.0).contiguous()
    assert target.dtype == (torch.uint8 if kind == "u8" else torch.float32)
    capacity = ops.raster_instances_estimate(2000, 2)
    fused = ops.refine_poses_raw(*r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, target, steps=steps, max_instances=capacity, retry=False)
    hand = hand_loop(ops, r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, target, steps, capacity)
    assert fused["history"].shape == (steps + 1, 2) and bool(torch.isfinite(fused["history"]).all())
    for k in RAW:
        assert fused[k].dtype == hand[k].dtype and torch.equal(fused[k], hand[k]), k
    assert fused["instances_needed"] == hand["instances_needed"] > 0 and not bool(fused["status"].any())
    assert bool(fused["delta"].abs().sum(1).gt(0).all())                                                       # the loop moved both views
    if steps > 1:
        assert bool((fused["best_step"] > 0).all()) and not torch.equal(fused["best_rows"], r["start_rows"])


def test_same_bytes_twice_and_each_view_alone(ops, refinement):
    r = refinement
    kw = dict(steps=8)
    both = ops.refine_poses_raw(*r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, r["target"], **kw)
    again = ops.refine_poses_raw(*r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, r["target"], **kw)
    for k in RAW:
        assert torch.equal(both[k], again[k]), k
    assert both["instances_needed"] == again["instances_needed"]
    for v in range(2):
        one = ops.refine_poses_raw(*r["tensors"], r["sh_degree"], r["start_rows"][v:v + 1].contiguous(), 64, 64, r["target"][v:v + 1].contiguous(), **kw)
        assert torch.equal(one["history"][:, 0], both["history"][:, v]), v
        for k in ("best_rows", "best_loss", "best_step", "delta", "status"):
            assert torch.equal(one[k][0], both[k][v]), (k, v)


@pytest.fixture(scope="module")
def both_backends(refinement):
    r = refinement
    return {b: r["refine"].refine_poses(r["scene"], r["images"], r["start"], r["K"], steps=60, downscale=1, backend=b) for b in ("torch", "fused")}


def test_fused_refinement_halves_both_errors(refinement, both_backends):
    r, refine = refinement, refinement["refine"]
    out, ref = both_backends["fused"], both_backends["torch"]
    t0, a0 = refine.pose_errors(r["gt"], r["start"])
    t1, a1 = refine.pose_errors(r["gt"], out["c2w"])
    tt, at = refine.pose_errors(r["gt"], ref["c2w"])
    print(f"fused refinement, 60 steps at 64 x 64: centre error {t0.tolist()} -> {t1.tolist()} (torch backend {tt.tolist()}), rotation error "
          f"{a0.tolist()} -> {a1.tolist()} deg (torch backend {at.tolist()}), loss {out['loss_start'].tolist()} -> {out['loss_best'].tolist()} at steps "
          f"{out['best_step'].tolist()}; max |history - torch's| {float((out['loss_history'] - ref['loss_history']).abs().max()):.3e}")
    assert bool((t0 > 0.04).all()) and bool((a0 > 1.0).all())
    assert bool((t1 <= 0.5 * t0).all()) and bool((a1 <= 0.5 * a0).all())
    assert bool((out["loss_best"] <= out["loss_start"]).all()) and torch.equal(out["loss_start"], out["loss_history"][0])
    assert torch.equal(out["loss_best"], out["loss_history"].min(dim=0).values)
    # the same kernels on the same rows: iterate 0's loss is the torch backend's, bit for bit
    assert torch.equal(out["loss_history"][0], ref["loss_history"][0])
    # the torch backend's keys, dtypes and shapes, plus status, all zero
    assert set(out) == set(ref) | {"status"}
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype and out[k].device == ref[k].device, k
    assert out["status"].shape == (2,) and out["status"].dtype == torch.int32 and not bool(out["status"].any())


def test_capacity_protocol(ops, refinement):
    r = refinement
    args = (*r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, r["target"])
    needed = ops.raster_views(*r["tensors"], r["sh_degree"], r["start_rows"], 64, 64, want_u8=False, want_instances=True)
    assert needed > 64
    small = ops.refine_poses_raw(*args, steps=5, max_instances=64, retry=False)
    assert small["status"].tolist() == [2, 2] and small["instances_needed"] == needed and small["max_instances"] == 64
    assert small["best_step"].tolist() == [0, 0] and torch.equal(small["best_rows"], r["start_rows"]) and bool(torch.isnan(small["history"]).all())
    ample = ops.refine_poses_raw(*args, steps=5, max_instances=4 * needed, retry=False)
    rerun = ops.refine_poses_raw(*args, steps=5, max_instances=64)
    assert not bool(rerun["status"].any()) and 64 < rerun["max_instances"] < 4 * needed
    for k in RAW:
        assert torch.equal(rerun[k], ample[k]), k


def test_refine_results_adds_its_keys_and_keeps_the_rest(refinement):
    r = refinement
    cams = r["cams"]
    results = [{"frame_id": i, "pred_c2w": r["start"][i].tolist(), "gt_c2w": r["gt"][i].tolist()} for i in range(2)]
    results.append({"frame_id": 2, "pred_c2w": np.full((4, 4), np.nan).tolist(), "gt_c2w": r["gt"][0].tolist()})
    before = [dict(x) for x in results]
    out = r["refine"].refine_results(r["scene"], list(cams) + [cams[0]], results, steps=10, downscale=2, backend="fused")
    for i in range(2):
        assert {k: out[i][k] for k in before[i]} == before[i]
        assert set(out[i]) - set(before[i]) == {"refined_c2w", "refined_translation_error", "refined_angular_error", "photometric_loss_before",
                                                "photometric_loss_after"}
        assert out[i]["photometric_loss_after"] < out[i]["photometric_loss_before"] and np.isfinite(out[i]["refined_translation_error"])
    assert str(out[2]) == str(before[2])
