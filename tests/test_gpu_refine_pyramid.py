"""A coarse-to-fine refinement schedule on the GPU: sixdgs_pose_rebase copies bits; sixdgs_refine_poses_levels against the same
schedule walked in Python over the raw ops (tests/pyramid_reference.py), every output bit for bit, on a 64 x 64 and on a 70 x 66 query
(whose level of downscale 4 is a cropped 17 x 16 image with a ragged tile edge); determinism and batching bit for bit; a one-level
schedule against sixdgs_refine_poses; the capacity protocol across levels; the keep-the-input invariant; the two backends of
refine_poses against each other; refine_results.  The fixture is test_gpu_refine_fused.py's: make_scene(2000, 0), two query views drawn
by the rasteriser, each start the true camera moved by that file's OFFSET.  Everything runs inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OFFSET = (0.03, -0.02, 0.04, 0.02, -0.015, 0.01)
OFFSET_SIGNS = (1.0, -1.0)
SCHEDULE = ((4, 5, 4e-3), (2, 5, 2e-3), (1, 5, 1e-3))
GUARD = 256
RAW = ("out_rows", "loss_input", "kept_input", "best_loss", "best_step", "status")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def queries(pkg, ops, syn):
    """size -> the fixture at that query size, made once."""
    refine = importlib.import_module("6dgs_amd.refine")
    render = importlib.import_module("6dgs_amd.render")
    test = importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 0), device="cuda")
    tensors, sh_degree = refine._scene_tensors(scene)
    tensors = tuple(t.detach() for t in tensors)
    cache = {}

    def make(width, height):
        if (width, height) in cache:
            return cache[(width, height)]
        views = render.render_views(scene, syn.make_cameras(2, 21, width=width, height=height), renderer="raster")
        gt, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in views])
        gt, K = torch.stack(gt), torch.stack(Ks)
        rows = torch.from_numpy(render.camera_rows(views))
        off = torch.tensor([[s * o for o in OFFSET] for s in OFFSET_SIGNS], dtype=torch.float32)
        w2c = torch.eye(4).repeat(2, 1, 1)
        w2c[:, :3, :] = refine.compose(rows, off)[:, :12].reshape(2, 3, 4)
        start = torch.linalg.inv(w2c)
        images = [v.image for v in views]
        stacked = refine._stack_images(images, "cuda")
        plan = refine.level_plan(SCHEDULE, width, height)
        targets = ops.target_pyramid(stacked, [p["downscale"] for p in plan])
        levels = [dict(width=p["width"], height=p["height"], steps=p["steps"], lr=p["lr"], target=t,
                       intrinsics=refine.scaled_intrinsics(K, p["downscale"], p["crop_x"], p["crop_y"]).cuda().contiguous())
                  for p, t in zip(plan, targets)]
        start_rows = torch.cat([torch.linalg.inv(start)[:, :3, :].reshape(2, 12).cuda(), levels[-1]["intrinsics"]], dim=1).contiguous()
        cache[(width, height)] = dict(refine=refine, scene=scene, cams=views, images=images, gt=gt, K=K, start=start, plan=plan, levels=levels,
                                      start_rows=start_rows, tensors=tensors, sh_degree=sh_degree, capacity=ops.raster_instances_estimate(2000, 2))
        return cache[(width, height)]

    return make


def with_capacity(levels, capacities):
    return [dict(lv, max_instances=c) for lv, c in zip(levels, capacities)]


def same_raw(a, b, what=""):
    for k in RAW:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)
    assert len(a["history"]) == len(b["history"])
    for l, (x, y) in enumerate(zip(a["history"], b["history"])):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "history", l)
    assert a["instances_needed"] == b["instances_needed"], what


def test_rebase_copies_bits(ops):
    rng = np.random.default_rng(3)
    rows = rng.integers(-2 ** 31, 2 ** 31, (67, 16), dtype=np.int64).astype(np.int32)      # every bit pattern: NaNs with payloads, -0, denormals
    intr = rng.integers(-2 ** 31, 2 ** 31, (67, 4), dtype=np.int64).astype(np.int32)
    r, k = torch.from_numpy(rows).cuda().view(torch.float32), torch.from_numpy(intr).cuda().view(torch.float32)
    out = ops.pose_rebase(r, k).view(torch.int32).cpu().numpy()
    assert np.array_equal(out[:, :12], rows[:, :12]) and np.array_equal(out[:, 12:], intr)
    # the raw call between guards, in place
    lib = importlib.import_module("6dgs_amd._lib").load()
    buf = torch.full((67 * 64 + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:-GUARD].view(torch.float32).reshape(67, 16)
    view.copy_(r)
    assert lib.sixdgs_pose_rebase(view.data_ptr(), k.data_ptr(), 67, view.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0x5A).all()) and bool((buf[-GUARD:] == 0x5A).all())
    assert np.array_equal(view.view(torch.int32).cpu().numpy(), out)


@pytest.mark.parametrize("size", ((64, 64), (70, 66)))
def test_schedule_is_the_walk_over_the_raw_ops_bit_for_bit(ops, queries, size):
    q = queries(*size)
    if size == (70, 66):
        assert (q["levels"][0]["width"], q["levels"][0]["height"]) == (17, 16) and (q["plan"][0]["crop_x"], q["plan"][0]["crop_y"]) == (1, 1)
    caps = [q["capacity"]] * 3
    fused = ops.refine_poses_levels_raw(*q["tensors"], q["sh_degree"], q["start_rows"], with_capacity(q["levels"], caps), retry=False)
    hand = R.walk(ops, torch, q["tensors"], q["sh_degree"], q["start_rows"], q["levels"], caps)
    same_raw(fused, hand, size)
    assert fused["best_loss"].shape == (3, 2) and [tuple(h.shape) for h in fused["history"]] == [(6, 2)] * 3
    assert all(bool(torch.isfinite(h).all()) for h in fused["history"]) and bool(torch.isfinite(fused["loss_input"]).all())
    assert not bool(fused["status"].any()) and all(n > 0 for n in fused["instances_needed"]) and fused["max_instances"] == caps
    assert bool((fused["best_step"] > 0).any()), "no level moved any view"
    # every level starts where the level before ended: its first loss is the best camera's, seen at the new resolution
    print(f"{size}: loss_input {fused['loss_input'].tolist()}, best per level {fused['best_loss'].tolist()}, kept {fused['kept_input'].tolist()}")


def test_same_bytes_twice_and_each_view_alone(ops, queries):
    q = queries(70, 66)
    args = (*q["tensors"], q["sh_degree"])
    both = ops.refine_poses_levels_raw(*args, q["start_rows"], q["levels"])
    again = ops.refine_poses_levels_raw(*args, q["start_rows"], q["levels"])
    same_raw(both, again, "twice")
    for v in range(2):
        levels = [dict(lv, target=lv["target"][v:v + 1].contiguous(), intrinsics=lv["intrinsics"][v:v + 1].contiguous()) for lv in q["levels"]]
        one = ops.refine_poses_levels_raw(*args, q["start_rows"][v:v + 1].contiguous(), levels)
        for k in ("out_rows", "loss_input", "kept_input", "status"):
            assert torch.equal(one[k][0], both[k][v]), (k, v)
        for k in ("best_loss", "best_step"):
            assert torch.equal(one[k][:, 0], both[k][:, v]), (k, v)
        for l in range(3):
            assert torch.equal(one["history"][l][:, 0], both["history"][l][:, v]), (l, v)


def test_one_level_is_sixdgs_refine_poses(ops, queries):
    q = queries(64, 64)
    lv = q["levels"][1]                                   # downscale 2
    start = ops.pose_rebase(q["start_rows"], lv["intrinsics"])
    levels = ops.refine_poses_levels_raw(*q["tensors"], q["sh_degree"], start, [dict(lv, steps=7)])
    single = ops.refine_poses_raw(*q["tensors"], q["sh_degree"], start, lv["width"], lv["height"], lv["target"], steps=7, lr=lv["lr"])
    assert torch.equal(levels["history"][0], single["history"]) and torch.equal(levels["best_loss"][0], single["best_loss"])
    assert torch.equal(levels["best_step"][0], single["best_step"]) and levels["instances_needed"] == [single["instances_needed"]]
    assert torch.equal(levels["loss_input"], single["history"][0])              # the input at the only level is iterate 0
    moved = single["best_step"] > 0
    assert torch.equal(levels["kept_input"] == 0, moved) and torch.equal(levels["out_rows"], single["best_rows"])


def test_capacity_too_small_at_the_middle_level(ops, queries):
    q = queries(64, 64)
    args = (*q["tensors"], q["sh_degree"])
    l0, l1, _ = q["levels"]
    first = ops.refine_poses_raw(*args, ops.pose_rebase(q["start_rows"], l0["intrinsics"]), l0["width"], l0["height"], l0["target"], steps=l0["steps"],
                                 lr=l0["lr"])
    start1 = ops.pose_rebase(first["best_rows"], l1["intrinsics"])
    needed1 = ops.raster_views(*args, start1, l1["width"], l1["height"], want_u8=False, want_instances=True)
    assert needed1 > 64
    ample = q["capacity"]
    small = ops.refine_poses_levels_raw(*args, q["start_rows"], with_capacity(q["levels"], [ample, 64, ample]), retry=False)
    assert small["status"].tolist() == [2, 2] and small["max_instances"] == [ample, 64, ample]
    assert small["instances_needed"][1] == needed1 and small["instances_needed"][0] == first["instances_needed"] and small["instances_needed"][2] > 0
    assert torch.equal(small["history"][0], first["history"]) and bool(torch.isfinite(small["history"][0]).all())
    assert bool(torch.isnan(small["history"][1]).all()) and bool(torch.isnan(small["history"][2]).all())
    assert bool(torch.isinf(small["best_loss"][1:]).all()) and small["best_step"][1:].tolist() == [[0, 0], [0, 0]]
    assert small["kept_input"].tolist() == [1, 1] and bool(torch.isfinite(small["loss_input"]).all())
    assert torch.equal(small["out_rows"].view(torch.int32), q["start_rows"].view(torch.int32))
    # with retry the call grows that level alone and ends as an ample run does
    fits = ops.refine_poses_levels_raw(*args, q["start_rows"], with_capacity(q["levels"], [ample] * 3), retry=False)
    rerun = ops.refine_poses_levels_raw(*args, q["start_rows"], with_capacity(q["levels"], [ample, 64, ample]))
    assert not bool(rerun["status"].any()) and rerun["max_instances"][0] == rerun["max_instances"][2] == ample and 64 < rerun["max_instances"][1]
    same_raw(rerun, fits, "rerun")
    # too small for the input's evaluation at the last level: its loss is NaN, and nothing after it is recorded
    none = ops.refine_poses_levels_raw(*args, q["start_rows"], with_capacity(q["levels"], [ample, ample, 64]), retry=False)
    assert none["status"].tolist() == [2, 2] and bool(torch.isnan(none["loss_input"]).all()) and none["kept_input"].tolist() == [1, 1]
    assert all(bool(torch.isnan(h).all()) for h in none["history"]) and torch.equal(none["out_rows"].view(torch.int32), q["start_rows"].view(torch.int32))


@pytest.fixture(scope="module")
def both_backends(queries):
    q = queries(64, 64)
    start = q["start"].clone()
    return {b: q["refine"].refine_poses(q["scene"], q["images"], start, q["K"], levels=SCHEDULE, backend=b) for b in ("torch", "fused")}


def test_kept_input_or_a_lower_loss_by_construction(queries, both_backends):
    q = queries(64, 64)
    for backend, out in both_backends.items():
        kept = out["kept_input"]
        assert kept.dtype == torch.bool and bool((kept | (out["loss_best"] < out["loss_input"])).all()), backend
        assert torch.equal(out["loss_start"], out["loss_input"]) and torch.equal(out["loss_best"], out["level_loss_best"][-1])
        for v in range(2):
            if bool(kept[v]):
                assert torch.equal(out["c2w"][v].cpu().view(torch.int32), q["start"][v].view(torch.int32)), (backend, v)
            else:
                assert not torch.equal(out["c2w"][v].cpu(), q["start"][v]), (backend, v)
    # a schedule that cannot help -- one step at a rate that throws the camera far off -- keeps the input pose, bit for bit
    out = q["refine"].refine_poses(q["scene"], q["images"], q["gt"].clone(), q["K"], levels=[(4, 1, 0.5), (1, 1, 0.5)], backend="fused")
    print(f"thrown: loss_input {out['loss_input'].tolist()}, best {out['level_loss_best'].tolist()}, kept {out['kept_input'].tolist()}")
    assert bool((out["kept_input"] | (out["loss_best"] < out["loss_input"])).all())
    assert torch.equal(out["c2w"][out["kept_input"]].cpu().view(torch.int32), q["gt"][out["kept_input"].cpu()].view(torch.int32))


def test_both_backends_agree(queries, both_backends):
    """The plan, the input's loss and every level's first history row.  The tolerance is test_gpu_refine_fused.py's for its two
    backends: the same kernels on the same rows give the same bits, so the comparison is torch.equal.  It holds beyond level 0 because
    the torch arm of a level schedule moves its cameras with the library's own pose step, under autograd's image and loss."""
    q = queries(64, 64)
    t, f = both_backends["torch"], both_backends["fused"]
    assert t["levels"] == f["levels"] == q["plan"]
    for l in range(len(SCHEDULE)):
        print(f"level {l}: first history row torch {t['loss_history'][l][0].tolist()} fused {f['loss_history'][l][0].tolist()}; "
              f"max |history difference| {float((t['loss_history'][l] - f['loss_history'][l]).abs().max()):.3e}")
    print(f"loss_input torch {t['loss_input'].tolist()} fused {f['loss_input'].tolist()}")
    assert torch.equal(t["loss_input"], f["loss_input"])
    for l in range(len(SCHEDULE)):
        assert torch.equal(t["loss_history"][l][0], f["loss_history"][l][0]), l
    # beyond what the schedule's contract asks: the same pose step on the same gradients, so every row and every result is the same bits
    for l in range(len(SCHEDULE)):
        assert torch.equal(t["loss_history"][l], f["loss_history"][l]), l
    for k in ("c2w", "loss_best", "best_step", "kept_input", "level_loss_best", "level_best_step", "status"):
        assert torch.equal(t[k], f[k]), k
    assert set(f) == set(t)
    for k in t:
        if k == "levels":
            continue
        if k == "loss_history":
            assert [x.shape for x in t[k]] == [x.shape for x in f[k]] and [x.dtype for x in t[k]] == [x.dtype for x in f[k]]
            continue
        assert t[k].shape == f[k].shape and t[k].dtype == f[k].dtype and t[k].device == f[k].device, k
    assert not bool(f["status"].any()) and not bool(t["status"].any())


def test_refine_results_with_levels_adds_its_keys_and_keeps_the_rest(queries):
    q = queries(64, 64)
    cams = q["cams"]
    results = [{"frame_id": i, "pred_c2w": q["start"][i].tolist(), "gt_c2w": q["gt"][i].tolist()} for i in range(2)]
    results.append({"frame_id": 2, "pred_c2w": np.full((4, 4), np.nan).tolist(), "gt_c2w": q["gt"][0].tolist()})
    before = [dict(x) for x in results]
    out = q["refine"].refine_results(q["scene"], list(cams) + [cams[0]], results, levels=[(4, 6, 4e-3), (2, 6, 2e-3)], backend="fused")
    for i in range(2):
        assert {k: out[i][k] for k in before[i]} == before[i]
        assert set(out[i]) - set(before[i]) == {"refined_c2w", "refined_translation_error", "refined_angular_error", "photometric_loss_before",
                                                "photometric_loss_after"}
        assert np.isfinite(out[i]["refined_translation_error"]) and np.isfinite(out[i]["photometric_loss_before"])
        assert out[i]["photometric_loss_after"] < out[i]["photometric_loss_before"] or out[i]["refined_c2w"] == before[i]["pred_c2w"]
    assert str(out[2]) == str(before[2])
