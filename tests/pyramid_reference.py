"""Restatements of a coarse-to-fine refinement schedule (csrc/pyramid_rules.h; include/sixdgs.h: sixdgs_target_pyramid,
sixdgs_pose_rebase, sixdgs_refine_poses_levels) in numpy and plain Python, for the CPU and the GPU tests.

    geometry, intrinsics          a level's size, crop and intrinsics
    target_f32                    a level's target, the stated fp32 expression operation by operation (the product's bits)
    target_f64                    the same in fp64: the plain mean of u / 255, composited or not
    bound_f32, bound_prepare      how far target_f32 and refine.prepare_target may lie from target_f64, from the count of roundings
    keep_input                    the rule that keeps the input pose
    walk                          sixdgs_refine_poses_levels composed from the raw ops, step by step

ROUNDINGS.  u = 2^-24 is the unit roundoff of fp32.  Without compositing the block sum S <= 255 * 2^16 and 255 d d are integers below
2^24, so float(S) / float(255 d d) rounds ONCE: |fp32 - exact| <= u * exact.  With compositing the expression
(float(S1) + (255 bg) float(S2)) / (65025 float(d d)) rounds at most SIX times -- float(S1) (S1 may pass 2^24), 255 bg, its product with
float(S2), the sum, 65025 float(d d) (which may pass 2^24), the quotient -- and for a background in [0, 1] every term is non-negative:
nothing cancels, each rounding moves the result by at most a factor (1 +- u), so |fp32 - exact| <= ((1 + u)^6 - 1) * exact.  The fp64
restatement's own error is below 1e-15 for values in [0, 1], which is added.

refine.prepare_target on the CPU forms per pixel u / 255 (one rounding) or, composited, (u_c / 255)(u_a / 255) + (1 - u_a / 255) bg (six
roundings of values in [0, 1]: two quotients, the product, the difference, its product, the sum), then the mean of n = d d such values:
a sum of n terms in SOME order (n - 1 roundings of partial sums that never exceed n) and one quotient.  Its result is therefore within
(1 | 6) u + (n - 1) u + u of the exact mean, whichever order the sum takes."""
import numpy as np

F = np.float32
U = 2.0 ** -24
ROUNDINGS = {False: 1, True: 6}
PREPARE_ELEMENT_ROUNDINGS = {False: 1, True: 6}
FP64_SLACK = 1e-15
MAX_LEVELS, MAX_DOWNSCALE = 8, 256


def geometry(W, H, d):
    """(w, h, ox, oy)."""
    w, h = W // d, H // d
    return w, h, (W - w * d) // 2, (H - h * d) // 2


def intrinsics(k4, d, ox, oy):
    """(fx / d, fy / d, (cx - ox) / d, (cy - oy) / d) in fp32, d, ox and oy converted first.  k4: [..., 4]."""
    k4 = np.asarray(k4, F)
    df = F(d)
    return np.stack([k4[..., 0] / df, k4[..., 1] / df, (k4[..., 2] - F(ox)) / df, (k4[..., 3] - F(oy)) / df], axis=-1).astype(F)


def _blocks(images, d):
    """uint8 [V,H,W,C] -> the crop's blocks as int64 [V,h,w,d*d,C]."""
    images = np.asarray(images)
    V, H, W, C = images.shape
    w, h, ox, oy = geometry(W, H, d)
    assert w >= 1 and h >= 1
    crop = images[:, oy:oy + h * d, ox:ox + w * d].astype(np.int64)
    return crop.reshape(V, h, d, w, d, C).transpose(0, 1, 3, 2, 4, 5).reshape(V, h, w, d * d, C)


def target_f32(images, d, composite=False, background=(1.0, 1.0, 1.0)):
    """A level's target [V,h,w,3] with the product's own operations: exact integer block sums, then the fp32 expression term by term."""
    b = _blocks(images, d)
    if not composite:
        S = b[..., :3].sum(axis=3)
        assert int(S.max(initial=0)) < 2 ** 24 and 255 * d * d < 2 ** 24
        return (S.astype(F) / F(255 * d * d)).astype(F)
    assert b.shape[-1] == 4
    S1 = (b[..., :3] * b[..., 3:]).sum(axis=3)
    S2 = (255 - b[..., 3]).sum(axis=3)[..., None]
    assert int(S1.max(initial=0)) < 2 ** 32
    bg255 = (F(255.0) * np.asarray(background, F)).astype(F)
    s1 = S1.astype(np.uint64).astype(F)                 # round to nearest, ties to even
    s2 = S2.astype(F)                                   # exact
    over = (bg255 * s2).astype(F)
    num = (s1 + over).astype(F)
    den = F(F(65025.0) * F(d * d))
    return (num / den).astype(F)


def target_f64(images, d, composite=False, background=(1.0, 1.0, 1.0)):
    """The plain mean of u / 255 over the blocks, composited over the (fp32-valued) background first or not, in fp64."""
    x = _blocks(images, d).astype(np.float64) / 255.0
    if composite:
        bg = np.asarray(background, F).astype(np.float64)
        return (x[..., :3] * x[..., 3:] + (1.0 - x[..., 3:]) * bg).mean(axis=3)
    return x[..., :3].mean(axis=3)


def bound_f32(t64, composite):
    """|target_f32 - target_f64| allowed per entry."""
    return ((1.0 + U) ** ROUNDINGS[bool(composite)] - 1.0) * np.abs(t64) + FP64_SLACK


def bound_prepare(d, composite):
    """|refine.prepare_target on the CPU - target_f64| allowed (values in [0, 1])."""
    k = PREPARE_ELEMENT_ROUNDINGS[bool(composite)] + (d * d - 1) + 1
    return k * U * (1.0 + k * U) + FP64_SLACK               # the second factor covers the products of the (1 +- u)


def keep_input(best_loss_last, loss_input):
    """NOT (best_loss_last < loss_input): a NaN on either side keeps the input, and so does a tie."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(best_loss_last, F) < np.asarray(loss_input, F))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def walk(ops, torch, tensors, sh_degree, start_rows, levels, capacities, lam=0.2, **hyper):
    """sixdgs_refine_poses_levels, literally, over ops.raster_views, ops.photometric_loss, ops.raster_views_backward, ops.pose_step and
    ops.pose_rebase.  levels: dicts with width, height, steps, lr, target, intrinsics.  Every capacity must fit (asserted)."""
    views, dev = start_rows.shape[0], start_rows.device
    last = levels[-1]
    needed = [0] * len(levels)
    # 1. the input's loss at the last level
    image, count = ops.raster_views(*tensors, sh_degree, start_rows, last["width"], last["height"], want_float=True, want_u8=False,
                                    want_instances=True, max_instances=capacities[-1])
    assert count <= capacities[-1]
    needed[-1] = count
    loss_input = ops.photometric_loss(image, last["target"], lambda_dssim=lam)
    status = torch.zeros(views, dtype=torch.int32, device=dev)
    # 2. the levels
    best_rows, histories, best_loss, best_step = start_rows, [], [], []
    for l, lv in enumerate(levels):
        start = ops.pose_rebase(best_rows, lv["intrinsics"])
        state = ops.pose_state(start)                       # delta, m, v, best_* fresh ...
        state["status"] = status                            # ... status carried
        history = torch.empty(lv["steps"] + 1, views, device=dev)
        for step in range(lv["steps"] + 1):
            final = step == lv["steps"]
            image, count, fwd = ops.raster_views(*tensors, sh_degree, state["rows"], lv["width"], lv["height"], want_float=True, want_u8=False,
                                                 want_instances=True, want_state=True, max_instances=capacities[l])
            assert count <= capacities[l] and fwd[1] == capacities[l]
            if final:
                loss, d_rows = ops.photometric_loss(image, lv["target"], lambda_dssim=lam), None
            else:
                loss, grad = ops.photometric_loss(image, lv["target"], lambda_dssim=lam, want_grad=True)
                d_rows = ops.raster_views_backward(*tensors, sh_degree, state["rows"], lv["width"], lv["height"], grad, fwd, want=("cams",))[6]
            ops.pose_step(start, loss, d_rows, state, history[step], step, instances=torch.tensor([count], dtype=torch.int64, device=dev),
                          max_instances=capacities[l], evaluate_only=final, lr=lv["lr"], **hyper)
        needed[l] = max(needed[l], int(state["instances_needed"]))
        best_rows, status = state["best_rows"], state["status"]
        histories.append(history)
        best_loss.append(state["best_loss"])
        best_step.append(state["best_step"])
    # 3. the last level's best camera, or the input
    kept = ~(best_loss[-1] < loss_input)
    return {"out_rows": torch.where(kept[:, None], start_rows, best_rows), "loss_input": loss_input, "kept_input": kept.to(torch.int32),
            "best_loss": torch.stack(best_loss), "best_step": torch.stack(best_step), "history": histories, "status": status,
            "instances_needed": needed}
