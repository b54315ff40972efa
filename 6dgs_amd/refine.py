"""Pose refinement by render-and-compare: the estimator's coarse pose is moved until the scene, drawn by its own renderer from that
pose, looks like the query image.

    refine_poses(scene, images, c2w, intrinsics)      Adam on a 6-vector per view under (1 - lambda) L1 + lambda (1 - SSIM)
    refine_results(scene, cameras_info, results)      the same as a post-pass over the list test_pose_estimation returns

Two backends run the same loop.  "torch" (the default) is described next; "fused" hands the whole loop to the library
(ops.refine_poses_raw -> sixdgs_refine_poses: the same three kernels per step, the pose arithmetic as HIP kernels, nothing read back
until the end), so its iterates differ from the torch ones by rounding only.

Per step: autograd.raster_views draws every view (sixdgs_raster_views), autograd.photometric_loss compares it with the target
(sixdgs_photometric_loss, one call for loss and gradient), the rasteriser's backward gives the camera rows' gradient
(sixdgs_raster_views_backward), and torch chains it through `compose` to the 6-vector.  Views never mix: the image, the loss, the
camera gradient and Adam's update are all per view, so refining views together or one by one gives the same iterates.

The parametrisation is tools/raster_fit.py's: delta = (translation, axis-angle) applied AFTER the starting w2c, [dR R | dR t + dt], so
delta = 0 is the starting pose and the step size means the same thing wherever the camera stands.  The target is the query image
averaged over downscale x downscale blocks (a centred crop to a multiple of downscale first), and the intrinsics follow:
fx / d, fy / d, (cx - crop_x) / d, (cy - crop_y) / d -- a pixel's centre is at (x + 0.5, y + 0.5) in both images.

    level_plan(levels, W, H)                          a coarse-to-fine schedule [(downscale, steps, lr), ...] checked, with its geometry
    refine_poses(..., levels=[(8, 30, 4e-3), ...])    the loop above once per level, each level started from the one before's best pose

With `levels` the targets of all levels come from one kernel (ops.target_pyramid -> sixdgs_target_pyramid) on both backends, the pose
arithmetic of both is the library's (ops.pose_step on the torch side, under autograd's image and loss), the input
pose's loss is taken at the last level first, and a view whose last level did not end below that loss keeps its input pose: a coarse
level can carry a pose somewhere worse at full resolution, and this is what stops it.  "fused" runs the whole schedule as one library
call (ops.refine_poses_levels_raw -> sixdgs_refine_poses_levels).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from . import autograd, ops

BACKENDS = ("torch", "fused")
DEFAULT_DOWNSCALE = 4
ALPHA_MODES = ("ignore", "composite")


def rodrigues(w: torch.Tensor) -> torch.Tensor:
    """Rotation matrices [..., 3, 3] of the axis-angle vectors w [..., 3] (differentiable, fine at w = 0).  Element-wise throughout:
    a vector's matrix does not depend on the others in the batch."""
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    th = torch.sqrt(th2 + 1e-20)
    zero = torch.zeros_like(w0)
    K = torch.stack([torch.stack([zero, -w2, w1], -1), torch.stack([w2, zero, -w0], -1), torch.stack([-w1, w0, zero], -1)], -2)
    eye = torch.eye(3, device=w.device, dtype=w.dtype).expand(K.shape)
    return eye + (torch.sin(th) / th)[..., None, None] * K + ((1 - torch.cos(th)) / (th2 + 1e-20))[..., None, None] * _mm(K, K)


def _mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b for [..., 3, 3] matrices (b may be [..., 3, k]) as three element-wise products added in order: no library GEMM whose
    summation could depend on the batch."""
    return (a[..., :, 0, None] * b[..., 0, None, :] + a[..., :, 1, None] * b[..., 1, None, :]) + a[..., :, 2, None] * b[..., 2, None, :]


def compose(row: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """The camera rows [..., 16] with the rigid motions delta [..., 6] = (translation, axis-angle) applied after their w2c:
    [dR R | dR t + dt]; fx, fy, cx, cy pass through."""
    m = row[..., :12].reshape(*row.shape[:-1], 3, 4)
    dR = rodrigues(delta[..., 3:])
    moved = _mm(dR, m)                                             # [dR R | dR t]
    moved = torch.cat([moved[..., :3], moved[..., 3:] + delta[..., :3, None]], dim=-1)
    return torch.cat([moved.reshape(*row.shape[:-1], 12), row[..., 12:]], dim=-1)


def prepare_target(images_u8: torch.Tensor, downscale: int, alpha: str = "ignore", background=(1.0, 1.0, 1.0)):
    """images_u8 uint8 [V,H,W,3|4] -> (target, crop_x, crop_y): with downscale 1 the rgb bytes themselves (uint8 [V,H,W,3], which the
    loss reads as u / 255); otherwise fp32 [V,H // d,W // d,3], the mean of u / 255 over d x d blocks of the centred crop that starts at
    (crop_x, crop_y) = ((W mod d) // 2, (H mod d) // 2).  alpha says what the fourth channel of an RGBA image means: "ignore" takes the
    rgb bytes as they lie; "composite" sets the value to rgb a + (1 - a) background with a = u / 255 before the blocks are averaged --
    what test.prepare_image feeds the backbone, and what a render over that background looks like (the target is then fp32 at
    downscale 1 too).  Images without a fourth channel are the same under both."""
    if alpha not in ALPHA_MODES:
        raise ValueError(f"alpha must be one of {ALPHA_MODES} (got {alpha!r})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    d = int(downscale)
    v, h, w, _ = images_u8.shape
    composite = alpha == "composite" and images_u8.shape[3] == 4
    if d == 1 and not composite:
        return images_u8[..., :3].contiguous(), 0, 0
    hh, ww = h // d, w // d
    if hh < 1 or ww < 1:
        raise ValueError(f"downscale {d} leaves nothing of a {w} x {h} image")
    oy, ox = (h - hh * d) // 2, (w - ww * d) // 2
    crop = images_u8[:, oy:oy + hh * d, ox:ox + ww * d]
    x = crop[..., :3].float() / 255.0
    if composite:
        a = crop[..., 3:].float() / 255.0
        x = x * a + (1.0 - a) * torch.tensor([float(b) for b in background], dtype=torch.float32, device=x.device)
    if d == 1:
        return x.contiguous(), ox, oy
    return x.reshape(v, hh, d, ww, d, 3).mean(dim=(2, 4)).contiguous(), ox, oy


def scaled_intrinsics(K: torch.Tensor, downscale: int, crop_x: int, crop_y: int) -> torch.Tensor:
    """K [..., 3, 3] -> [..., 4] = (fx, fy, cx, cy) of the cropped, downscaled image."""
    d = float(downscale)
    return torch.stack([K[..., 0, 0] / d, K[..., 1, 1] / d, (K[..., 0, 2] - crop_x) / d, (K[..., 1, 2] - crop_y) / d], dim=-1)


def pose_errors(gt_c2w: torch.Tensor, pred_c2w: torch.Tensor):
    """(translation error, angular error in degrees) per pose, [V] each: the formulas test_pose_estimation's errors come from
    (pose_errors of csrc/device_math.h, the reference's error_computation.py:3-8): |t_gt - t_pred| and
    acos(clamp((trace(R_gt R_pred^-1) - 1) / 2, -1, 1)); NaN where R_pred is singular."""
    gt, pr = gt_c2w.detach().float().cpu(), pred_c2w.detach().float().cpu()
    t = (gt[..., :3, 3] - pr[..., :3, 3]).norm(dim=-1)
    ang = torch.full_like(t, float("nan"))
    for i in range(t.numel()):
        r = pr.reshape(-1, 4, 4)[i, :3, :3]
        if torch.isfinite(r).all() and float(torch.linalg.det(r)) != 0.0:
            tr = (gt.reshape(-1, 4, 4)[i, :3, :3] @ torch.linalg.inv(r)).trace()
            ang.view(-1)[i] = torch.rad2deg(torch.acos(((tr - 1.0) / 2.0).clamp(-1.0, 1.0)))
    return t, ang


def _scene_tensors(scene):
    return (scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc, scene._features_rest), int(scene.active_sh_degree)


def _stack_images(images, dev) -> torch.Tensor:
    if torch.is_tensor(images) and images.dim() == 4:
        images = list(images)
    images = list(images)
    if not images:
        raise ValueError("no images")
    out = []
    for im in images:
        t = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(np.asarray(im)))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (3, 4):
            raise ValueError(f"images must be uint8 [H,W,3|4] (got {t.dtype} {tuple(t.shape)})")
        if tuple(t.shape) != tuple(out[0].shape if out else t.shape):
            raise ValueError("images must be of one size")
        out.append(t)
    return torch.stack([t.to(dev) for t in out])


def check_poses(images, c2w, intrinsics, min_views: int = 0):
    """The poses c2w [V,4,4] and intrinsics K [3,3] or [V,3,3] of `images`, arrays or tensors -> (c2w [V,4,4], K [V,3,3]) as float32:
    finite poses, one per image, at least min_views of them.  Nothing here needs the GPU."""
    c2w = torch.as_tensor(np.asarray(c2w) if not torch.is_tensor(c2w) else c2w).detach().float()
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4) or c2w.shape[0] < min_views:
        raise ValueError(f"c2w must be [V,4,4] (got {tuple(c2w.shape)})")
    views = c2w.shape[0]
    K = torch.as_tensor(np.asarray(intrinsics) if not torch.is_tensor(intrinsics) else intrinsics).detach().float()
    if tuple(K.shape) == (3, 3):
        K = K[None].expand(views, 3, 3)
    if tuple(K.shape) != (views, 3, 3):
        raise ValueError(f"intrinsics must be [3,3] or [{views},3,3] (got {tuple(K.shape)})")
    n_images = images.shape[0] if torch.is_tensor(images) else len(images)
    if n_images != views:
        raise ValueError(f"{n_images} images for {views} poses")
    if not torch.isfinite(c2w).all():
        raise ValueError("c2w must be finite")
    return c2w, K


def posed_views(images, c2w, K, dev, downscale: int, alpha: str, background):
    """check_poses' (c2w, K) and the images -> (target, rows, width, height) on dev: prepare_target's target and the camera rows [V,16]
    = w2c rows 0..2, then the intrinsics of the cropped, downscaled image.  The 4 x 4 inversions run on the host, as
    test.gt_pose_and_intrinsics' does."""
    target, ox, oy = prepare_target(_stack_images(images, dev), downscale, alpha, background)
    rows = torch.cat([torch.linalg.inv(c2w.cpu())[:, :3, :].reshape(c2w.shape[0], 12), scaled_intrinsics(K.cpu(), downscale, ox, oy)], dim=1)
    return target, rows.to(dev).contiguous(), int(target.shape[2]), int(target.shape[1])


def _rows_to_c2w(best_rows: torch.Tensor, best_step: torch.Tensor, c2w: torch.Tensor) -> torch.Tensor:
    """The c2w [V,4,4] of the best camera rows (inverted on the host); the input pose itself where the best step is 0."""
    return _rows_to_c2w_unless(best_rows, best_step == 0, c2w)


def _rows_to_c2w_unless(rows: torch.Tensor, keep: torch.Tensor, c2w: torch.Tensor) -> torch.Tensor:
    """The c2w [V,4,4] of the camera rows (inverted on the host); the input pose c2w itself, bit for bit, where `keep` [V] is set."""
    views, dev = c2w.shape[0], c2w.device
    w2c = torch.eye(4).repeat(views, 1, 1)
    w2c[:, :3, :] = rows[:, :12].reshape(views, 3, 4).cpu()
    return torch.where(keep.to(dev)[:, None, None], c2w, torch.linalg.inv(w2c).to(dev))


MAX_LEVELS, MAX_DOWNSCALE = ops.PYRAMID_MAX_LEVELS, ops.PYRAMID_MAX_DOWNSCALE


def parse_levels(text: str):
    """"8:30:4e-3,4:30:2e-3,2:40:1e-3" -> [(8, 30, 4e-3), (4, 30, 2e-3), (2, 40, 1e-3)]: downscale:steps:lr per level, coarse to fine."""
    out = []
    for part in str(text).split(","):
        fields = part.strip().split(":")
        if len(fields) != 3:
            raise ValueError(f"a level is downscale:steps:lr (got {part!r})")
        try:
            out.append((int(fields[0]), int(fields[1]), float(fields[2])))
        except ValueError:
            raise ValueError(f"a level is downscale:steps:lr with two integers and a number (got {part!r})") from None
    return out


def level_plan(levels, width: int, height: int) -> List[dict]:
    """Check a level schedule for a width x height query and give its geometry.  levels: 1 to 8 entries (downscale, steps, lr), in the
    order they run (coarse to fine); downscale an integer in [1, 256] that leaves at least one pixel of the image, steps an integer
    >= 1, lr positive and finite.  Returns per level a dict: downscale, steps, lr, width, height (of the level's image), crop_x, crop_y
    (where its centred crop starts in the query) -- prepare_target's and scaled_intrinsics' numbers.  Needs no GPU."""
    try:
        levels = [tuple(lv) for lv in levels]
    except TypeError:
        raise ValueError(f"levels must be a sequence of (downscale, steps, lr) (got {levels!r})") from None
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"levels must have 1 to {MAX_LEVELS} entries (got {len(levels)})")
    if int(width) < 1 or int(height) < 1:
        raise ValueError(f"width and height must be positive (got {width} x {height})")
    plan = []
    for i, lv in enumerate(levels):
        if len(lv) != 3:
            raise ValueError(f"level {i} must be (downscale, steps, lr) (got {lv!r})")
        d, steps, lr = lv
        for name, x in (("downscale", d), ("steps", steps)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
                raise ValueError(f"level {i}: {name} must be a positive integer (got {x!r})")
        if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not (float(lr) > 0.0 and float(lr) < float("inf")):
            raise ValueError(f"level {i}: lr must be positive and finite (got {lr!r})")
        d, steps = int(d), int(steps)
        if d > MAX_DOWNSCALE:
            raise ValueError(f"level {i}: downscale must be at most {MAX_DOWNSCALE} (got {d})")
        w, h, ox, oy = ops.pyramid_geometry(width, height, d)
        if w < 1 or h < 1:
            raise ValueError(f"level {i}: downscale {d} leaves nothing of a {width} x {height} image")
        plan.append({"downscale": d, "steps": steps, "lr": float(lr), "width": w, "height": h, "crop_x": ox, "crop_y": oy})
    return plan


def _image_size(images):
    """(width, height) of the first image, without moving anything."""
    first = images[0] if not (torch.is_tensor(images) and images.dim() == 3) else images
    shape = tuple(first.shape) if hasattr(first, "shape") else np.asarray(first).shape
    if len(shape) != 3:
        raise ValueError(f"images must be uint8 [H,W,3|4] (got shape {shape})")
    return int(shape[1]), int(shape[0])


def _refine_levels(tensors, sh_degree, images, c2w, K, dev, plan, lambda_dssim, background, scale_modifier, backend, alpha) -> dict:
    """refine_poses with a level plan: the targets of every level from ops.target_pyramid, then the schedule on either backend."""
    views = c2w.shape[0]
    stacked = _stack_images(images, dev)
    composite = alpha == "composite" and stacked.shape[3] == 4
    targets = ops.target_pyramid(stacked, [lv["downscale"] for lv in plan], composite=composite, background=background)
    intr = [scaled_intrinsics(K.cpu(), lv["downscale"], lv["crop_x"], lv["crop_y"]).to(dev).contiguous() for lv in plan]
    start_rows = torch.cat([torch.linalg.inv(c2w.cpu())[:, :3, :].reshape(views, 12).to(dev), intr[-1]], dim=1).contiguous()
    c2w = c2w.to(dev)
    kw = dict(background=background, scale_modifier=scale_modifier)
    if backend == "fused":
        raw = ops.refine_poses_levels_raw(*tensors, sh_degree, start_rows,
                                          [dict(width=lv["width"], height=lv["height"], steps=lv["steps"], lr=lv["lr"], target=t, intrinsics=k)
                                           for lv, t, k in zip(plan, targets, intr)], lambda_dssim=float(lambda_dssim), **kw)
        kept = raw["kept_input"] != 0
        return {"c2w": _rows_to_c2w_unless(raw["out_rows"], kept, c2w), "loss_start": raw["loss_input"].clone(), "loss_best": raw["best_loss"][-1].clone(),
                "best_step": raw["best_step"][-1].to(torch.int64), "loss_history": [h.clone() for h in raw["history"]], "levels": plan,
                "loss_input": raw["loss_input"], "kept_input": kept, "level_loss_best": raw["best_loss"],
                "level_best_step": raw["best_step"].to(torch.int64), "status": raw["status"]}
    # the torch arm: autograd draws and compares, step by step from the host; the pose arithmetic and its rules are sixdgs_pose_step's,
    # the library's own, so both arms move a view by the same bits and a level starts from the same camera in both
    with torch.no_grad():
        image = autograd.raster_views(*tensors, sh_degree, start_rows, plan[-1]["width"], plan[-1]["height"], **kw)
        loss_input = autograd.photometric_loss(image, targets[-1], lambda_dssim)
    status = torch.zeros(views, dtype=torch.int32, device=dev)
    histories, level_best, level_step = [], [], []
    carried = start_rows
    for lv, target, k in zip(plan, targets, intr):
        start = ops.pose_rebase(carried, k)
        state = ops.pose_state(start)                        # delta, m, v and best_* fresh; status carried
        state["status"] = status
        history = torch.empty(lv["steps"] + 1, views, device=dev)
        for step in range(lv["steps"] + 1):
            last = step == lv["steps"]
            rows = state["rows"].detach().clone().requires_grad_(not last)
            with torch.set_grad_enabled(not last):
                image = autograd.raster_views(*tensors, sh_degree, rows, lv["width"], lv["height"], **kw)
                loss = autograd.photometric_loss(image, target, lambda_dssim)
            d_rows = None if last else torch.autograd.grad(loss.sum(), rows)[0].contiguous()
            ops.pose_step(start, loss.detach().contiguous(), d_rows, state, history[step], step, evaluate_only=last, lr=lv["lr"])
        histories.append(history)
        level_best.append(state["best_loss"])
        level_step.append(state["best_step"].to(torch.int64))
        carried = state["best_rows"]
    kept = ~(level_best[-1] < loss_input)                   # a NaN on either side and a tie keep the input
    return {"c2w": _rows_to_c2w_unless(carried, kept, c2w), "loss_start": loss_input.clone(), "loss_best": level_best[-1].clone(),
            "best_step": level_step[-1], "loss_history": histories, "levels": plan, "loss_input": loss_input, "kept_input": kept,
            "level_loss_best": torch.stack(level_best), "level_best_step": torch.stack(level_step), "status": status}


def refine_poses(scene, images, c2w, intrinsics, *, steps: int = 100, lr: float = 2e-3, lambda_dssim: float = 0.2, downscale=None,
                 background=(1.0, 1.0, 1.0), scale_modifier: float = 1.0, backend: str = "torch", alpha: str = "ignore", levels=None) -> dict:
    """Refine the poses c2w [V,4,4] of the query `images` (uint8 [H,W,3|4] arrays or GPU tensors of one size) against `scene`
    (a GaussianScene on the GPU).  intrinsics: K [3,3] or [V,3,3] as test.gt_pose_and_intrinsics gives it.  Adam (lr) for `steps`
    steps on [V,6], objective photometric_loss(raster_views(...)).sum() at 1 / downscale of the resolution (downscale None: 4).
    Returns a dict of tensors on the scene's device: c2w [V,4,4] -- per view the iterate with the lowest loss, the input pose itself
    where no step lowered it --, loss_start [V], loss_best [V], best_step [V] (int64) and loss_history [steps + 1, V].
    backend "fused" runs the loop as one library call (ops.refine_poses_raw) and adds status [V] (int32, 0 = fine; bit 0: the view met a
    loss or gradient that was not finite and stopped moving there).  alpha: prepare_target's, with this call's background.
    levels: None, or a coarse-to-fine schedule [(downscale, steps, lr), ...] (level_plan checks it).  With levels the arguments steps, lr
    are IGNORED, unchecked, and any downscale beside levels raises ValueError; every level runs the loop above from
    the level before's best pose with fresh Adam state, and the returned dict changes as follows: loss_start = loss_input [V] is the
    input pose's loss at the LAST level and loss_best [V] / best_step [V] are the last level's, so the two losses are at one
    resolution; kept_input [V] (bool) is set where NOT (loss_best < loss_input) -- there c2w is the input pose, bit for bit --;
    loss_history is a list of per-level [steps_l + 1, V] tensors; level_loss_best and level_best_step are [L, V]; levels is the plan.
    With levels BOTH backends return status [V], carried across the levels: "torch" draws and compares through autograd step by step
    from the host and hands the camera rows' gradient to the library's pose step (ops.pose_step), "fused" makes one call; the pose
    arithmetic is the same code in both, so they give the same iterates.  (Without levels "torch" keeps its own compose and Adam.)"""
    if levels is not None:
        if downscale is not None:
            raise ValueError(f"levels and downscale exclude each other (got downscale {downscale} beside levels)")
        steps, lr = 1, 1.0                                  # ignored with levels: nothing of them is checked or used
    downscale = DEFAULT_DOWNSCALE if downscale is None else downscale
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS} (got {backend!r})")
    if alpha not in ALPHA_MODES:
        raise ValueError(f"alpha must be one of {ALPHA_MODES} (got {alpha!r})")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"steps must be a positive integer (got {steps})")
    if not (float(lr) > 0.0 and float(lr) < float("inf")):
        raise ValueError(f"lr must be positive and finite (got {lr})")
    if isinstance(downscale, bool) or int(downscale) != downscale or int(downscale) < 1:
        raise ValueError(f"downscale must be a positive integer (got {downscale})")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1] (got {lambda_dssim})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    steps, downscale = int(steps), int(downscale)
    c2w, K = check_poses(images, c2w, intrinsics)
    views = c2w.shape[0]
    plan = None if levels is None else level_plan(levels, *_image_size(images))
    tensors, sh_degree = _scene_tensors(scene)
    if not tensors[0].is_cuda:
        raise RuntimeError("6dgs_amd: refine_poses needs the scene on the GPU (no CPU fallback on the product path)")
    dev = tensors[0].device
    tensors = tuple(t.detach() for t in tensors)
    if plan is not None:
        return _refine_levels(tensors, sh_degree, images, c2w, K, dev, plan, lambda_dssim, background, scale_modifier, backend, alpha)
    target, start, width, height = posed_views(images, c2w, K, dev, downscale, alpha, background)
    c2w = c2w.to(dev)
    if backend == "fused":
        raw = ops.refine_poses_raw(*tensors, sh_degree, start, width, height, target, steps=steps, lambda_dssim=float(lambda_dssim), lr=float(lr),
                                   background=background, scale_modifier=scale_modifier)
        out = _rows_to_c2w(raw["best_rows"], raw["best_step"], c2w)
        return {"c2w": out, "loss_start": raw["history"][0].clone(), "loss_best": raw["best_loss"], "best_step": raw["best_step"].to(torch.int64),
                "loss_history": raw["history"], "status": raw["status"]}
    delta = torch.zeros(views, 6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([delta], lr=float(lr))
    history = torch.empty(steps + 1, views, device=dev)
    best = torch.full((views,), float("inf"), device=dev)
    best_step = torch.zeros(views, dtype=torch.int64, device=dev)
    best_rows = start.clone()
    kw = dict(background=background, scale_modifier=scale_modifier)
    for step in range(steps + 1):
        last = step == steps
        with torch.set_grad_enabled(not last):
            rows = compose(start, delta)
            image = autograd.raster_views(*tensors, sh_degree, rows, width, height, **kw)
            loss = autograd.photometric_loss(image, target, lambda_dssim)
        with torch.no_grad():
            history[step] = loss
            better = loss < best
            best = torch.where(better, loss, best)
            best_step = torch.where(better, torch.full_like(best_step, step), best_step)
            best_rows = torch.where(better[:, None], rows.detach(), best_rows)
        if not last:
            opt.zero_grad()
            loss.sum().backward()
            opt.step()
    out = _rows_to_c2w(best_rows, best_step, c2w)
    return {"c2w": out, "loss_start": history[0].clone(), "loss_best": best, "best_step": best_step, "loss_history": history}


def refine_results(scene, cameras_info: Sequence, results: List[dict], *, batch_size: int = 8, **kw) -> List[dict]:
    """A post-pass over the list test_pose_estimation(cameras_info, ...) returned (results[i] belongs to cameras_info[i]): every
    entry with a finite pred_c2w gains refined_c2w, refined_translation_error, refined_angular_error (against its gt_c2w),
    photometric_loss_before and photometric_loss_after; existing keys are untouched.  ValueError when a camera's image is not of the
    camera's width x height (its intrinsics would not be the image's).  Views of one image size are refined
    `batch_size` at a time; kw goes to refine_poses (backend and alpha among it)."""
    from .test import gt_pose_and_intrinsics

    if len(results) != len(cameras_info):
        raise ValueError(f"{len(results)} results for {len(cameras_info)} cameras")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    groups = {}
    for i, (cam, res) in enumerate(zip(cameras_info, results)):
        if np.isfinite(np.asarray(res["pred_c2w"], np.float64)).all():
            shape = tuple(np.asarray(cam.image).shape)
            if shape[:2] != (int(cam.height), int(cam.width)):      # the intrinsics come from width, height and the field of view
                raise ValueError(f"camera {i}: its image is {shape[1]} x {shape[0]} but the camera says {cam.width} x {cam.height}")
            groups.setdefault(shape, []).append(i)
    for which in groups.values():
        for b0 in range(0, len(which), int(batch_size)):
            part = which[b0:b0 + int(batch_size)]
            pred = torch.tensor([results[i]["pred_c2w"] for i in part], dtype=torch.float32)
            gt = torch.tensor([results[i]["gt_c2w"] for i in part], dtype=torch.float32)
            Ks = torch.stack([gt_pose_and_intrinsics(cameras_info[i], "cpu")[1] for i in part])
            out = refine_poses(scene, [np.asarray(cameras_info[i].image) for i in part], pred, Ks, **kw)
            t_err, a_err = pose_errors(gt, out["c2w"])
            refined, before, after = out["c2w"].cpu(), out["loss_start"].cpu(), out["loss_best"].cpu()
            for j, i in enumerate(part):
                results[i].update(refined_c2w=refined[j].tolist(), refined_translation_error=float(t_err[j]),
                                  refined_angular_error=float(a_err[j]), photometric_loss_before=float(before[j]),
                                  photometric_loss_after=float(after[j]))
    return results
