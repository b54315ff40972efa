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
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from . import autograd, ops

BACKENDS = ("torch", "fused")
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
    views, dev = c2w.shape[0], c2w.device
    w2c = torch.eye(4).repeat(views, 1, 1)
    w2c[:, :3, :] = best_rows[:, :12].reshape(views, 3, 4).cpu()
    return torch.where((best_step == 0)[:, None, None], c2w, torch.linalg.inv(w2c).to(dev))


def refine_poses(scene, images, c2w, intrinsics, *, steps: int = 100, lr: float = 2e-3, lambda_dssim: float = 0.2, downscale: int = 4,
                 background=(1.0, 1.0, 1.0), scale_modifier: float = 1.0, backend: str = "torch", alpha: str = "ignore") -> dict:
    """Refine the poses c2w [V,4,4] of the query `images` (uint8 [H,W,3|4] arrays or GPU tensors of one size) against `scene`
    (a GaussianScene on the GPU).  intrinsics: K [3,3] or [V,3,3] as test.gt_pose_and_intrinsics gives it.  Adam (lr) for `steps`
    steps on [V,6], objective photometric_loss(raster_views(...)).sum() at 1 / downscale of the resolution.
    Returns a dict of tensors on the scene's device: c2w [V,4,4] -- per view the iterate with the lowest loss, the input pose itself
    where no step lowered it --, loss_start [V], loss_best [V], best_step [V] (int64) and loss_history [steps + 1, V].
    backend "fused" runs the loop as one library call (ops.refine_poses_raw) and adds status [V] (int32, 0 = fine; bit 0: the view met a
    loss or gradient that was not finite and stopped moving there).  alpha: prepare_target's, with this call's background."""
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
    tensors, sh_degree = _scene_tensors(scene)
    if not tensors[0].is_cuda:
        raise RuntimeError("6dgs_amd: refine_poses needs the scene on the GPU (no CPU fallback on the product path)")
    dev = tensors[0].device
    tensors = tuple(t.detach() for t in tensors)
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
