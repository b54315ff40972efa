"""train_id_module -- the on-box training of the scorer (pose_estimation/train.py:16-317), SURVEY 8(f)#1.

No pretrained id_module.th ships with the reference: every scene trains its own IdentificationModule for 1500 iterations of 32
accumulated single-image steps on rays re-emitted every 10 iterations.  The loop below follows the reference step for step
(same sampling calls in the same order, same loss terms and weights, same optimiser, same checkpoint layout) on top of this
build's pieces: rays from the HIP emitter (`rays_generator` is `functools.partial(generate_all_possible_rays, model)` as in
pretrain_eval_attention.py:73), the differentiable `IdentificationModule.forward` (PyTorch-ROCm autograd), the HIP target
scores of `DistanceBasedScoreLoss`, and the HIP inference path for the periodic evaluation (`test_pose_estimation`).
TensorBoard logging is optional (the package is not a dependency): without it the scalars go to `log_fn` / nowhere.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import ops
from .distance_based_loss import DistanceBasedScoreLoss
from .test import gt_pose_and_intrinsics, test_pose_estimation


class _NoWriter:
    def add_text(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass


def _writer():
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter()
    except Exception:
        return _NoWriter()


def prepare_training_image(image, device):
    """train.py:109-121: uint8 [H,W,3|4] -> fp32 image in [0,1] (RGBA composited on white) and the alpha > 0.3 mask."""
    img = torch.from_numpy(np.array(image)).to(device=device, dtype=torch.float32) / 255.0
    if img.shape[-1] == 4:
        mask = img[..., -1] > 0.3
        img = torch.multiply(img[..., :3], img[..., -1:]) + (1 - img[..., -1:])
    else:
        mask = torch.ones_like(img[..., -1], dtype=torch.bool, device=device)
    return img, mask


def training_step_loss(id_module, loss_fn, camera_info, rays_ori, rays_dirs, rays_rgb, model_up, device):
    """One accumulated step (train.py:106-170): forward on one training image, score loss + 0.1 x camera-up loss.
    Returns (combined loss, score loss, camera-up loss) as tensors (combined may be NaN: the caller skips it)."""
    img, mask = prepare_training_image(camera_info.image, device)
    c2w, K = gt_pose_and_intrinsics(camera_info, device)
    scores, attn_map, _, up, rays_idx = id_module(img, mask, rays_ori, rays_dirs, rays_rgb)
    loss_score, _ = loss_fn(scores, c2w.to(device), K.to(device), rays_ori[rays_idx], rays_dirs[rays_idx], attn_map.shape[-2],
                            id_module.backbone_wrapper.backbone_wh, model_up=model_up)
    cam_up = -0.5 * torch.cosine_similarity(model_up, up, dim=-1) + 0.5
    return loss_score + 0.1 * cam_up, loss_score, cam_up


class _GateGrad(torch.autograd.Function):
    """Identity in the forward; the backward passes the gradient of image b ([B, ...], first axis) only where keep[b], and an exact 0
    elsewhere -- whatever the upstream value is (0 x NaN from a skipped image's loss stays out of the scorer's backward)."""

    @staticmethod
    def forward(ctx, x, keep):
        ctx.save_for_backward(keep)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        return torch.where(keep.view(-1, *([1] * (g.dim() - 1))), g, torch.zeros_like(g)), None


def window_step_loss(id_module, imgs, masks, poses, rays_ori, rays_dirs, rays_rgb, model_up, gradient_accumulation_steps: int, ray_groups: int = 1):
    """The accumulated steps of one iteration as ONE window (train_id_module(batched_window=True)): forward_window on all images, the
    targets of ops.distance_target, per image score loss + 0.1 x camera-up loss, and their sum over the images whose combined loss is
    finite, divided by gradient_accumulation_steps -- the value whose gradient the per-image loop accumulates (a data-parallel rank passes
    its block of the draws and the GLOBAL gradient_accumulation_steps: the ranks' losses and gradients sum to the iteration's).  An image whose combined
    loss is not finite contributes exactly 0 to every gradient (the per-image loop's `continue`): its gradients are gated before they
    reach the scorer's backward and the camera-up head.  poses [B,4,4] on the device.  Returns (loss, the logged sums [3] = (sum of the
    finite combined losses, their camera-up and score terms / gradient_accumulation_steps), finite [B]); nothing is read on the host.
    ray_groups: the split of the scorer's backward over the rays (forward_window; 1 = unsplit, 0 = auto)."""
    scores, up, n_host = id_module.forward_window(imgs, masks, rays_ori, rays_dirs, rays_rgb, ray_groups)
    target = torch.stack([ops.distance_target(rays_ori, rays_dirs, poses[i], n) for i, n in enumerate(n_host)])

    def terms(s, u):
        loss_score = torch.square(s - target).mean(dim=-1)
        cam_up = -0.5 * torch.cosine_similarity(model_up[None], u, dim=-1) + 0.5
        return loss_score, cam_up

    with torch.no_grad():
        ls, cu = terms(scores, up)
        finite = torch.isfinite(ls + 0.1 * cu)
    loss_score, cam_up = terms(_GateGrad.apply(scores, finite), _GateGrad.apply(up, finite))
    zero = torch.zeros_like(loss_score)
    combined = torch.where(finite, loss_score + 0.1 * cam_up, zero)
    loss = combined.sum() / gradient_accumulation_steps
    with torch.no_grad():
        logs = torch.stack([combined.sum(), torch.where(finite, cam_up, zero).sum() / gradient_accumulation_steps,
                            torch.where(finite, loss_score, zero).sum() / gradient_accumulation_steps])
    return loss, logs, finite


def train_id_module(ckpt_path, device, id_module, rays_generator: Optional[Callable[[], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]],
                    scene_info, sequence_id, category_id, start_iterations: int = 0, renewal_every_n_iterations: int = 10,
                    display_every_n_iterations: int = 20, val_every_n_iterations: int = 20, n_iterations: int = 1500,
                    gradient_accumulation_steps: int = 32, lock_backbone: bool = True, log_fn: Optional[Callable[[str, float, int], None]] = None,
                    batched_window: bool = False, data_parallel: bool = False, backward_ray_groups: int = 1):
    """batched_window: every iteration's gradient_accumulation_steps images go through ONE window (window_step_loss: one ray-MLP forward
    and backward instead of one per image, the image side as one batch, no host read before optimizer.step()) instead of the
    reference's per-image loop.  Same image draw, loss, optimiser and checkpoint; needs lock_backbone (the backbone has no backward).

    data_parallel (needs batched_window; every rank of the process group calls this): the window of each iteration is split over the
    ranks.  Rank 0 alone emits the rays and draws the images, with the random numbers of a single-rank run, and broadcasts both (the rays
    at every renewal, the draw every iteration); rank r scores its block dd.shard_range(gradient_accumulation_steps, r, world) of the draw
    against the full divisor, and dd.sum_gradients adds the ranks' gradients and logged sums in ONE all-reduce, after which every rank
    steps its optimiser on the same bits (the parameters stay identical without a broadcast).  A rank whose window step raises
    RuntimeError makes every rank raise together.  Evaluation and checkpoint stay on rank 0; the others wait in the next collective, on
    the long-wait group.  Without a process group, or at world 1: the plain window.
    backward_ray_groups: the split of the scorer's backward over the rays in the window (ops.score_backward: 1 = unsplit, 0 = auto)."""
    from . import distributed as dd

    if batched_window and not lock_backbone:
        raise ValueError("batched_window=True needs lock_backbone=True: the batched image side runs the backbone without autograd")
    if data_parallel and not batched_window:
        raise ValueError("data_parallel=True needs batched_window=True: the ranks split the window of each iteration")
    if int(backward_ray_groups) < 0:
        raise ValueError(f"backward_ray_groups must be >= 0 (got {backward_ray_groups})")
    dp = data_parallel and dd.is_dist() and dd.world() > 1
    rank, world = (dd.rank(), dd.world()) if dp else (0, 1)
    if dp and world > gradient_accumulation_steps:
        raise ValueError(f"data_parallel=True over {world} ranks needs at least as many images per iteration (gradient_accumulation_steps = "
                         f"{gradient_accumulation_steps})")
    from transformers.optimization import Adafactor        # the reference's optimiser (train.py:13,42-47), default arguments

    id_module.train()
    extra = []
    if lock_backbone:
        id_module.backbone_wrapper.eval()
    else:
        extra = list(id_module.backbone_wrapper.parameters())
    params = (list(id_module.ray_preprocessor.parameters()) + list(id_module.attention.parameters())
              + list(id_module.camera_direction_prediction_network.parameters()) + extra)
    optimizer = Adafactor(params)
    loss_fn = DistanceBasedScoreLoss()
    writer = _writer()
    for k, v in (("ckpt_path", ckpt_path), ("category_id", category_id), ("sequence_id", sequence_id)):
        writer.add_text("config/" + k, str(v))

    def log(tag, value, step):
        writer.add_scalar(tag, value, global_step=step)
        if log_fn is not None:
            log_fn(tag, float(value), step)

    model_up = torch.from_numpy(np.mean(np.asarray([c.R[:3, 1] for c in scene_info.train_cameras], dtype=np.float32), axis=0)).to(device)
    if batched_window:      # the training images on the device once: (image, mask or None when there is no alpha channel), and the poses
        window = [(img, mask if np.asarray(c.image).shape[-1] == 4 else None)
                  for c in scene_info.train_cameras for img, mask in [prepare_training_image(c.image, device)]]
        window_poses = torch.stack([gt_pose_and_intrinsics(c, device)[0] for c in scene_info.train_cameras]).to(device)
    rays_ori = rays_dirs = rays_rgb = None
    running_loss = 0.0
    lo, hi = dd.shard_range(gradient_accumulation_steps, rank, world)
    pending = None          # data-parallel rank 0: an exception of its own work between two collectives (emission, draw, evaluation)
    for iteration in range(start_iterations, n_iterations):
        renew = iteration % renewal_every_n_iterations == 0
        if not dp:
            if renew:
                rays_ori, rays_dirs, rays_rgb = rays_generator()
            optimizer.zero_grad()
            img_idx = torch.randint(0, len(scene_info.train_cameras), (gradient_accumulation_steps,), dtype=torch.long, device=device)
        else:
            # rank 0 emits and draws (the random numbers of a single-rank run) and broadcasts [failure flag, draw]; then, at a renewal, the
            # R x 9 floats of the rays (R first).  A failure of rank 0 reaches every rank through the flag: all raise at the same point.
            ctl = torch.zeros(gradient_accumulation_steps + 1, dtype=torch.long, device=device)
            if rank == 0 and pending is None:
                try:
                    fresh = torch.cat(rays_generator(), dim=-1) if renew else None
                    ctl[1:] = torch.randint(0, len(scene_info.train_cameras), (gradient_accumulation_steps,), dtype=torch.long, device=device)
                except Exception as e:  # noqa: BLE001 -- re-raised below, after the ranks have met
                    pending = e
            if rank == 0 and pending is not None:
                ctl[0] = 1
            ctl = dd.broadcast_tensor(ctl, 0, device, dtype=torch.long, shape=(gradient_accumulation_steps + 1,))
            if int(ctl[0]):
                if pending is not None:
                    raise pending
                raise RuntimeError(f"6dgs_amd: rank 0 failed before training iteration {iteration}; rank {rank} leaves the scene with it")
            if renew:
                rays = dd.broadcast_tensor(fresh if rank == 0 else None, 0, device)
                rays_ori, rays_dirs, rays_rgb = (rays[:, i: i + 3].contiguous() for i in (0, 3, 6))
            optimizer.zero_grad()
            img_idx = ctl[1:]
        if dp:
            err = None
            try:
                idx = img_idx[lo:hi].tolist()
                loss, logs, _ = window_step_loss(id_module, [window[i][0] for i in idx], [window[i][1] for i in idx], window_poses[img_idx[lo:hi]],
                                                 rays_ori, rays_dirs, rays_rgb, model_up, gradient_accumulation_steps, backward_ray_groups)
                loss.backward()
            except Exception as e:      # noqa: BLE001 -- this rank contributes zeros and the flag; every rank raises after the reduce
                err, logs = e, torch.zeros(3, device=device)
            try:
                logs = dd.sum_gradients(params, logs, failed=err is not None)
            except RuntimeError:
                if err is not None:                     # the failing rank re-raises its own exception, the others the peers' RuntimeError
                    raise err
                raise
            optimizer.step()
            acc_loss, acc_up, acc_score = logs.tolist()
        elif batched_window:
            idx = img_idx.tolist()                                      # the draw on the host, once
            loss, logs, _ = window_step_loss(id_module, [window[i][0] for i in idx], [window[i][1] for i in idx], window_poses[img_idx],
                                             rays_ori, rays_dirs, rays_rgb, model_up, gradient_accumulation_steps, backward_ray_groups)
            loss.backward()
            optimizer.step()
            acc_loss, acc_up, acc_score = logs.tolist()                 # the logged scalars, read once per iteration
        else:
            acc_loss = acc_up = acc_score = 0.0
            for step in range(gradient_accumulation_steps):
                cam = scene_info.train_cameras[img_idx[step]]
                combined, loss_score, cam_up = training_step_loss(id_module, loss_fn, cam, rays_ori, rays_dirs, rays_rgb, model_up, device)
                if combined.isnan().any():
                    continue
                (combined / gradient_accumulation_steps).backward()
                acc_loss += combined.item()
                acc_up += cam_up.item() / gradient_accumulation_steps
                acc_score += loss_score.item() / gradient_accumulation_steps
            optimizer.step()
        id_module.invalidate_caches()                 # the inference-side packed weights / key cache follow the parameters
        log("train/loss", acc_loss, iteration)
        log("train/cam_up", acc_up, iteration)
        log("train/loss_score", acc_score, iteration)
        running_loss += acc_loss
        if iteration % display_every_n_iterations == display_every_n_iterations - 1:
            if rank == 0:
                print(f"[{iteration}] loss: {running_loss / display_every_n_iterations}")
            running_loss = 0.0
        if iteration % val_every_n_iterations == val_every_n_iterations - 1 and rank == 0:
            try:
                for split, cams in (("train", scene_info.train_cameras), ("val", scene_info.test_cameras)):
                    print(f"Eval on {'validation' if split == 'val' else split}...")
                    _, te, ae, sc, rc = test_pose_estimation(cams, id_module, rays_ori, rays_dirs, rays_rgb, model_up, sequence_id=sequence_id,
                                                             category_id=category_id, loss_fn=loss_fn)
                    for tag, v in (("avg_translation_error", te), ("avg_angular_error", ae), ("avg_loss_score", sc), ("recall", rc)):
                        log(f"{split}/{tag}", v, iteration)
            except Exception as e:      # noqa: BLE001 -- data-parallel, not the last iteration: the peers wait in the next broadcast
                if not dp or iteration == n_iterations - 1:
                    raise
                pending = e
            id_module.train()
            if lock_backbone:
                id_module.backbone_wrapper.eval()
    if rank != 0:                                       # the checkpoint is rank 0's (the parameters are the same bits on every rank)
        return
    torch.save({"epoch": n_iterations, "model_state_dict": id_module.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                "running_loss": running_loss}, ckpt_path)
