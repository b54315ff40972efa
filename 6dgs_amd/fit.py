"""Fitting a scene's Gaussians to posed views: the scene, drawn by its own renderer from the given poses, is moved until it looks like
the given images.

    fit_scene(scene, images, c2w, intrinsics, steps=...)      Adam on the six parameter arrays under (1 - lambda) L1 + lambda (1 - SSIM)

This is the loop the reference makes a scene with (train.py:94-122, scene/gaussian_model.py:230-282) WITHOUT densification: the number
of Gaussians is fixed for a whole fit -- no clone, split or prune, whose statistics the rasteriser's backward does not expose.  What is
kept: one Adam group per array with its own rate (f_rest at feature_lr / 20), the exponentially decaying position rate, the SH degree
that steps up every sh_up_every iterations, the periodic opacity reset, and the sampling of views without replacement.

Two backends run the same loop.  "torch" (the default, the reference arm): torch.optim.Adam over six groups, autograd.raster_views and
autograd.photometric_loss.  "fused": the whole loop as one library call (ops.fit_scene_raw -> sixdgs_fit_scene: the same kernels per
step, Adam and the reset as HIP kernels, nothing read back until the end), so its iterates differ from the torch ones by Adam's
rounding order only.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import autograd, ops
from .refine import ALPHA_MODES, BACKENDS, check_poses, posed_views
from .scene import GaussianScene

GROUPS = ops.FIT_GROUPS
_SCENE_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scale": "_scaling", "rot": "_rotation"}


def position_lr(iteration, lr_init: float = 1.6e-4, lr_final: float = 1.6e-6, max_steps: int = 30000, spatial_lr_scale: float = 1.0,
                delay_mult: float = 0.01, delay_steps: int = 0) -> float:
    """The position rate at `iteration` (= step + 1): log-linear from lr_init to lr_final over max_steps iterations, both times
    spatial_lr_scale: exp(log(init) (1 - t) + log(final) t), t = clip(iteration / max_steps, 0, 1).  With delay_steps > 0 the rate is
    eased in by delay_mult + (1 - delay_mult) sin(pi / 2 clip(iteration / delay_steps, 0, 1)); the fit's call leaves delay_steps at 0,
    so that factor is 1.  0 for a negative iteration or when both rates are 0."""
    init, final = float(lr_init) * float(spatial_lr_scale), float(lr_final) * float(spatial_lr_scale)
    if iteration < 0 or (init == 0.0 and final == 0.0):
        return 0.0
    delay = 1.0
    if delay_steps > 0:
        delay = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(iteration / delay_steps, 0.0), 1.0))
    t = min(max(iteration / max_steps, 0.0), 1.0)
    return delay * math.exp(math.log(init) * (1.0 - t) + math.log(final) * t)


def default_schedule(n_views: int, steps: int, batch: int = 1, seed: int = 0) -> np.ndarray:
    """View indices [steps, batch] sampled without replacement: a shuffled stack of all views is popped until it is empty, then
    refilled and shuffled again.  Reproducible by seed."""
    rng = np.random.default_rng(seed)
    stack, out = [], np.empty(steps * batch, np.int32)
    for i in range(out.size):
        if not stack:
            stack = list(rng.permutation(n_views))
        out[i] = stack.pop()
    return out.reshape(steps, batch)


def reset_opacity_(opacity: torch.Tensor, ceiling: float) -> None:
    """opacity logits -> the logit of min(sigmoid(x), ceiling), in place (the torch arm's reset)."""
    o = torch.clamp(torch.sigmoid(opacity), max=ceiling)
    opacity.copy_(torch.log(o / (1.0 - o)))


def _int_at_least(x, low, name):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < low:
        raise ValueError(f"{name} must be an integer >= {low} (got {x!r})")
    return int(x)


def _rate(x, name):
    if isinstance(x, bool) or not (0.0 <= float(x) < float("inf")):
        raise ValueError(f"{name} must be non-negative and finite (got {x!r})")
    return float(x)


def fit_scene(scene, images, c2w, intrinsics, *, steps, batch: int = 1, backend: str = "torch", groups=GROUPS, position_lr_init: float = 1.6e-4,
              position_lr_final: float = 1.6e-6, position_lr_delay_mult: float = 0.01, position_lr_max_steps: int = 30000,
              spatial_lr_scale: float = 1.0, feature_lr: float = 2.5e-3, opacity_lr: float = 0.05, scaling_lr: float = 5e-3,
              rotation_lr: float = 1e-3, eps: float = 1e-15, lambda_dssim: float = 0.2, sh_degree_start=None, sh_up_every: int = 1000,
              opacity_reset_every: int = 0, reset_ceiling: float = 0.01, downscale: int = 1, alpha: str = "ignore",
              background=(1.0, 1.0, 1.0), seed: int = 0, schedule=None):
    """Fit `scene` (a GaussianScene on the GPU) to the posed `images` (uint8 [H,W,3|4] arrays or GPU tensors of one size) seen from
    c2w [V,4,4] with intrinsics K [3,3] or [V,3,3]: `steps` Adam steps, each on `batch` views, objective
    photometric_loss(raster_views(...)).sum() at 1 / downscale of the resolution.  Returns (new_scene, report): new_scene is a NEW
    GaussianScene -- the input scene is never written --, report a dict with loss_history [steps, batch] (the loss of each view BEFORE
    the step's update), views [steps, batch] (int64) and status (int32 [1]; 0 = fine, bit 0: a gradient entry was not finite and was
    left out -- the fused backend alone reports it).

    The number of Gaussians is fixed: no densification.  groups: the arrays that move, among ("xyz", "f_dc", "f_rest", "opacity",
    "scale", "rot"); the others are copied unchanged.  Rates: the reference's defaults; f_rest learns at feature_lr / 20; the position
    rate is position_lr(s + 1, ...) at step s.  sh_degree_start=None renders at the scene's active degree throughout; otherwise the
    degree starts there and rises by one every sh_up_every iterations up to the scene's maximum (the new scene's active degree is the
    last one used).  opacity_reset_every=0 means never -- the default, because without densification a reset mostly harms; otherwise
    the opacity is reset to at most reset_ceiling after every opacity_reset_every-th iteration (only when "opacity" is among groups).
    schedule: int [steps, batch] view indices, overriding the default sampling without replacement (default_schedule, by seed).
    alpha, downscale, background: refine.prepare_target's."""
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS} (got {backend!r})")
    if alpha not in ALPHA_MODES:
        raise ValueError(f"alpha must be one of {ALPHA_MODES} (got {alpha!r})")
    steps, batch = _int_at_least(steps, 1, "steps"), _int_at_least(batch, 1, "batch")
    downscale, sh_up_every = _int_at_least(downscale, 1, "downscale"), _int_at_least(sh_up_every, 1, "sh_up_every")
    opacity_reset_every, seed = _int_at_least(opacity_reset_every, 0, "opacity_reset_every"), _int_at_least(seed, 0, "seed")
    position_lr_max_steps = _int_at_least(position_lr_max_steps, 1, "position_lr_max_steps")
    try:
        groups = tuple(groups)
    except TypeError:
        raise ValueError(f"groups must name some of {GROUPS} (got {groups!r})") from None
    if not groups or any(g not in GROUPS for g in groups) or len(set(groups)) != len(groups):
        raise ValueError(f"groups must name some of {GROUPS}, each once (got {groups})")
    rates = {k: _rate(v, k) for k, v in (("position_lr_init", position_lr_init), ("position_lr_final", position_lr_final),
                                         ("position_lr_delay_mult", position_lr_delay_mult), ("spatial_lr_scale", spatial_lr_scale),
                                         ("feature_lr", feature_lr), ("opacity_lr", opacity_lr), ("scaling_lr", scaling_lr),
                                         ("rotation_lr", rotation_lr), ("eps", eps))}
    if (rates["position_lr_init"] == 0.0) != (rates["position_lr_final"] == 0.0):
        raise ValueError("position_lr_init and position_lr_final must both be positive or both be 0")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1] (got {lambda_dssim})")
    if not 0.0 < float(reset_ceiling) < 1.0:
        raise ValueError(f"reset_ceiling must be in (0, 1) (got {reset_ceiling})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    if not isinstance(scene, GaussianScene):
        raise ValueError(f"scene must be a GaussianScene (got {type(scene).__name__})")
    max_degree = int(scene.max_sh_degree)
    if sh_degree_start is not None:
        sh_degree_start = _int_at_least(sh_degree_start, 0, "sh_degree_start")
        if sh_degree_start > max_degree:
            raise ValueError(f"sh_degree_start must be at most the scene's degree {max_degree} (got {sh_degree_start})")
    c2w, K = check_poses(images, c2w, intrinsics, min_views=1)
    n_views = c2w.shape[0]
    if schedule is None:
        views = default_schedule(n_views, steps, batch, seed)
    else:
        views = np.asarray(schedule.cpu() if torch.is_tensor(schedule) else schedule)
        if views.shape != (steps, batch) or not np.issubdtype(views.dtype, np.integer) or views.min() < 0 or views.max() >= n_views:
            raise ValueError(f"schedule must be [{steps},{batch}] integers in [0, {n_views})")
        views = views.astype(np.int32)
    if not scene._xyz.is_cuda:
        raise RuntimeError("6dgs_amd: fit_scene needs the scene on the GPU (no CPU fallback on the product path)")
    dev = scene._xyz.device
    params = {k: getattr(scene, a).detach().float().contiguous().clone() for k, a in _SCENE_ATTR.items()}
    target, cams, width, height = posed_views(images, c2w, K, dev, downscale, alpha, background)
    # the per-step schedule, the same numbers for both backends
    lrs = np.empty((steps, len(GROUPS)), np.float64)
    for s in range(steps):
        xyz_lr = position_lr(s + 1, rates["position_lr_init"], rates["position_lr_final"], position_lr_max_steps, rates["spatial_lr_scale"],
                             rates["position_lr_delay_mult"])
        lrs[s] = (xyz_lr, rates["feature_lr"], rates["feature_lr"] / 20.0, rates["opacity_lr"], rates["scaling_lr"], rates["rotation_lr"])
    if sh_degree_start is None:
        degrees = np.full(steps, int(scene.active_sh_degree), np.int32)
    else:       # the reference raises the degree at the START of every sh_up_every-th iteration
        degrees = np.minimum(sh_degree_start + (np.arange(steps) + 1) // sh_up_every, max_degree).astype(np.int32)
    resets = np.zeros(steps, bool)
    if opacity_reset_every > 0 and "opacity" in groups:
        resets = (np.arange(steps) + 1) % opacity_reset_every == 0
    views_t = torch.from_numpy(views.astype(np.int64)).to(dev)
    eps, lam = rates["eps"], float(lambda_dssim)
    if backend == "fused":
        raw = ops.fit_scene_raw(params, cams, width, height, target, views=views, lrs=lrs, sh_degrees=degrees, resets=resets, groups=groups,
                                lambda_dssim=lam, eps=eps, reset_ceiling=float(reset_ceiling), background=background)
        history, status = raw["history"], raw["status"]
    else:
        history = torch.empty(steps, batch, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for k in groups:
            params[k].requires_grad_(True)
        opt = torch.optim.Adam([{"params": [params[k]], "lr": float(lrs[0][GROUPS.index(k)]), "name": k} for k in groups], lr=0.0, eps=eps)
        order = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")
        for s in range(steps):
            for group in opt.param_groups:
                group["lr"] = float(np.float32(lrs[s][GROUPS.index(group["name"])]))
            idx = views_t[s]
            image = autograd.raster_views(*[params[k] for k in order], int(degrees[s]), cams[idx].contiguous(), width, height, background=background)
            loss = autograd.photometric_loss(image, target[idx].contiguous(), lam)
            history[s] = loss.detach()
            opt.zero_grad(set_to_none=True)
            loss.sum().backward()
            opt.step()
            if resets[s]:
                with torch.no_grad():
                    reset_opacity_(params["opacity"], float(reset_ceiling))
                    state = opt.state[params["opacity"]]
                    state["exp_avg"].zero_()
                    state["exp_avg_sq"].zero_()
        params = {k: v.detach() for k, v in params.items()}
    new = GaussianScene(max_degree)
    new.active_sh_degree = int(degrees[-1])
    for k, a in _SCENE_ATTR.items():
        setattr(new, a, params[k])
    return new, {"loss_history": history, "views": views_t, "status": status}
