"""Fitting a scene's Gaussians to posed views: the scene, drawn by its own renderer from the given poses, is moved until it looks like
the given images.

    fit_scene(scene, images, c2w, intrinsics, steps=...)      Adam on the six parameter arrays under (1 - lambda) L1 + lambda (1 - SSIM)

This is the loop the reference makes a scene with (train.py:94-184, scene/gaussian_model.py:230-282 and :422-632): one Adam group
per array with its own rate (f_rest at feature_lr / 20), the exponentially decaying position rate, the SH degree that steps up every
sh_up_every iterations, the periodic opacity reset, the sampling of views without replacement and -- with densify=... -- adaptive
density control: the statistics of every pass (ops.densify_stats), and every `interval` iterations a round of clone, split and prune
(ops.densify) that changes the number of Gaussians.  Without densify the number is fixed for the whole fit.

Deviations from the reference, with densify: a round's iteration makes NO Adam update (in the reference the freshly made parameters
carry no gradient, so its optimiser steps nothing there either) and Adam's counter counts the updates actually made; the opacity
reset follows the Adam update of its iteration, as it does without densify (the reference resets first and so skips the opacity's
update on that iteration); screen_size defaults to 0, because the reference zeroes max_radii2D before it prunes and its screen-size
test never fires; the per-pass gradient statistic is the norm of the NDC-position gradient, (0.5 W du, 0.5 H dv), as include/sixdgs.h
defines it; the split's normals come from torch.randn on the host, seeded from `seed` and the round number, for both backends.

Two backends run the same loop.  "torch" (the default, the reference arm): torch.optim.Adam over six groups, autograd.raster_views and
autograd.photometric_loss.  "fused": the whole loop as one library call (ops.fit_scene_raw -> sixdgs_fit_scene: the same kernels per
step, Adam and the reset as HIP kernels, nothing read back until the end), so its iterates differ from the torch ones by Adam's
rounding order only.  With densify the fused run is cut into segments that end at the rounds' iterations: one
sixdgs_fit_scene_steps call per segment, one sixdgs_densify call per round and ONE 8-byte read of n_out behind it -- the only
read-back, at most once per `interval` steps; the torch arm runs the same schedule with torch.optim.Adam, the raw render ops (so that
ops.densify_stats can follow the backward) and the round in plain torch ops (densify_torch).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import autograd, ops
from .evaluate import evaluate_prepared
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


DENSIFY_DEFAULTS = {"from_iter": 500, "until_iter": 15000, "interval": 100, "grad_threshold": 2e-4, "percent_dense": 0.01, "min_opacity": 0.005,
                    "extent": None, "prune_big_after": 3000, "screen_size": 0, "reset_at_from_iter": False, "seed": 0}


def densify_options(densify) -> dict:
    """fit_scene's densify argument -- a dict (or an object with attributes) naming some of DENSIFY_DEFAULTS' options -- checked and
    completed with the reference's defaults.  extent None means cameras_extent of the fit's poses."""
    if not isinstance(densify, dict):
        densify = {k: getattr(densify, k) for k in DENSIFY_DEFAULTS if hasattr(densify, k)}
    unknown = sorted(set(densify) - set(DENSIFY_DEFAULTS))
    if unknown:
        raise ValueError(f"densify: unknown options {unknown} (known: {sorted(DENSIFY_DEFAULTS)})")
    o = {**DENSIFY_DEFAULTS, **densify}
    for k in ("from_iter", "until_iter", "prune_big_after", "screen_size", "seed"):
        o[k] = _int_at_least(o[k], 0, f"densify[{k!r}]")
    o["interval"] = _int_at_least(o["interval"], 1, "densify['interval']")
    for k in ("grad_threshold", "percent_dense") + (("extent",) if o["extent"] is not None else ()):
        if isinstance(o[k], bool) or not (0.0 < float(o[k]) < float("inf")):
            raise ValueError(f"densify[{k!r}] must be positive and finite (got {o[k]!r})")
        o[k] = float(o[k])
    if isinstance(o["min_opacity"], bool) or not (0.0 <= float(o["min_opacity"]) < 1.0):
        raise ValueError(f"densify['min_opacity'] must be in [0, 1) (got {o['min_opacity']!r})")
    o["min_opacity"], o["reset_at_from_iter"] = float(o["min_opacity"]), bool(o["reset_at_from_iter"])
    return o


def cameras_extent(c2w) -> float:
    """The reference's cameras_extent (scene/datasets_utils.py:7-25): 1.1 x the largest distance of a camera centre from their mean."""
    centres = np.asarray(c2w.detach().cpu() if torch.is_tensor(c2w) else c2w, dtype=np.float64)[:, :3, 3]
    return float(1.1 * np.max(np.linalg.norm(centres - centres.mean(axis=0, keepdims=True), axis=1)))


def densify_plan(steps: int, densify, opacity_reset_every: int = 0, opacity_moves: bool = True) -> dict:
    """What happens at iteration it = s + 1 of a fit, as bool arrays [steps] -- a pure host function.  densify None: every step
    updates, none accumulates or densifies, and the opacity resets after every opacity_reset_every-th iteration (today's loop).
    Otherwise, after train.py:152-184: while it < until_iter the pass's statistics are accumulated ("stats"), a round runs when
    it > from_iter and it % interval == 0 ("round"; that step makes no update, and prunes big Gaussians when it > prune_big_after:
    "prune_big"), and the opacity is reset when it % opacity_reset_every == 0 or, with reset_at_from_iter, it == from_iter ("reset").
    Resets are dropped when the opacity does not move."""
    it = np.arange(int(steps)) + 1
    every = int(opacity_reset_every)
    periodic = (it % every == 0) if every > 0 else np.zeros(int(steps), bool)
    if densify is None:
        none = np.zeros(int(steps), bool)
        plan = {"update": ~none, "stats": none, "round": none.copy(), "prune_big": none.copy(), "reset": periodic}
    else:
        o = densify_options(densify)
        active = it < o["until_iter"]
        rounds = active & (it > o["from_iter"]) & (it % o["interval"] == 0)
        reset = active & (periodic | (o["reset_at_from_iter"] & (it == o["from_iter"])))
        plan = {"update": ~rounds, "stats": active, "round": rounds, "prune_big": it > o["prune_big_after"], "reset": reset}
    if not opacity_moves:
        plan["reset"] = np.zeros(int(steps), bool)
    return plan


def round_noise(n: int, seed: int, round_no: int, device) -> torch.Tensor:
    """The standard normals [n,2,3] of round round_no (from 0) of a fit seeded with `seed`: the same numbers for both backends."""
    gen = torch.Generator().manual_seed(int(seed) * 1000003 + int(round_no))
    return torch.randn((int(n), 2, 3), generator=gen).to(device)


def _rotmat(q: torch.Tensor) -> torch.Tensor:
    """device_math.h's quat_to_rotmat in torch: q = (w, x, y, z) [n,4], normalised twice -> [n,3,3]."""
    q = q / torch.clamp(q.norm(dim=1, keepdim=True), min=1e-12)
    r, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def densify_torch(params: dict, state: dict, stats: dict, noise: torch.Tensor, *, grad_threshold, percent_dense, extent, min_opacity,
                  prune_big, screen_size: int = 0, scale_is_log: bool = True, opacity_is_logit: bool = True):
    """ops.densify in plain torch ops, after the reference's densify_and_clone, densify_and_split, densification_postfix and
    prune_points (masks, cat, indexing): the torch arm's round, and the GPU tests' second restatement.  params: the six arrays by
    name; state: name -> (exp_avg, exp_avg_sq) in the arrays' shapes, or None for a group the optimiser holds no state of -- the
    surgery of cat_tensors_to_optimizer / _prune_optimizer: zeros for what is new, the mask for what is pruned; stats:
    ops.densify_stats_state's dict; noise [n,2,3].  The thresholds are ops.densify_thresholds': compared in the stored domain.
    Returns (new params, new state, (n_out, clones, split sources, candidates pruned))."""
    t = ops.densify_thresholds(grad_threshold=grad_threshold, percent_dense=percent_dense, extent=extent, min_opacity=min_opacity,
                               scale_is_log=scale_is_log, opacity_is_logit=opacity_is_logit)
    n = params["xyz"].shape[0]
    denom = stats["denom"]
    avg = torch.where(denom > 0, stats["grad_accum"] / denom.float(), torch.zeros_like(stats["grad_accum"]))
    scale = params["scale"]
    big = scale.max(dim=1).values > t["dense"]
    selected = avg >= t["grad"]
    clone, split = selected & ~big, selected & big
    # densify_and_clone, then densify_and_split (which sees a zero gradient for the clones), then its prune of the split sources
    src = torch.cat([torch.nonzero(~split)[:, 0], torch.nonzero(clone)[:, 0], torch.nonzero(split)[:, 0], torch.nonzero(split)[:, 0]])
    n_keep, n_clone, n_split = n - int(split.sum()), int(clone.sum()), int(split.sum())
    new = {k: v[src] for k, v in params.items()}
    first_child = n_keep + n_clone
    sigma = torch.exp(scale[split]) if scale_is_log else scale[split]
    rot = _rotmat(params["rot"][split])
    for j in range(2):
        rows = slice(first_child + j * n_split, first_child + (j + 1) * n_split)
        new["xyz"][rows] = torch.bmm(rot, (sigma * noise[split, j]).unsqueeze(-1)).squeeze(-1) + params["xyz"][split]
        new["scale"][rows] = scale[split] - 0.470003629 if scale_is_log else scale[split] / torch.tensor(1.6, device=scale.device)
    original = torch.arange(src.shape[0], device=src.device) < n_keep
    radii = torch.where(original, stats["max_radii"][src], torch.zeros_like(src, dtype=torch.int32))
    # prune_points on the candidates' own stored values
    prune = new["opacity"].reshape(-1) < t["opacity"]
    if prune_big:
        prune = prune | (new["scale"].max(dim=1).values > t["world"])
        if screen_size > 0:
            prune = prune | (radii > screen_size)
    keep = ~prune
    new = {k: v[keep] for k, v in new.items()}
    new_state = {}
    for k, mv in state.items():
        new_state[k] = None if mv is None else tuple(torch.where(original.reshape(-1, *[1] * (x.dim() - 1)), x[src], torch.zeros_like(x[src]))[keep]
                                                    for x in mv)
    n_out = int(keep.sum())
    return new, new_state, (n_out, n_clone, n_split, n + n_clone + n_split - n_out)


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
              background=(1.0, 1.0, 1.0), seed: int = 0, schedule=None, densify=None, evaluate=None):
    """Fit `scene` (a GaussianScene on the GPU) to the posed `images` (uint8 [H,W,3|4] arrays or GPU tensors of one size) seen from
    c2w [V,4,4] with intrinsics K [3,3] or [V,3,3]: `steps` Adam steps, each on `batch` views, objective
    photometric_loss(raster_views(...)).sum() at 1 / downscale of the resolution.  Returns (new_scene, report): new_scene is a NEW
    GaussianScene -- the input scene is never written --, report a dict with loss_history [steps, batch] (the loss of each view BEFORE
    the step's update), views [steps, batch] (int64) and status (int32 [1]; 0 = fine, bit 0: a gradient entry was not finite and was
    left out -- the fused backend alone reports it).

    densify=None: the number of Gaussians is fixed -- today's loop, bit for bit.  Otherwise a dict (or an object with attributes) of
    DENSIFY_DEFAULTS' options, the reference's defaults: statistics are accumulated while it < until_iter (it = step + 1); when
    it > from_iter and it % interval == 0 the step makes NO Adam update (Adam's counter counts the updates actually made) and a round
    of clone / split / prune runs with grad_threshold, percent_dense, min_opacity, extent (None: cameras_extent(c2w)), big Gaussians
    pruned when it > prune_big_after, screen_size (0: off, the reference's behaviour), the split's normals from torch.randn seeded from
    densify's seed and the round number; the statistics are zeroed after a round; the opacity is reset, after the step's update or
    round, while it < until_iter when it % opacity_reset_every == 0 or, with reset_at_from_iter, it == from_iter.  report then gains
    rounds (int64 [R,6] on the host, one row per round: iteration, n before, clones, split sources, candidates pruned, n after) and
    n_final (= len(new_scene)).  The fused backend reads n_out (8 bytes) once per round and nothing else until the end.  groups: the arrays that move, among ("xyz", "f_dc", "f_rest", "opacity",
    "scale", "rot"); the others are copied unchanged.  Rates: the reference's defaults; f_rest learns at feature_lr / 20; the position
    rate is position_lr(s + 1, ...) at step s.  sh_degree_start=None renders at the scene's active degree throughout; otherwise the
    degree starts there and rises by one every sh_up_every iterations up to the scene's maximum (the new scene's active degree is the
    last one used).  opacity_reset_every=0 means never -- the default, because without densification a reset mostly harms; otherwise
    the opacity is reset to at most reset_ceiling after every opacity_reset_every-th iteration (only when "opacity" is among groups).
    schedule: int [steps, batch] view indices, overriding the default sampling without replacement (default_schedule, by seed).
    alpha, downscale, background: refine.prepare_target's.

    evaluate=None: nothing is measured -- today's loop, bit for bit.  Otherwise a dict {images, c2w, intrinsics, at, quantise=False,
    chunk=8}: held-out views (evaluate.evaluate_views' arguments; downscale, alpha and background are the fit's) and `at`, step indices
    in [0, steps].  An evaluation at s sees the scene BEFORE step s's update, at that step's SH degree; s = steps means the final
    scene.  The reference's --test_iterations k is s = k - 1 in a fit without densification, because training_report runs before
    the iteration's optimiser step.  report["evaluations"] is then a list, in ascending s, of {step, n (the Gaussians at that point),
    l1, psnr, psnr_channels, ssim}: evaluate_views' means.  The fused backends cut their run at `at` (sixdgs_fit_scene_steps segments,
    which compose to the one call bit for bit); evaluating never changes the fit."""
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
    if densify is not None:
        densify_options(densify)
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
    plan = densify_plan(steps, densify, opacity_reset_every, "opacity" in groups)
    resets = plan["reset"]
    watch = None if evaluate is None else _Evaluations(evaluate, steps, degrees, dev, downscale, alpha, background)
    views_t = torch.from_numpy(views.astype(np.int64)).to(dev)
    eps, lam = rates["eps"], float(lambda_dssim)
    if densify is not None:
        opts = densify_options(densify)
        if opts["extent"] is None:
            opts["extent"] = cameras_extent(c2w)
        run = _fit_densify_fused if backend == "fused" else _fit_densify_torch
        params, history, status, rounds = run(params, cams, width, height, target, views_t, lrs, degrees, plan, opts, groups, lam, eps,
                                              float(reset_ceiling), background, watch)
        extra = {"rounds": rounds, "n_final": int(params["xyz"].shape[0])}
    elif backend == "fused" and watch is not None:
        extra = {}
        history, status = _fit_fused_cut(params, cams, width, height, target, views, lrs, degrees, resets, groups, lam, eps,
                                         float(reset_ceiling), background, watch)
    elif backend == "fused":
        extra = {}
        raw = ops.fit_scene_raw(params, cams, width, height, target, views=views, lrs=lrs, sh_degrees=degrees, resets=resets, groups=groups,
                                lambda_dssim=lam, eps=eps, reset_ceiling=float(reset_ceiling), background=background)
        history, status = raw["history"], raw["status"]
    else:
        extra = {}
        history = torch.empty(steps, batch, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for k in groups:
            params[k].requires_grad_(True)
        opt = torch.optim.Adam([{"params": [params[k]], "lr": float(lrs[0][GROUPS.index(k)]), "name": k} for k in groups], lr=0.0, eps=eps)
        order = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")
        for s in range(steps):
            for group in opt.param_groups:
                group["lr"] = float(np.float32(lrs[s][GROUPS.index(group["name"])]))
            if watch is not None:
                watch.before(s, params)
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
    if watch is not None:
        watch.before(steps, params)
        extra["evaluations"] = watch.rows
    new = GaussianScene(max_degree)
    new.active_sh_degree = int(degrees[-1])
    for k, a in _SCENE_ATTR.items():
        setattr(new, a, params[k])
    return new, {"loss_history": history, "views": views_t, "status": status, **extra}


_ORDER = ops.SCENE_ARRAYS


class _Evaluations:
    """fit_scene's evaluate argument, checked and prepared once: before(s, params) measures the held-out views when s is in `at`."""

    KEYS = {"images", "c2w", "intrinsics", "at", "quantise", "chunk"}

    def __init__(self, spec, steps, degrees, dev, downscale, alpha, background):
        if not isinstance(spec, dict) or not {"images", "c2w", "intrinsics", "at"} <= set(spec) <= self.KEYS:
            raise ValueError(f"evaluate must be a dict with images, c2w, intrinsics, at and optionally quantise, chunk (got {spec!r:.80})")
        at = sorted({_int_at_least(s, 0, "evaluate['at']") for s in spec["at"]})
        if not at or at[-1] > steps:
            raise ValueError(f"evaluate['at'] must name step indices in [0, {steps}]")
        self.at, self.steps, self.degrees, self.background = at, steps, degrees, background
        self.quantise, self.chunk = bool(spec.get("quantise", False)), _int_at_least(spec.get("chunk", 8), 1, "evaluate['chunk']")
        c2w, K = check_poses(spec["images"], spec["c2w"], spec["intrinsics"], min_views=1)
        self.target, self.cams, self.width, self.height = posed_views(spec["images"], c2w, K, dev, downscale, alpha, background)
        self.rows = []

    def cuts(self):
        """The steps a fused run has to stop before."""
        return [s for s in self.at if 0 < s < self.steps]

    def restart(self):
        self.rows = []

    def before(self, s, params):
        if s not in self.at:
            return
        with torch.no_grad():
            r = evaluate_prepared([params[k].detach() for k in _ORDER], int(self.degrees[min(s, self.steps - 1)]), self.cams, self.width,
                                  self.height, self.target, quantise=self.quantise, chunk=self.chunk, background=self.background)
        self.rows.append({"step": int(s), "n": int(params["xyz"].shape[0]), "l1": float(r["mean_l1"]), "psnr": float(r["mean_psnr"]),
                          "psnr_channels": float(r["mean_psnr_channels"]), "ssim": float(r["mean_ssim"])})


def _fit_fused_cut(params, cams, width, height, target, views, lrs, degrees, resets, groups, lam, eps, ceiling, background, watch):
    """fit_scene's fused backend without densification, cut before the steps `watch` measures at: one sixdgs_fit_scene_steps call per
    segment from state zeroed here -- together the one sixdgs_fit_scene call, bit for bit.  status and the largest instance count are
    read once at the end; when the capacity was too small the fit runs once more from the start, as ops.fit_scene_raw does.
    params is updated in place -> (history, status)."""
    steps, batch = views.shape
    dev = cams.device
    n = params["xyz"].shape[0]
    start = {k: v.clone() for k, v in params.items()}
    ends = watch.cuts() + [steps]
    capacity = ops.raster_instances_estimate(n, batch)
    for attempt in range(2):
        state = ops.gaussian_adam_state(params)
        state["instances_needed"] = torch.zeros(1, dtype=torch.int64, device=dev)
        history = torch.empty(steps, batch, device=dev)
        watch.restart()
        first = 0
        for end in ends:
            watch.before(first, params)
            seg = slice(first, end)
            history[seg] = ops.fit_scene_steps_raw(params, cams, width, height, target, state, views=views[seg], lrs=lrs[seg],
                                                   sh_degrees=degrees[seg], resets=resets[seg], first_adam_step=first, groups=groups,
                                                   lambda_dssim=lam, eps=eps, reset_ceiling=ceiling, background=background,
                                                   max_instances=capacity)
            first = end
        flags = torch.cat([state["status"].to(torch.int64), state["instances_needed"]]).cpu()
        if not int(flags[0]) & ops.FIT_STATUS_CAPACITY:
            break
        if attempt == 1 or int(flags[1]) > ops.RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: fit_scene still needs {int(flags[1])} tile instances after {attempt + 1} runs (limit 2^31 - 1): "
                               "fit fewer views at once")
        for k, v in start.items():
            params[k].copy_(v)
        capacity = ops._grown(int(flags[1]))
    return history, state["status"]


def _round_kw(opts, prune_big):
    return dict(grad_threshold=opts["grad_threshold"], percent_dense=opts["percent_dense"], extent=opts["extent"],
                min_opacity=opts["min_opacity"], prune_big=bool(prune_big), screen_size=opts["screen_size"])


def _rounds_table(rows, dev):
    """[(iteration, n before, counts int64 [4] on the device)] -> int64 [R,6] on the host: iteration, n before, clones, split sources,
    candidates pruned, n after."""
    if not rows:
        return torch.zeros(0, 6, dtype=torch.int64)
    counts = torch.stack([torch.as_tensor(c, dtype=torch.int64, device=dev) for _, _, c in rows]).cpu()
    head = torch.tensor([[it, n] for it, n, _ in rows], dtype=torch.int64)
    return torch.cat([head, counts[:, 1:], counts[:, :1]], dim=1)


def _fit_densify_fused(start, cams, width, height, target, views_t, lrs, degrees, plan, opts, groups, lam, eps, ceiling, background, watch=None):
    """fit_scene's fused backend with densification: segments of sixdgs_fit_scene_steps that end at the rounds' iterations, one
    sixdgs_densify per round into buffers of 2 n rows (so a round never retries) and one 8-byte read of n_out behind it.  status and the
    largest instance count are read once at the end; when the capacity was too small the whole fit runs once more, from the start,
    with 5/4 of what it needed as every segment's floor."""
    steps, batch = views_t.shape
    dev = cams.device
    views = views_t.cpu().numpy().astype(np.int32)
    ends = [int(s) + 1 for s in np.nonzero(plan["round"])[0]]
    if not ends or ends[-1] != steps:
        ends.append(steps)
    if watch is not None:           # the evaluations' cut points; a segment that ends at one of them alone is no round's
        ends = sorted(set(ends) | set(watch.cuts()))
    floor = 0
    for attempt in range(2):
        params = {k: v.clone() for k, v in start.items()}
        n = params["xyz"].shape[0]
        state = ops.gaussian_adam_state(params)
        state["instances_needed"] = torch.zeros(1, dtype=torch.int64, device=dev)
        stats = ops.densify_stats_state(n, dev)
        history = torch.empty(steps, batch, device=dev)
        rows, first, updates_made = [], 0, 0
        if watch is not None:
            watch.restart()
        for end in ends:
            if watch is not None:
                watch.before(first, params)
            seg = slice(first, end)
            is_round = bool(plan["round"][end - 1])
            seg_resets = plan["reset"][seg].copy()
            reset_after_round = is_round and bool(seg_resets[-1])
            if is_round:
                seg_resets[-1] = False          # the round comes first, as in the reference: the reset follows it below
            history[seg] = ops.fit_scene_steps_raw(params, cams, width, height, target, state, views=views[seg], lrs=lrs[seg],
                                                   sh_degrees=degrees[seg], resets=seg_resets, updates=plan["update"][seg],
                                                   stats_steps=plan["stats"][seg], stats=stats, first_adam_step=updates_made, groups=groups,
                                                   lambda_dssim=lam, eps=eps, reset_ceiling=ceiling, background=background,
                                                   max_instances=max(ops.raster_instances_estimate(n, batch), floor))
            updates_made += int(plan["update"][seg].sum())
            if is_round:
                noise = round_noise(n, opts["seed"], len(rows), dev)
                params, new_state, counts = ops.densify(params, state, stats, noise, **_round_kw(opts, plan["prune_big"][end - 1]))
                rows.append((end, n, counts))
                n = params["xyz"].shape[0]
                state = {**new_state, "instances_needed": state["instances_needed"]}
                stats = ops.densify_stats_state(n, dev)
                if reset_after_round and n > 0:
                    sl = ops.gaussian_adam_slices(n, 1 + params["f_rest"].shape[1])["opacity"]
                    ops.opacity_reset(params["opacity"], state["m"][sl], state["v"][sl], ceiling=ceiling)
            first = end
        flags = torch.cat([state["status"].to(torch.int64), state["instances_needed"]]).cpu()
        if not int(flags[0]) & ops.FIT_STATUS_CAPACITY:
            break
        if attempt == 1 or int(flags[1]) > ops.RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: fit_scene still needs {int(flags[1])} tile instances after {attempt + 1} runs (limit 2^31 - 1): "
                               "fit fewer views at once")
        floor = ops._grown(int(flags[1]))
    return params, history, state["status"], _rounds_table(rows, dev)


def _fit_densify_torch(start, cams, width, height, target, views_t, lrs, degrees, plan, opts, groups, lam, eps, ceiling, background, watch=None):
    """fit_scene's torch backend with densification, the reference arm: the same schedule with torch.optim.Adam; the render pass goes
    through the raw ops so that ops.densify_stats can follow the backward; the round is densify_torch, with the optimiser-state surgery
    of the reference's cat_tensors_to_optimizer / _prune_optimizer."""
    steps, batch = views_t.shape
    dev = cams.device
    params = {k: v.clone() for k, v in start.items()}
    n = params["xyz"].shape[0]
    opt = torch.optim.Adam([{"params": [params[k]], "lr": float(lrs[0][GROUPS.index(k)]), "name": k} for k in groups], lr=0.0, eps=eps)
    stats = ops.densify_stats_state(n, dev)
    history = torch.empty(steps, batch, device=dev)
    rows = []
    want = tuple(k for k in _ORDER if k in groups)
    for s in range(steps):
        if watch is not None:
            watch.before(s, params)
        for group in opt.param_groups:
            group["lr"] = float(np.float32(lrs[s][GROUPS.index(group["name"])]))
        idx = views_t[s]
        rows_s, tgt = cams[idx].contiguous(), target[idx].contiguous()
        scene = [params[k] for k in _ORDER]
        image, radii, fwd = ops.raster_views(*scene, int(degrees[s]), rows_s, width, height, want_float=True, want_u8=False, want_radii=True,
                                             want_state=True, background=background)
        loss, grad = ops.photometric_loss(image, tgt, lambda_dssim=lam, want_grad=True)
        history[s] = loss
        if n > 0:
            bwd_ws = torch.empty(max(ops.raster_views_backward_workspace_bytes(n, batch, width, height, fwd[1]), 1), dtype=torch.uint8, device=dev)
            grads = ops.raster_views_backward(*scene, int(degrees[s]), rows_s, width, height, grad, fwd, background=background, want=want,
                                              workspace=bwd_ws)
            if plan["stats"][s]:
                ops.densify_stats(fwd, bwd_ws, radii, stats, width, height)
            if plan["update"][s]:
                for k, g in zip(ops.RASTER_GRADIENTS, grads):
                    if g is not None:
                        params[k].grad = g
                opt.step()
                opt.zero_grad(set_to_none=True)
        if plan["round"][s]:
            held = {k: opt.state.get(params[k]) for k in groups}
            state = {k: (None if not held[k] else (held[k]["exp_avg"], held[k]["exp_avg_sq"])) for k in groups}
            new, new_state, counts = densify_torch(params, state, stats, round_noise(n, opts["seed"], len(rows), dev),
                                                   **_round_kw(opts, plan["prune_big"][s]))
            rows.append((s + 1, n, counts))
            for group in opt.param_groups:
                k = group["name"]
                opt.state.pop(params[k], None)
                group["params"][0] = new[k]
                if held[k]:
                    held[k]["exp_avg"], held[k]["exp_avg_sq"] = new_state[k]
                    opt.state[new[k]] = held[k]
            params, n = new, new["xyz"].shape[0]
            stats = ops.densify_stats_state(n, dev)
        if plan["reset"][s] and n > 0:
            reset_opacity_(params["opacity"], ceiling)
            held = opt.state.get(params["opacity"])
            if held:
                held["exp_avg"].zero_()
                held["exp_avg_sq"].zero_()
    return params, history, torch.zeros(1, dtype=torch.int32, device=dev), _rounds_table(rows, dev)
