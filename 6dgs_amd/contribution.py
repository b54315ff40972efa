"""What each Gaussian of a scene contributes to a set of views, and the two uses of it that join the scene side to the estimator.

    scene_contribution(scene, c2w, intrinsics, width, height)     weight, peak, pixels, stops, seen, inert per Gaussian
    prune_by_contribution(scene, contrib, ...)                    the scene without the Gaussians the views do not need
    generate_all_possible_rays(scene, importance=weight)          emit rays from the Gaussians a camera can see

The rasteriser's blend forms alpha T for every (pixel, Gaussian) it adds; sixdgs_raster_contrib (include/sixdgs.h) repeats that walk on
a completed forward's workspace and keeps the sum, the maximum, the number of pixels that added the Gaussian and the number of pixels it
stopped -- a direct measurement, where the backward with a hand-made gradient gave one sum, no counts, and the colour clamp in the way.
ops.scene_contrib_raw -> sixdgs_scene_contrib runs it over many views in chunks as one library call.

A Gaussian is INERT for the views when no pixel added it and it stopped none: removing it changes no pixel's walk, so the views render
to the same bytes without it (tests/test_gpu_raster_contrib.py holds that end to end).  Nothing here is on by default anywhere.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .scene import GaussianScene


def camera_rows(c2w, intrinsics) -> torch.Tensor:
    """c2w [V,4,4] and K [3,3] or [V,3,3] -> the rasteriser's camera rows [V,16] (w2c rows 0..2, fx, fy, cx, cy), float32 on the host;
    the 4 x 4 inversions run on the host, as refine.posed_views' do."""
    c2w = torch.as_tensor(np.asarray(c2w) if not torch.is_tensor(c2w) else c2w).detach().float().cpu()
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4) or c2w.shape[0] < 1:
        raise ValueError(f"c2w must be [V,4,4] with at least one view (got {tuple(c2w.shape)})")
    if not torch.isfinite(c2w).all():
        raise ValueError("c2w must be finite")
    views = c2w.shape[0]
    K = torch.as_tensor(np.asarray(intrinsics) if not torch.is_tensor(intrinsics) else intrinsics).detach().float().cpu()
    if tuple(K.shape) == (3, 3):
        K = K[None].expand(views, 3, 3)
    if tuple(K.shape) != (views, 3, 3):
        raise ValueError(f"intrinsics must be [3,3] or [{views},3,3] (got {tuple(K.shape)})")
    return torch.cat([torch.linalg.inv(c2w)[:, :3, :].reshape(views, 12), torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1)],
                     dim=1).contiguous()


def scene_contribution(scene, c2w, intrinsics, width: int, height: int, *, chunk: int = 8, sh_degree=None, scale_modifier: float = 1.0,
                       per_view: bool = False) -> dict:
    """Measure `scene` (a GaussianScene on the GPU) on the views c2w [V,4,4] with intrinsics K [3,3] or [V,3,3] at width x height,
    `chunk` views per rasteriser launch.  Returns a dict of device tensors over the N Gaussians: weight (float32, the sum of alpha T
    over all pixels of all views), peak (float32, the largest alpha T), pixels and stops (int64, pixels that added it / that it
    stopped), seen (int32, views in which some pixel added it), inert (bool, pixels == 0 and stops == 0), status (int32 [1], 0 = fine)
    and with per_view view_weight float32 [V,N], view_pixels int32 [V,N].  sh_degree None: the scene's active degree (the colour does
    not enter the result; the degree is the rasteriser's argument)."""
    if not isinstance(scene, GaussianScene):
        raise ValueError(f"scene must be a GaussianScene (got {type(scene).__name__})")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    degree = int(scene.active_sh_degree) if sh_degree is None else sh_degree
    if isinstance(degree, bool) or int(degree) != degree or not 0 <= int(degree) <= int(scene.max_sh_degree):
        raise ValueError(f"sh_degree must be in [0, {int(scene.max_sh_degree)}] (got {sh_degree!r})")
    rows = camera_rows(c2w, intrinsics)
    if not scene._xyz.is_cuda:
        raise RuntimeError("6dgs_amd: scene_contribution needs the scene on the GPU (no CPU fallback on the product path)")
    arrays = [t.detach().float().contiguous() for t in (scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc,
                                                        scene._features_rest)]
    raw = ops.scene_contrib_raw(*arrays, int(degree), rows.to(scene._xyz.device), int(width), int(height), chunk=int(chunk),
                                want_views=bool(per_view), scale_modifier=scale_modifier)
    out = {k: raw[k] for k, _ in ops.CONTRIB}
    out["inert"] = (out["pixels"] == 0) & (out["stops"] == 0)
    if per_view:
        out.update({k: raw[k] for k, _ in ops.CONTRIB_VIEWS})
    out["status"] = raw["status"]
    return out


def contribution_keep(contrib: dict, *, drop_inert: bool = True, min_peak=None, min_seen=None, keep_fraction=None) -> torch.Tensor:
    """The bool mask [N] of the Gaussians that pass every criterion given (AND): not inert (drop_inert); peak >= min_peak; seen >=
    min_seen; among the round(keep_fraction N) of largest weight, equal weights to the smaller index.  Runs where the tensors are."""
    for k in ("weight", "peak", "pixels", "stops", "seen"):
        if not isinstance(contrib, dict) or not torch.is_tensor(contrib.get(k)) or contrib[k].dim() != 1:
            raise ValueError("contrib must be the dict of scene_contribution")
    n = contrib["weight"].shape[0]
    if any(contrib[k].shape[0] != n for k in ("peak", "pixels", "stops", "seen")):
        raise ValueError("contrib's tensors disagree about the number of Gaussians")
    keep = torch.ones(n, dtype=torch.bool, device=contrib["weight"].device)
    if drop_inert:
        keep &= (contrib["pixels"] != 0) | (contrib["stops"] != 0)
    if min_peak is not None:
        if not float(min_peak) >= 0.0:
            raise ValueError(f"min_peak must not be negative (got {min_peak})")
        keep &= contrib["peak"] >= float(min_peak)
    if min_seen is not None:
        if isinstance(min_seen, bool) or int(min_seen) != min_seen or int(min_seen) < 0:
            raise ValueError(f"min_seen must be a non-negative integer (got {min_seen!r})")
        keep &= contrib["seen"] >= int(min_seen)
    if keep_fraction is not None:
        if not 0.0 <= float(keep_fraction) <= 1.0:
            raise ValueError(f"keep_fraction must be in [0, 1] (got {keep_fraction})")
        k = int(round(float(keep_fraction) * n))
        # a stable descending sort: among equal weights the smaller index comes first
        order = torch.sort(contrib["weight"], descending=True, stable=True).indices
        top = torch.zeros(n, dtype=torch.bool, device=keep.device)
        top[order[:k]] = True
        keep &= top
    return keep


def prune_by_contribution(scene, contrib: dict, *, drop_inert: bool = True, min_peak=None, min_seen=None, keep_fraction=None):
    """The scene without the Gaussians scene_contribution's measurement says the views do not need -> (new_scene, keep): keep the bool
    mask [N] of contribution_keep (the criteria combine by AND), new_scene = scene.subset(keep).  The input scene is never written."""
    if not isinstance(scene, GaussianScene):
        raise ValueError(f"scene must be a GaussianScene (got {type(scene).__name__})")
    keep = contribution_keep(contrib, drop_inert=drop_inert, min_peak=min_peak, min_seen=min_seen, keep_fraction=keep_fraction)
    if keep.shape[0] != len(scene):
        raise ValueError(f"contrib is of {keep.shape[0]} Gaussians, the scene has {len(scene)}")
    return scene.subset(keep.to(scene._xyz.device)), keep
