"""Scoring a scene on held-out views: how close its renders are to images it was not fitted to.

    evaluate_views(scene, images, c2w, intrinsics)      L1, SSIM, MSE and PSNR per view and their means

The views are rasterised and measured on the GPU in chunks, as one library call (ops.evaluate_views_raw -> sixdgs_evaluate_views);
the only read-back is the [V,6] table of per-view numbers at the end.  The definitions are the reference's two:

  quantise=True   metrics.py:69-89 -- renders and ground truth pass through an 8-bit PNG (render.py:25-40: torchvision's save_image,
                  then to_tensor) before SSIM and PSNR are formed, and the means are torch.tensor(values).mean() in fp32.
  quantise=False  train.py:233-289's training_report -- both sides clamped to [0, 1], L1 and PSNR.

PSNR is derived here from the device's fp32 mse in fp64: psnr = float32(10 log10(1 / mse)), metrics.py's psnr of a [1,3,H,W] pair
(utils/image_utils.py:19-23 with the whole image as one batch entry); psnr_channels = the mean of the three per-channel PSNRs, what
train.py:275 prints, because image_utils.psnr on a [3,H,W] tensor takes the channel as the batch.  mse == 0 gives +inf, as the
reference does.  LPIPS (metrics.py:77) is absent: it needs VGG weights, and none can be had offline.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .refine import ALPHA_MODES, check_poses, posed_views
from .scene import GaussianScene

FIELDS = ("l1", "ssim", "mse", "psnr", "psnr_channels")


def psnr_of_mse(mse) -> np.ndarray:
    """float32(10 log10(1 / mse)) per entry, the logarithm in fp64 from the fp32 mse; +inf where mse == 0."""
    m = np.asarray(mse, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(1.0 / m)).astype(np.float32)


def psnr_of_channels(mse_rgb) -> np.ndarray:
    """mse_rgb [..., 3] -> the mean of the three channels' PSNRs, formed in fp64 and rounded to float32 once."""
    m = np.asarray(mse_rgb, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(1.0 / m)).mean(axis=-1).astype(np.float32)


def mean_f32(values) -> np.float32:
    """The fp32 mean of per-view values as metrics.py:85-87 forms it: torch.tensor(values).mean()."""
    t = torch.from_numpy(np.ascontiguousarray(values, np.float32))
    return np.float32(t.mean().item()) if t.numel() else np.float32("nan")


def summarise(metrics: np.ndarray) -> dict:
    """ops.METRICS' table [V,6] on the host -> the per-view arrays of FIELDS and their mean_*."""
    out = {"l1": metrics[:, 0].copy(), "ssim": metrics[:, 1].copy(), "mse": metrics[:, 2].copy(), "psnr": psnr_of_mse(metrics[:, 2]),
           "psnr_channels": psnr_of_channels(metrics[:, 3:6])}
    out.update({"mean_" + k: mean_f32(out[k]) for k in FIELDS})
    return out


def evaluate_prepared(arrays, sh_degree: int, cams, width: int, height: int, target, *, quantise, chunk, background, return_renders=False) -> dict:
    """evaluate_views behind the preparation: arrays in ops.SCENE_ARRAYS' order, camera rows [V,16] and a target as posed_views makes them."""
    raw = ops.evaluate_views_raw(*arrays, int(sh_degree), cams, width, height, target, quantise=bool(quantise), chunk=chunk,
                                 want_render=return_renders, background=background)
    out = summarise(raw["metrics"].cpu().numpy())
    out["status"] = int(raw["status"].item())
    if return_renders:
        out["renders"] = raw["render"]
    return out


def evaluate_views(scene, images, c2w, intrinsics, *, quantise: bool = True, chunk: int = 8, downscale: int = 1, alpha: str = "ignore",
                   background=(1.0, 1.0, 1.0), sh_degree=None, return_renders: bool = False) -> dict:
    """Measure `scene` (a GaussianScene on the GPU) against the posed `images` (uint8 [H,W,3|4] arrays or GPU tensors of one size) seen
    from c2w [V,4,4] with intrinsics K [3,3] or [V,3,3], `chunk` views per rasteriser launch.  quantise=True is metrics.py's definition
    (the 8-bit PNG round trip of render.py before the comparison), False train.py's training_report (a clamp to [0, 1]); the module's
    docstring says which reference line each number belongs to.  sh_degree None: the scene's active degree.  alpha, downscale,
    background: refine.prepare_target's.  Returns a dict: the fp32 arrays [V] l1, ssim, mse, psnr, psnr_channels; mean_l1 .. the fp32
    mean of each; status (0 = fine); and with return_renders renders, uint8 [V,H,W,3] on the GPU: the bytes a PNG of the render holds."""
    if alpha not in ALPHA_MODES:
        raise ValueError(f"alpha must be one of {ALPHA_MODES} (got {alpha!r})")
    if isinstance(downscale, bool) or int(downscale) != downscale or int(downscale) < 1:
        raise ValueError(f"downscale must be a positive integer (got {downscale!r})")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    if not isinstance(scene, GaussianScene):
        raise ValueError(f"scene must be a GaussianScene (got {type(scene).__name__})")
    degree = int(scene.active_sh_degree) if sh_degree is None else sh_degree
    if isinstance(degree, bool) or int(degree) != degree or not 0 <= int(degree) <= int(scene.max_sh_degree):
        raise ValueError(f"sh_degree must be in [0, {int(scene.max_sh_degree)}] (got {sh_degree!r})")
    c2w, K = check_poses(images, c2w, intrinsics, min_views=1)
    if not scene._xyz.is_cuda:
        raise RuntimeError("6dgs_amd: evaluate_views needs the scene on the GPU (no CPU fallback on the product path)")
    dev = scene._xyz.device
    target, cams, width, height = posed_views(images, c2w, K, dev, int(downscale), alpha, background)
    arrays = [t.detach().float().contiguous() for t in (scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc,
                                                        scene._features_rest)]
    return evaluate_prepared(arrays, int(degree), cams, width, height, target, quantise=quantise, chunk=int(chunk), background=background,
                             return_renders=return_renders)
