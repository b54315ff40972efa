"""render_views -- views of a GaussianScene, by one of two renderers:

  "disc"    ops.splat_views: the Gaussians as z-buffered flat discs (the default; described below)
  "raster"  ops.raster_views: the alpha-blended 3DGS forward rasteriser -- anisotropic footprints from each Gaussian's scale and
            rotation, its opacity, front-to-back blending over 16 x 16 tiles; the views the scene's own renderer gives

No real scenes or checkpoints ship with this build, and `synthetic.make_cameras` fills its images with random bytes: nothing in them
depends on the camera, so a scorer cannot learn a pose from them.  The views rendered here do depend on it -- every pixel carries the SH
colour of the nearest Gaussian towards the camera, the colour the ray emitter gives a ray from that Gaussian to the camera -- which is
what training a stand-in scene needs.  The disc renderer is a stand-in view generator, not the 3DGS rasteriser (no blending, no
anisotropic footprints, no anti-aliasing); renderer="raster" is that rasteriser.

The camera of a rendered view is the camera `test.gt_pose_and_intrinsics` derives from the same CameraInfo (w2c = [R^T | T],
fx = fov2focal(FovX, width), principal point at the image centre): the image and the ground-truth pose of the loss and of the error
metrics belong to one camera.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .scene import CameraInfo, GaussianScene
from .test import fov2focal

WORKSPACE_BUDGET = 1 << 30       # bytes of depth buffer + colours per launch: sizes the batches of views


def _field(cam, name):
    return cam[name] if isinstance(cam, dict) else getattr(cam, name)


def camera_rows(cameras: Sequence) -> np.ndarray:
    """[V,16] fp32: w2c rows 0..2 (= [R^T | T], 12 floats), fx, fy, cx, cy -- the camera of test.gt_pose_and_intrinsics."""
    out = np.empty((len(cameras), 16), np.float32)
    for i, c in enumerate(cameras):
        rot, t = np.asarray(_field(c, "R"), np.float64), np.asarray(_field(c, "T"), np.float64).reshape(-1)
        if rot.shape != (3, 3) or t.shape != (3,):
            raise ValueError(f"camera {i}: R must be 3 x 3 and T of length 3 (got {rot.shape}, {t.shape})")
        w, h = int(_field(c, "width")), int(_field(c, "height"))
        out[i, :12] = np.concatenate([rot.T, t[:, None]], axis=1).reshape(-1)
        out[i, 12:] = (fov2focal(_field(c, "FovX"), w), fov2focal(_field(c, "FovY"), h), w / 2, h / 2)
    return out


def _as_camera_info(cam, image) -> CameraInfo:
    if isinstance(cam, dict):
        return CameraInfo(**{**{k: cam[k] for k in CameraInfo._fields}, "image": image})
    return cam._replace(image=image)


@torch.no_grad()
def render_views(scene: GaussianScene, cameras: Sequence, *, rgba: bool = False, extent: float = 1.0, near_z: float = 0.05,
                 background=(1.0, 1.0, 1.0), batch_size: Optional[int] = None, return_device: bool = False, renderer: str = "disc",
                 scale_modifier: float = 1.0) -> List[CameraInfo]:
    """New CameraInfos (same poses and intrinsics) whose `image` is the rendered uint8 array [height, width, 3 | 4].
    cameras: CameraInfos or the dicts of synthetic.make_cameras.  rgba: alpha 255 on covered pixels, 0 on the background, so that the
    backbone wrapper's mask -> token selection sees the silhouette.  Views of one size are rendered `batch_size` per launch (default: as
    many as fit WORKSPACE_BUDGET); the images do not depend on it.  return_device: also return the images as uint8 GPU tensors.
    renderer="raster": the 3DGS rasteriser instead of the discs; it uses the scene's rotations and opacities and scale_modifier, ignores
    extent and near_z (its near plane is 0.2), and with rgba the alpha channel is round(255 (1 - T))."""
    if renderer not in ("disc", "raster"):
        raise ValueError(f"renderer must be 'disc' or 'raster' (got {renderer!r})")
    if not (float(scale_modifier) > 0.0 and float(scale_modifier) < float("inf")):
        raise ValueError(f"scale_modifier must be positive and finite (got {scale_modifier})")
    if not (float(extent) > 0.0 and float(extent) < float("inf")):
        raise ValueError(f"extent must be positive and finite (got {extent})")
    if not float(near_z) >= 0.0:
        raise ValueError(f"near_z must be >= 0 (got {near_z})")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    cameras = list(cameras)
    rows = camera_rows(cameras)
    if not scene.get_xyz.is_cuda:
        raise RuntimeError("6dgs_amd: render_views needs the scene on the GPU (no CPU fallback on the product path)")
    sizes = [(int(_field(c, "width")), int(_field(c, "height"))) for c in cameras]
    dev = scene.get_xyz.device
    n = len(scene)
    images: List[Optional[torch.Tensor]] = [None] * len(cameras)
    for size in sorted(set(sizes)):
        which = [i for i, s in enumerate(sizes) if s == size]
        if renderer == "raster":
            per_view = max(ops.raster_views_workspace_bytes(n, 1, *size, ops.raster_instances_estimate(n, 1)), 1)
            step = int(batch_size) if batch_size is not None else max(1, WORKSPACE_BUDGET // per_view)
            per_view_instances = ops.raster_instances_estimate(n, 1)
            for b0 in range(0, len(which), step):
                part = which[b0:b0 + step]
                img, needed = ops.raster_views(scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc,
                                               scene._features_rest, scene.active_sh_degree, torch.from_numpy(rows[part]).to(dev), size[0], size[1],
                                               channels=4 if rgba else 3, scale_modifier=scale_modifier, background=background,
                                               max_instances=min(per_view_instances * len(part), ops.RASTER_MAX_INSTANCES), want_instances=True)
                # the next batch starts from what this one needed (plus a quarter), so that only the first one can run twice
                per_view_instances = max(per_view_instances, -(-needed // len(part)) * 5 // 4)
                for j, i in enumerate(part):
                    images[i] = img[j]
            continue
        per_view = max(ops.splat_views_workspace_bytes(n, 1, *size), 1)
        step = int(batch_size) if batch_size is not None else max(1, WORKSPACE_BUDGET // per_view)
        workspace = torch.empty(ops.splat_views_workspace_bytes(n, min(step, len(which)), *size), dtype=torch.uint8, device=dev)
        for b0 in range(0, len(which), step):
            part = which[b0:b0 + step]
            img = ops.splat_views(scene._xyz, scene._scaling, scene._features_dc, scene._features_rest, scene.active_sh_degree,
                                  torch.from_numpy(rows[part]).to(dev), size[0], size[1], channels=4 if rgba else 3, extent=extent,
                                  near_z=near_z, background=background, workspace=workspace)
            for j, i in enumerate(part):
                images[i] = img[j]
    host = [im.cpu().numpy() for im in images]
    out = [_as_camera_info(c, h) for c, h in zip(cameras, host)]
    return (out, images) if return_device else out


DEPTH_KINDS = ("median", "expected")


def _depth_groups(scene, cameras, kind, points, want_image, chunk, scale_modifier, background=(1.0, 1.0, 1.0)):
    """The raw depth call per group of cameras of one size -> [(indices of the group's cameras, ops.scene_depth_raw's dict)]."""
    if kind not in DEPTH_KINDS:
        raise ValueError(f"kind must be 'median' or 'expected' (got {kind!r})")
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    if not (float(scale_modifier) > 0.0 and float(scale_modifier) < float("inf")):
        raise ValueError(f"scale_modifier must be positive and finite (got {scale_modifier})")
    cameras = list(cameras)
    rows = camera_rows(cameras)
    if not scene.get_xyz.is_cuda:
        raise RuntimeError("6dgs_amd: depth maps need the scene on the GPU (no CPU fallback on the product path)")
    sizes = [(int(_field(c, "width")), int(_field(c, "height"))) for c in cameras]
    dev = scene.get_xyz.device
    want = ("median", "median_index", "alpha") if kind == "median" else ("expected", "alpha")
    groups = []
    for size in sorted(set(sizes)):
        which = [i for i, s in enumerate(sizes) if s == size]
        raw = ops.scene_depth_raw(scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc, scene._features_rest,
                                  scene.active_sh_degree, torch.from_numpy(rows[which]).to(dev), size[0], size[1], want=want,
                                  points=kind if points else None, want_image=want_image, chunk=int(chunk), scale_modifier=scale_modifier,
                                  background=background)
        groups.append((which, raw))
    return cameras, groups


def _depth_of(raw, kind):
    """(depth, valid) [V,H,W] of one raw call: the median, or expected / alpha where alpha > 0 and 0 elsewhere."""
    if kind == "median":
        return raw["median"], raw["median_index"] >= 0
    valid = raw["alpha"] > 0
    return torch.where(valid, raw["expected"] / raw["alpha"], torch.zeros_like(raw["expected"])), valid


@torch.no_grad()
def render_depth(scene: GaussianScene, cameras: Sequence, *, kind: str = "median", points: bool = False, chunk: int = 8,
                 scale_modifier: float = 1.0, return_device: bool = False) -> dict:
    """Depth maps of the views the 3DGS rasteriser renders (ops.scene_depth_raw; sixdgs_raster_depth in include/sixdgs.h defines
    them).  kind="median": the camera depth of the Gaussian that takes the pixel's transmittance below one half; "expected": the
    alpha-weighted mean depth of what the pixel saw, expected / alpha.  Returns a dict of lists, one entry per camera in the order
    given: depth float32 [H,W] (0 where there is none), alpha float32 [H,W], valid bool [H,W]; with kind="median" index int32 [H,W]
    (that Gaussian, -1 where there is none); with points=True points float32 [H,W,3], the world point of the pixel's ray at `depth`
    (zeros where not valid).  When every camera has the same size the entries are stacked to [V,H,W(,3)] arrays instead.  Cameras of
    one size are rendered together, `chunk` views per launch; the maps do not depend on it.  numpy arrays, or with return_device
    GPU tensors."""
    cameras, groups = _depth_groups(scene, cameras, kind, bool(points), False, chunk, scale_modifier)
    keys = ("depth", "alpha", "valid") + (("index",) if kind == "median" else ()) + (("points",) if points else ())
    out = {k: [None] * len(cameras) for k in keys}
    for which, raw in groups:
        depth, valid = _depth_of(raw, kind)
        maps = {"depth": depth, "alpha": raw["alpha"], "valid": valid, "index": raw.get("median_index"), "points": raw.get("points")}
        for j, i in enumerate(which):
            for k in keys:
                out[k][i] = maps[k][j]
    if len(groups) <= 1:
        out = {k: (torch.stack(v) if v else torch.empty(0)) for k, v in out.items()}
        return out if return_device else {k: v.cpu().numpy() for k, v in out.items()}
    return out if return_device else {k: [t.cpu().numpy() for t in v] for k, v in out.items()}


@torch.no_grad()
def surface_points(scene: GaussianScene, cameras: Sequence, *, min_alpha: float = 0.5, stride: int = 1, kind: str = "median",
                   chunk: int = 8, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0)):
    """A surface point cloud from views: the world points (render_depth's `points`) of every `stride`-th pixel, in x and in y, that is
    valid and has alpha >= min_alpha, coloured from the rasteriser's uint8 image of the same pass.  Returns GPU tensors (xyz float32
    [M,3], rgb uint8 [M,3], view int32 [M] -- the camera's position in `cameras` --, pixel int32 [M,2] = (x, y)), ordered by size
    group, then view, then row-major pixel; GaussianScene.from_points(xyz, rgb / 255) re-seeds a scene from them."""
    if not 0.0 <= float(min_alpha) <= 1.0:
        raise ValueError(f"min_alpha must be in [0, 1] (got {min_alpha})")
    if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
        raise ValueError(f"stride must be a positive integer (got {stride!r})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    cameras, groups = _depth_groups(scene, cameras, kind, True, True, chunk, scale_modifier, background)
    dev = scene.get_xyz.device
    parts = []
    for which, raw in groups:
        _, valid = _depth_of(raw, kind)
        keep = valid & (raw["alpha"] >= float(min_alpha))
        grid = torch.zeros_like(keep)
        grid[:, ::int(stride), ::int(stride)] = True
        keep &= grid
        v, y, x = torch.nonzero(keep, as_tuple=True)
        parts.append((raw["points"][keep], raw["image"][keep][:, :3], torch.tensor(which, dtype=torch.int32, device=dev)[v],
                      torch.stack([x, y], dim=1).to(torch.int32)))
    if not parts:
        return (torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, 2, dtype=torch.int32, device=dev))
    return tuple(torch.cat([p[k] for p in parts]) for k in range(4))
