"""Tensor-level front end of the C ABI (include/sixdgs.h): PyTorch owns memory and streams, the HIP
library does the work.  Every function requires CUDA(ROCm) tensors -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import threading
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import Profile, ScorerWeights, check

D = 384
MMA_DEFAULT, MMA_F32, MMA_BF16X6, MMA_F16X3, MMA_F16X3_L32 = -1, 0, 1, 2, 3
F16_MODES = (MMA_F16X3, MMA_F16X3_L32)     # scaled fp16 key planes; they differ in how the logits are stored between the passes
MMA_LIBRARY_DEFAULT = MMA_F16X3
_mma_mode = MMA_DEFAULT


def set_mma_mode(mode: int):
    """Select how the fp32 contractions run on the matrix cores (see SIXDGS_MMA_* in include/sixdgs.h)."""
    global _mma_mode
    assert mode in (MMA_DEFAULT, MMA_F32, MMA_BF16X6, MMA_F16X3, MMA_F16X3_L32)
    _mma_mode = mode


def get_mma_mode() -> int:
    return _mma_mode


def effective_mma_mode() -> int:
    """The mode MMA_DEFAULT resolves to inside the library."""
    return MMA_LIBRARY_DEFAULT if _mma_mode == MMA_DEFAULT else _mma_mode

RAY_IN_PAD = 144
TOK_IN = 398
MAX_TOKENS = 256


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


_tls = threading.local()     # .device: index of the device of the call being marshalled on this thread (set by _on_device / _need_gpu)


def _stream():
    """The current PyTorch stream OF THE TENSORS' DEVICE (not of whatever device is current in the process)."""
    dev = getattr(_tls, "device", None)
    return C.c_void_p(torch.cuda.current_stream(dev if dev is not None else torch.cuda.current_device()).cuda_stream)


def _first_device(objs):
    for a in objs:
        if torch.is_tensor(a):
            if a.is_cuda:
                return a.device
        elif isinstance(a, (PackedWeights, SelectStream)):
            if getattr(a, "device", None) is not None:      # None while the object is being constructed
                return a.device
        elif isinstance(a, (list, tuple)) and a and torch.is_tensor(a[0]) and a[0].is_cuda:
            return a[0].device
        elif isinstance(a, (str, torch.device)) and not isinstance(a, bool):
            try:
                d = torch.device(a)
            except (RuntimeError, TypeError, ValueError):
                continue
            if d.type == "cuda":
                return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
    return None


def _on_device(fn):
    """Every library call runs with the device of its tensor arguments current -- the kernels launch on the device that is current
    when the library is entered -- and puts the process's current device back afterwards (a call on cuda:1 tensors does not move
    the caller to cuda:1).  The device is kept per THREAD for _stream(), so concurrent callers on different devices do not see each
    other's choice."""
    @functools.wraps(fn)
    def scoped(*args, **kwargs):
        dev = _first_device(list(args) + list(kwargs.values()))
        prev = getattr(_tls, "device", None)
        try:
            if dev is None or not torch.cuda.is_available():
                return fn(*args, **kwargs)
            _tls.device = dev.index
            if dev.index == torch.cuda.current_device():
                return fn(*args, **kwargs)
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)
        finally:
            _tls.device = prev
    return scoped


def _need_gpu(*ts):
    """Every tensor argument must be a GPU tensor, all on ONE device -- the device _on_device made current for the call."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("6dgs_amd: tensors must live on the GPU (no CPU fallback on the product path)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"6dgs_amd: tensor arguments on different devices ({dev} and {t.device})")
    if dev is not None:
        _tls.device = dev.index


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _i64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.int64).contiguous()


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
@_on_device
def mask_degraded(log_scale: torch.Tensor, target_points: int = 50) -> torch.Tensor:
    log_scale = _f32(log_scale)
    _need_gpu(log_scale)
    n = log_scale.shape[0]
    out = torch.empty(n, dtype=torch.uint8, device=log_scale.device)
    check(_lib.load().sixdgs_mask_degraded(_p(log_scale), n, int(target_points), _p(out), _stream()), "mask_degraded")
    return out.bool()


@_on_device
def sym_eig_3x3(mats: torch.Tensor, eigenvectors: bool = True):
    mats = _f32(mats)
    _need_gpu(mats)
    shape = mats.shape[:-2]
    m = mats.reshape(-1, 3, 3)
    vals = torch.empty(m.shape[0], 3, device=m.device)
    vecs = torch.empty(m.shape[0], 3, 3, device=m.device) if eigenvectors else None
    check(_lib.load().sixdgs_sym_eig_3x3(_p(m), m.shape[0], _p(vals), _p(vecs), _stream()), "sym_eig_3x3")
    return vals.reshape(*shape, 3), (vecs.reshape(*shape, 3, 3) if eigenvectors else None)


KNN_GRID_FROM = 16384     # clouds at least this large take the grid search (identical results, O(E) instead of O(E^2))


@_on_device
def normals_knn(query: torch.Tensor, cloud: torch.Tensor, k: int = 20, return_knn: bool = False, method: str = "auto"):
    """a4.  method: "brute" (the reference's exhaustive search), "grid" (uniform-grid search, same neighbour lists and
    normals bit for bit) or "auto" (grid from KNN_GRID_FROM points)."""
    same = query is cloud
    query, cloud = _f32(query), _f32(cloud)
    if same:
        query = cloud                      # keeps the pointer identity the grid kernel uses to walk the queries in cell order
    _need_gpu(query, cloud)
    lib = _lib.load()
    nq, e = query.shape[0], cloud.shape[0]
    out = torch.empty(nq, 3, device=query.device)
    knn = torch.empty(nq, k, dtype=torch.int64, device=query.device) if return_knn else None
    if method not in ("auto", "brute", "grid"):
        raise ValueError(method)
    if method == "grid" or (method == "auto" and e >= KNN_GRID_FROM):
        ws = torch.empty(lib.sixdgs_normals_knn_grid_workspace_bytes(e), dtype=torch.uint8, device=query.device)
        check(lib.sixdgs_normals_knn_grid(_p(query), nq, _p(cloud), e, int(k), _p(out), _p(knn), _p(ws), ws.numel(), _stream()),
              "normals_knn_grid")
    else:
        check(lib.sixdgs_normals_knn(_p(query), nq, _p(cloud), e, int(k), _p(out), _p(knn), _stream()), "normals_knn")
    return (out, knn) if return_knn else out


@_on_device
def quadricell_centers(scale: torch.Tensor, target_points: int = 50, table_res: int = 1000):
    """a6 alone: (points[C,3], ellipsoid_id[C]) for activated semi axes scale[E,3]."""
    scale = _f32(scale)
    _need_gpu(scale)
    lib = _lib.load()
    e = scale.shape[0]
    dev = scale.device
    counts = torch.empty(max(e, 1), dtype=torch.int64, device=dev)
    offs = torch.empty(max(e, 1), dtype=torch.int64, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    check(lib.sixdgs_quadricell_cell_counts(_p(scale), e, int(target_points), _p(counts), _p(offs), _p(total), _stream()),
          "quadricell_cell_counts")
    c = int(total[0].item())
    pts = torch.empty(c, 3, device=dev)
    eid = torch.empty(c, dtype=torch.int64, device=dev)
    if c:
        check(lib.sixdgs_quadricell_centers(_p(scale), e, int(target_points), int(table_res), _p(offs), _p(pts), _p(eid),
                                            _stream()), "quadricell_centers")
    return pts, eid


@_on_device
def emit_quadricell(xyz, scale, rot, f_dc, f_rest, sh_degree: int, sel: Optional[torch.Tensor], normals, target_points: int = 50,
                    table_res: int = 1000, scale_is_log: bool = True, want_rgb: bool = True):
    """a1+a6+a7+a10: returns ori[R,3], dir[R,3], rgb[R,3] (or None), src[R] (Gaussian id), n_cells."""
    xyz, scale, rot, normals = _f32(xyz), _f32(scale), _f32(rot), _f32(normals)
    _need_gpu(xyz, scale, rot, normals)
    lib = _lib.load()
    dev = xyz.device
    sel_t = _i64(sel) if sel is not None else None
    e = sel_t.shape[0] if sel_t is not None else xyz.shape[0]
    assert normals.shape[0] == e
    counts = torch.empty(max(e, 1), dtype=torch.int64, device=dev)
    offs = torch.empty(max(e, 1), dtype=torch.int64, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    check(lib.sixdgs_emit_quadricell_count(_p(xyz), _p(scale), int(scale_is_log), _p(rot), _p(sel_t), e, _p(normals),
                                           int(target_points), int(table_res), _p(counts), _p(offs), _p(total), _stream()),
          "emit_quadricell_count")
    tot = total.tolist()  # the one host sync of the emitter (the reference syncs at sampling.py:145)
    r, n_cells = int(tot[0]), int(tot[1])
    ori = torch.empty(r, 3, device=dev)
    dr = torch.empty(r, 3, device=dev)
    src = torch.empty(r, dtype=torch.int64, device=dev)
    rgb = None
    n_coef = 1
    if want_rgb:
        f_dc, f_rest = _f32(f_dc), _f32(f_rest)
        n_coef = 1 + f_rest.shape[1]
        rgb = torch.empty(r, 3, device=dev)
    else:
        sh_degree = 0                       # no colour asked for: the degree names no coefficients (the entry point checks it against n_coef)
    if r:
        check(lib.sixdgs_emit_quadricell_write(_p(xyz), _p(scale), int(scale_is_log), _p(rot), _p(f_dc if want_rgb else None),
                                               _p(f_rest if want_rgb else None), int(sh_degree), int(n_coef), _p(sel_t), e,
                                               _p(normals), int(target_points), int(table_res), _p(offs), _p(ori), _p(dr),
                                               _p(rgb), _p(src), _stream()), "emit_quadricell_write")
    return ori, dr, rgb, src, n_cells


@_on_device
def isocell_distribution(ray_target: int, n0: int = 1, device="cuda") -> torch.Tensor:
    lib = _lib.load()
    cnt = C.c_int64(0)
    check(lib.sixdgs_isocell_distribution(int(ray_target), int(n0), None, C.byref(cnt), _stream()), "isocell_distribution")
    out = torch.empty(cnt.value, 3, device=device)
    _need_gpu(out)
    check(lib.sixdgs_isocell_distribution(int(ray_target), int(n0), _p(out), C.byref(cnt), _stream()), "isocell_distribution")
    return out


@_on_device
def rotate_isocell(dirs: torch.Tensor, normals: torch.Tensor) -> torch.Tensor:
    dirs, normals = _f32(dirs), _f32(normals)
    _need_gpu(dirs, normals)
    out = torch.empty(normals.shape[0], dirs.shape[0], 3, device=dirs.device)
    check(_lib.load().sixdgs_rotate_isocell(_p(dirs), dirs.shape[0], _p(normals), normals.shape[0], _p(out), _stream()),
          "rotate_isocell")
    return out


@_on_device
def emit_isocell(xyz, scale, rot, f_dc, f_rest, sh_degree: int, sel, normals, dirs, scale_is_log: bool = True,
                 want_rgb: bool = True, want_src: bool = True):
    xyz, scale, rot, normals, dirs = _f32(xyz), _f32(scale), _f32(rot), _f32(normals), _f32(dirs)
    _need_gpu(xyz, scale, rot, normals, dirs)
    dev = xyz.device
    sel_t = _i64(sel) if sel is not None else None
    e = sel_t.shape[0] if sel_t is not None else xyz.shape[0]
    k = dirs.shape[0]
    ori = torch.empty(e * k, 3, device=dev)
    dr = torch.empty(e * k, 3, device=dev)
    rgb = torch.empty(e * k, 3, device=dev) if want_rgb else None
    src = torch.empty(e * k, dtype=torch.int64, device=dev) if want_src else None
    n_coef = 1
    if want_rgb:
        f_dc, f_rest = _f32(f_dc), _f32(f_rest)
        n_coef = 1 + f_rest.shape[1]
    else:
        sh_degree = 0                       # as in emit_quadricell
    check(_lib.load().sixdgs_emit_isocell(_p(xyz), _p(scale), int(scale_is_log), _p(rot), _p(f_dc if want_rgb else None),
                                          _p(f_rest if want_rgb else None), int(sh_degree), int(n_coef), _p(sel_t), e,
                                          _p(normals), _p(dirs), k, _p(ori), _p(dr), _p(rgb), _p(src), _stream()), "emit_isocell")
    return ori, dr, rgb, src


@_on_device
def eval_sh_color(sh: torch.Tensor, dirs: torch.Tensor, sh_degree: int) -> torch.Tensor:
    sh, dirs = _f32(sh), _f32(dirs)
    _need_gpu(sh, dirs)
    out = torch.empty(dirs.shape[0], 3, device=dirs.device)
    check(_lib.load().sixdgs_eval_sh_color(_p(sh), sh.shape[-1], _p(dirs), dirs.shape[0], int(sh_degree), _p(out), _stream()),
          "eval_sh_color")
    return out


# ---------------------------------------------------------------------------------------------
# rendering a scene and comparing it with a target: what the functions below share.  Every check here runs before _need_gpu.
# ---------------------------------------------------------------------------------------------
RASTER_INSTANCES_PER_GAUSSIAN = 8       # first guess of the tile instances a (view, Gaussian) pair needs; an overflow is retried exactly
RASTER_MAX_INSTANCES = (1 << 31) - 1
SCENE_ARRAYS = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")      # the order the rasteriser's entry points take a scene in


def raster_instances_estimate(n: int, views: int) -> int:
    return int(min(max(RASTER_INSTANCES_PER_GAUSSIAN * int(n) * int(views), 4096), RASTER_MAX_INSTANCES))


def _scene_shape(xyz, scale, rot, opacity, f_dc, f_rest):
    """(n, n_coef) of a scene's arrays, which must agree about n; rot and opacity may be None (the splatter takes neither)."""
    n = xyz.shape[0]
    n_coef = 1 + (f_rest.shape[1] if f_rest.dim() == 3 else 0)
    if (xyz.shape != (n, 3) or scale.shape != (n, 3) or (rot is not None and rot.shape != (n, 4))
            or (opacity is not None and opacity.numel() != n) or f_dc.numel() != 3 * n or f_rest.numel() != 3 * n * (n_coef - 1)):
        raise ValueError("scene arrays disagree about the number of Gaussians")
    return n, n_coef


def _scene(xyz, scale, rot, opacity, f_dc, f_rest):
    """A scene's arrays as contiguous float32 -> (the six tensors, n, n_coef)."""
    t = tuple(None if a is None else _f32(a) for a in (xyz, scale, rot, opacity, f_dc, f_rest))
    return (t, *_scene_shape(*t))


def _scene_args(t, n_coef, scale_is_log, opacity_is_logit):
    """The eight arguments the rasteriser's entry points begin with."""
    xyz, scale, rot, opacity, f_dc, f_rest = t
    return (_p(xyz), _p(scale), int(scale_is_log), _p(rot), _p(opacity), int(opacity_is_logit), _p(f_dc), _p(f_rest if n_coef > 1 else None))


def _view_args(cams, width, height, background, scale_modifier=1.0, name="cams"):
    """The arguments that say how the views are drawn -> (cams as contiguous float32, width, height)."""
    if not (float(scale_modifier) > 0.0 and float(scale_modifier) < float("inf")):
        raise ValueError(f"scale_modifier must be positive and finite (got {scale_modifier})")
    if int(width) < 1 or int(height) < 1:
        raise ValueError(f"width and height must be positive (got {width} x {height})")
    if not torch.is_tensor(cams) or cams.dim() != 2 or cams.shape[1] != 16:
        raise ValueError(f"{name} must be a [views,16] tensor (got {tuple(cams.shape) if torch.is_tensor(cams) else type(cams).__name__})")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    return _f32(cams), int(width), int(height)


def _background(background, dev):
    return torch.tensor([float(b) for b in background], dtype=torch.float32).to(dev)


def _target_args(target, views, height, width):
    """A target image, fp32 [views,height,width,3|4] or uint8 [views,height,width,3] and contiguous -> (target, is_u8, stride)."""
    if not torch.is_tensor(target) or target.dim() != 4 or tuple(target.shape[:3]) != (views, height, width):
        raise ValueError(f"target must be a [{views},{height},{width},3|4] tensor (got {tuple(target.shape) if torch.is_tensor(target) else type(target).__name__})")
    if target.dtype == torch.uint8:
        if target.shape[3] != 3:
            raise ValueError("a uint8 target must have 3 channels")
    elif target.dtype != torch.float32 or target.shape[3] not in (3, 4):
        raise ValueError(f"target must be float32 with 3 or 4 channels, or uint8 with 3 (got {target.dtype} with {target.shape[3]})")
    if not target.is_contiguous():
        raise ValueError("target must be contiguous")
    return target.detach(), int(target.dtype == torch.uint8), int(target.shape[3])


def _lambda(lambda_dssim) -> float:
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1] (got {lambda_dssim})")
    return float(lambda_dssim)


def _capacity(max_instances, n, views) -> int:
    """The instance capacity a call starts with: the caller's, or the estimate."""
    if max_instances is None:
        return raster_instances_estimate(n, views)
    if not 1 <= int(max_instances) <= RASTER_MAX_INSTANCES:
        raise ValueError(f"max_instances must be in [1, 2^31) (got {max_instances})")
    return int(max_instances)


def _grown(needed: int) -> int:
    """The capacity of the next run of a fused loop that overflowed: 5/4 of what it needed."""
    return min(max(needed + needed // 4, 1), RASTER_MAX_INSTANCES)


def _workspace(workspace, need, dev):
    """The caller's workspace if it holds `need` bytes, else a new one -> (the tensor, its bytes)."""
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    return workspace, workspace.numel() * workspace.element_size()


def splat_views_workspace_bytes(n: int, views: int, width: int, height: int) -> int:
    return int(_lib.load().sixdgs_splat_views_workspace_bytes(int(n), int(views), int(width), int(height)))


@_on_device
def splat_views(xyz, scale, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int, channels: int = 3,
                extent: float = 1.0, near_z: float = 0.05, background=(1.0, 1.0, 1.0), want_winner: bool = False,
                scale_is_log: bool = True, workspace: Optional[torch.Tensor] = None):
    """Synthetic query views: the Gaussians as z-buffered flat discs in their SH colour towards the camera (sixdgs_splat_views in
    include/sixdgs.h defines the image pixel by pixel).  cams [V,16] = w2c rows 0..2 (12 floats), fx, fy, cx, cy per view.
    Returns the uint8 image [V,height,width,channels], and with want_winner (image, winner int32 [V,height,width], -1 = background)."""
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4 (got {channels})")
    if not (float(extent) > 0.0 and float(extent) < float("inf")):
        raise ValueError(f"extent must be positive and finite (got {extent})")
    if not float(near_z) >= 0.0:
        raise ValueError(f"near_z must be >= 0 (got {near_z})")
    cams, width, height = _view_args(cams, width, height, background)
    (xyz, scale, _, _, f_dc, f_rest), n, n_coef = _scene(xyz, scale, None, None, f_dc, f_rest)
    views = cams.shape[0]
    _need_gpu(xyz, scale, f_dc, f_rest, cams, workspace)
    lib = _lib.load()
    dev = xyz.device
    ws, ws_bytes = _workspace(workspace, lib.sixdgs_splat_views_workspace_bytes(n, views, width, height), dev)
    bg = _background(background, dev)
    image = torch.empty(views, height, width, channels, dtype=torch.uint8, device=dev)
    winner = torch.empty(views, height, width, dtype=torch.int32, device=dev) if want_winner else None
    check(lib.sixdgs_splat_views(_p(xyz), _p(scale), int(scale_is_log), _p(f_dc), _p(f_rest if n_coef > 1 else None), int(sh_degree),
                                 int(n_coef), n, _p(cams), views, width, height, int(channels), float(extent), float(near_z),
                                 _p(bg), _p(image), _p(winner), _p(ws), ws_bytes, _stream()),
          "splat_views")
    return (image, winner) if want_winner else image


def raster_views_workspace_bytes(n: int, views: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_raster_views_workspace_bytes(int(n), int(views), int(width), int(height), int(max_instances)))


@_on_device
def raster_views(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int, channels: int = 3,
                 scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0), want_float: bool = False, want_u8: bool = True,
                 want_radii: bool = False, want_instances: bool = False, scale_is_log: bool = True, opacity_is_logit: bool = True,
                 max_instances: Optional[int] = None, workspace: Optional[torch.Tensor] = None, profile: Optional[Profile] = None,
                 want_state: bool = False):
    """Views of the scene by the alpha-blended 3DGS forward rasteriser (sixdgs_raster_views in include/sixdgs.h defines the image
    operation by operation).  cams [V,16] = w2c rows 0..2 (12 floats), fx, fy, cx, cy per view; opacity [N] or [N,1].
    Returns, in this order and as far as asked for: the float image [V,height,width,4] (rgb, 1 - T: want_float), the uint8 image
    [V,height,width,channels] (want_u8), radii int32 [V,N] (want_radii), the number of tile instances the scene needed (want_instances);
    one value alone is returned bare.  The call runs with a capacity estimate (or max_instances), reads the needed count -- one
    synchronisation -- and on overflow runs once more with the exact size.  want_state appends the forward's state for
    raster_views_backward: (the workspace tensor the call ran in, the capacity it ran with)."""
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4 (got {channels})")
    cams, width, height = _view_args(cams, width, height, background, scale_modifier)
    if not (want_float or want_u8 or want_radii or want_instances or want_state):
        raise ValueError("nothing asked for: want_float, want_u8, want_radii and want_instances are all off")
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views = cams.shape[0]
    capacity = _capacity(max_instances, n, views)
    _need_gpu(*scene, cams, workspace)
    lib = _lib.load()
    dev = scene[0].device
    bg = _background(background, dev)
    image_f = torch.empty(views, height, width, 4, dtype=torch.float32, device=dev) if want_float else None
    image_u = torch.empty(views, height, width, channels, dtype=torch.uint8, device=dev) if want_u8 else None
    radii = torch.empty(views, n, dtype=torch.int32, device=dev) if want_radii else None
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    needed = 0
    for attempt in range(2):
        need = lib.sixdgs_raster_views_workspace_bytes(n, views, width, height, capacity)
        if need == 0 and views > 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(workspace, need, dev)
        check(lib.sixdgs_raster_views(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n, _p(cams),
                                      views, width, height, float(scale_modifier), _p(bg), _p(image_f), _p(image_u), int(channels), _p(radii),
                                      capacity, _p(count), _p(ws), ws_bytes, _stream(), profile),
              "raster_views")
        needed = int(count.item()) if views > 0 else 0
        if needed <= capacity:
            break
        if attempt == 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: raster_views needs {needed} tile instances per launch (limit 2^31 - 1): render fewer views at once")
        capacity = needed
    out = [o for o, want in ((image_f, want_float), (image_u, want_u8), (radii, want_radii), (needed, want_instances),
                             ((ws, capacity), want_state)) if want]
    return out[0] if len(out) == 1 else tuple(out)


def raster_views_backward_workspace_bytes(n: int, views: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_raster_views_backward_workspace_bytes(int(n), int(views), int(width), int(height), int(max_instances)))


RASTER_GRADIENTS = SCENE_ARRAYS + ("cams",)


@_on_device
def raster_views_backward(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int,
                          grad_image: torch.Tensor, state, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0),
                          scale_is_log: bool = True, opacity_is_logit: bool = True, want=RASTER_GRADIENTS,
                          workspace: Optional[torch.Tensor] = None, profile: Optional[Profile] = None):
    """The gradients of raster_views' float image (sixdgs_raster_views_backward in include/sixdgs.h defines them): grad_image
    [V,height,width,4] = dL / d image_f32; state = (workspace, capacity) of a raster_views(..., want_state=True) call on the same
    arguments, not written since.  Returns a tuple in the order of RASTER_GRADIENTS -- d xyz [N,3], d scale [N,3], d rot [N,4],
    d opacity (the shape of opacity), d f_dc, d f_rest (their shapes), d cams [V,16] -- with None for the names not in `want`."""
    cams, width, height = _view_args(cams, width, height, background, scale_modifier)
    want = tuple(want)
    if not want or any(w not in RASTER_GRADIENTS for w in want):
        raise ValueError(f"want must name some of {RASTER_GRADIENTS} (got {want})")
    if (not isinstance(state, (tuple, list)) or len(state) != 2 or not torch.is_tensor(state[0])
            or not 1 <= int(state[1]) <= RASTER_MAX_INSTANCES):
        raise ValueError("state must be the (workspace, capacity) pair of raster_views(..., want_state=True)")
    fwd_ws, capacity = state[0], int(state[1])
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views = cams.shape[0]
    if not torch.is_tensor(grad_image) or tuple(grad_image.shape) != (views, height, width, 4):
        raise ValueError(f"grad_image must be a [{views},{height},{width},4] tensor")
    grad_image = _f32(grad_image)
    _need_gpu(*scene, cams, grad_image, fwd_ws, workspace)
    lib = _lib.load()
    dev = scene[0].device
    need = lib.sixdgs_raster_views_backward_workspace_bytes(n, views, width, height, capacity)
    if need == 0 and views > 0:
        raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, {width} x {height}, instances {capacity})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    bg = _background(background, dev)
    like = dict(zip(RASTER_GRADIENTS, (*scene, cams)))
    # (views == 0 launches nothing: zeros are the sum over no views)
    out = {k: (torch.zeros_like(like[k]) if views == 0 else torch.empty_like(like[k])) for k in want}
    check(lib.sixdgs_raster_views_backward(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n,
                                           _p(cams), views, width, height, float(scale_modifier), _p(bg), _p(grad_image), capacity,
                                           _p(fwd_ws), fwd_ws.numel() * fwd_ws.element_size(), *[_p(out.get(k)) for k in RASTER_GRADIENTS],
                                           _p(ws), ws_bytes, _stream(), profile),
          "raster_views_backward")
    return tuple(out.get(k) for k in RASTER_GRADIENTS)


# the accumulators of sixdgs_raster_contrib, in the order its entry points take them
CONTRIB = (("weight", torch.float32), ("peak", torch.float32), ("pixels", torch.int64), ("stops", torch.int64), ("seen", torch.int32))
CONTRIB_VIEWS = (("view_weight", torch.float32), ("view_pixels", torch.int32))
CONTRIB_STATUS_CAPACITY = 2


def contrib_state(n: int, device) -> dict:
    """The accumulators of raster_contrib, zeroed: weight, peak float32 [n], pixels, stops int64 [n], seen int32 [n]."""
    return {k: torch.zeros(int(n), dtype=dt, device=device) for k, dt in CONTRIB}


def _check_contrib(out, n):
    if not isinstance(out, dict) or any(k not in dict(CONTRIB) for k in out):
        raise ValueError(f"out must be a dict with some of the keys {tuple(k for k, _ in CONTRIB)} (ops.contrib_state makes it)")
    for k, dt in CONTRIB:
        t = out.get(k)
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous()):
            raise ValueError(f"out[{k!r}] must be a contiguous {dt} [{n}] tensor (ops.contrib_state makes the dict)")


def raster_contrib_workspace_bytes(n: int, views: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_raster_contrib_workspace_bytes(int(n), int(views), int(width), int(height), int(max_instances)))


@_on_device
def raster_contrib(state, n: int, views: int, width: int, height: int, out: Optional[dict] = None, *, want_views: bool = False,
                   workspace: Optional[torch.Tensor] = None, profile: Optional[Profile] = None) -> dict:
    """Every Gaussian's contribution to the views of one forward (sixdgs_raster_contrib in include/sixdgs.h defines it): state = the
    (workspace, capacity) pair of raster_views(..., want_state=True) on n Gaussians and `views` rows at width x height, not written
    since.  out: the accumulators, UPDATED IN PLACE -- ops.contrib_state's dict or a part of it (a missing key is not computed); None
    starts from zeros.  Returns out, with want_views plus view_weight float32 [V,N] and view_pixels int32 [V,N] (written)."""
    if (not isinstance(state, (tuple, list)) or len(state) != 2 or not torch.is_tensor(state[0])
            or not 1 <= int(state[1]) <= RASTER_MAX_INSTANCES):
        raise ValueError("state must be the (workspace, capacity) pair of raster_views(..., want_state=True)")
    fwd_ws, capacity = state[0], int(state[1])
    n, views, width, height = int(n), int(views), int(width), int(height)
    if n < 0 or views < 0 or width < 1 or height < 1:
        raise ValueError(f"n and views must not be negative, width and height positive (got {n}, {views}, {width} x {height})")
    dev = fwd_ws.device
    if out is None:
        out = contrib_state(n, dev)
    _check_contrib(out, n)
    _need_gpu(fwd_ws, workspace, *out.values())
    lib = _lib.load()
    need = lib.sixdgs_raster_contrib_workspace_bytes(n, views, width, height, capacity)
    if need == 0:
        raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, {width} x {height}, instances {capacity})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    res = dict(out)
    if want_views:
        res.update({k: torch.zeros(views, n, dtype=dt, device=dev) for k, dt in CONTRIB_VIEWS})
    check(lib.sixdgs_raster_contrib(n, views, width, height, capacity, _p(fwd_ws), fwd_ws.numel() * fwd_ws.element_size(),
                                    *[_p(res.get(k)) for k, _ in CONTRIB + CONTRIB_VIEWS], _p(ws), ws_bytes, _stream(), profile),
          "raster_contrib")
    return res


def scene_contrib_workspace_bytes(n: int, chunk: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_scene_contrib_workspace_bytes(int(n), int(chunk), int(width), int(height), int(max_instances)))


@_on_device
def scene_contrib_raw(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int, *,
                      chunk: int = 8, want_views: bool = False, scale_modifier: float = 1.0, scale_is_log: bool = True,
                      opacity_is_logit: bool = True, max_instances: Optional[int] = None, retry: bool = True,
                      workspace: Optional[torch.Tensor] = None) -> dict:
    """Every Gaussian's contribution to the views cams [V,16] as ONE library call (sixdgs_scene_contrib in include/sixdgs.h): chunks of
    `chunk` views, each projected, sorted and walked on the device, nothing read back in between.  max_instances is the capacity of
    one chunk.  Returns a dict: the accumulators of CONTRIB from zero (weight, peak float32 [N]; pixels, stops int64 [N]; seen int32
    [N]), with want_views view_weight float32 [V,N] and view_pixels int32 [V,N], status (int32 [1]; bit 1: a chunk did not fit the
    capacity and is missing from the sums), instances_needed and max_instances (ints).  The call reads status and instances_needed
    once at the end and -- with retry -- on bit 1 starts again from zeros with the needed capacity."""
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    cams, width, height = _view_args(cams, width, height, (0.0, 0.0, 0.0), scale_modifier)
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views = cams.shape[0]
    chunk = max(min(int(chunk), views), 1)
    capacity = _capacity(max_instances, n, chunk)
    _need_gpu(*scene, cams, workspace)
    lib = _lib.load()
    dev = scene[0].device
    out = contrib_state(n, dev)
    if want_views:
        out.update({k: torch.zeros(views, n, dtype=dt, device=dev) for k, dt in CONTRIB_VIEWS})
    out["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    needed_t = torch.zeros(1, dtype=torch.int64, device=dev)
    needed = 0
    for attempt in range(2):
        need = lib.sixdgs_scene_contrib_workspace_bytes(n, chunk, width, height, capacity)
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, chunk {chunk}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(workspace, need, dev)
        check(lib.sixdgs_scene_contrib(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n, _p(cams),
                                       views, width, height, float(scale_modifier), chunk, capacity,
                                       *[_p(out.get(k)) for k, _ in CONTRIB + CONTRIB_VIEWS], _p(out["status"]), _p(needed_t), _p(ws), ws_bytes,
                                       _stream()),
              "scene_contrib")
        if views == 0:
            break
        # the one host read of the call: the status word and the largest instance count seen
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = int(flags[1])
        if not retry or not int(flags[0]) & CONTRIB_STATUS_CAPACITY:
            break
        if attempt == 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: scene_contrib needs {needed} tile instances per chunk (limit 2^31 - 1): use a smaller chunk")
        capacity = needed
        for k, _ in CONTRIB:           # the chunks that fitted are in the sums already
            out[k].zero_()
    out["instances_needed"] = needed
    out["max_instances"] = capacity
    return out


# the maps of sixdgs_raster_depth, in the order its entry points take them (points, [V,H,W,3], comes behind them)
DEPTH_MAPS = (("expected", torch.float32), ("median", torch.float32), ("median_index", torch.int32), ("alpha", torch.float32))
DEPTH_POINTS = {"median": 0, "expected": 1}
DEPTH_STATUS_CAPACITY = 2


def _depth_want(want, points):
    want = tuple(want)
    if any(w not in dict(DEPTH_MAPS) for w in want):
        raise ValueError(f"want must name some of {tuple(k for k, _ in DEPTH_MAPS)} (got {want})")
    if points is not None and points not in DEPTH_POINTS:
        raise ValueError(f"points must be None, 'median' or 'expected' (got {points!r})")
    if not want and points is None:
        raise ValueError("nothing asked for: want is empty and points is None")
    return want


def raster_depth_workspace_bytes(n: int, views: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_raster_depth_workspace_bytes(int(n), int(views), int(width), int(height), int(max_instances)))


@_on_device
def raster_depth(state, n: int, views: int, width: int, height: int, *, cams: Optional[torch.Tensor] = None,
                 want=("expected", "median", "median_index", "alpha"), points: Optional[str] = None,
                 workspace: Optional[torch.Tensor] = None, profile: Optional[Profile] = None) -> dict:
    """The depth maps of the views of one forward (sixdgs_raster_depth in include/sixdgs.h defines them): state = the (workspace,
    capacity) pair of raster_views(..., want_state=True) on n Gaussians and `views` rows at width x height, not written since.  Returns
    a dict with the maps named in `want`, [V,height,width] each -- expected (the blend's depth channel, un-normalised), median, alpha
    float32, median_index int32 (-1: T stayed at or above 0.5) -- and with points="median" | "expected" the world points
    [V,height,width,3] at that depth (zeros where the pixel has none); these need cams [V,16], the forward's rows."""
    if (not isinstance(state, (tuple, list)) or len(state) != 2 or not torch.is_tensor(state[0])
            or not 1 <= int(state[1]) <= RASTER_MAX_INSTANCES):
        raise ValueError("state must be the (workspace, capacity) pair of raster_views(..., want_state=True)")
    fwd_ws, capacity = state[0], int(state[1])
    n, views, width, height = int(n), int(views), int(width), int(height)
    if n < 0 or views < 0 or width < 1 or height < 1:
        raise ValueError(f"n and views must not be negative, width and height positive (got {n}, {views}, {width} x {height})")
    want = _depth_want(want, points)
    if points is not None:
        if not torch.is_tensor(cams) or tuple(cams.shape) != (views, 16):
            raise ValueError(f"points need cams, the forward's [{views},16] rows (got {tuple(cams.shape) if torch.is_tensor(cams) else type(cams).__name__})")
        cams = _f32(cams)
    else:
        cams = None
    dev = fwd_ws.device
    _need_gpu(fwd_ws, cams, workspace)
    lib = _lib.load()
    need = lib.sixdgs_raster_depth_workspace_bytes(n, views, width, height, capacity)
    if need == 0:
        raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, {width} x {height}, instances {capacity})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    res = {k: torch.empty(views, height, width, dtype=dt, device=dev) for k, dt in DEPTH_MAPS if k in want}
    if points is not None:
        res["points"] = torch.empty(views, height, width, 3, dtype=torch.float32, device=dev)
    check(lib.sixdgs_raster_depth(n, views, width, height, capacity, _p(fwd_ws), fwd_ws.numel() * fwd_ws.element_size(), _p(cams),
                                  *[_p(res.get(k)) for k, _ in DEPTH_MAPS], _p(res.get("points")), DEPTH_POINTS.get(points, 0), _p(ws), ws_bytes,
                                  _stream(), profile),
          "raster_depth")
    return res


def scene_depth_workspace_bytes(n: int, chunk: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_scene_depth_workspace_bytes(int(n), int(chunk), int(width), int(height), int(max_instances)))


@_on_device
def scene_depth_raw(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int, *,
                    want=("expected", "median", "median_index", "alpha"), points: Optional[str] = None, want_image: bool = False,
                    channels: int = 3, chunk: int = 8, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0), scale_is_log: bool = True,
                    opacity_is_logit: bool = True, max_instances: Optional[int] = None, retry: bool = True,
                    workspace: Optional[torch.Tensor] = None) -> dict:
    """The depth maps of the views cams [V,16] as ONE library call (sixdgs_scene_depth in include/sixdgs.h): chunks of `chunk` views,
    each rasterised and walked on the device, nothing read back in between.  max_instances is the capacity of one chunk.  Returns a
    dict: the maps named in `want` and `points` as raster_depth returns them, image (uint8 [V,height,width,channels], the rasteriser's
    own image of the same pass, with want_image), status (int32 [1]; bit 1: a chunk did not fit the capacity and its rows are as they
    were allocated: zeros, median_index -1), instances_needed and max_instances (ints).  The call reads status and instances_needed
    once at the end and -- with retry -- on bit 1 runs once more with the needed capacity."""
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4 (got {channels})")
    want = _depth_want(want, points)
    cams, width, height = _view_args(cams, width, height, background, scale_modifier)
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views = cams.shape[0]
    chunk = max(min(int(chunk), views), 1)
    capacity = _capacity(max_instances, n, chunk)
    _need_gpu(*scene, cams, workspace)
    lib = _lib.load()
    dev = scene[0].device
    bg = _background(background, dev)
    out = {k: torch.zeros(views, height, width, dtype=dt, device=dev) for k, dt in DEPTH_MAPS if k in want}
    if "median_index" in out:
        out["median_index"].fill_(-1)
    if points is not None:
        out["points"] = torch.zeros(views, height, width, 3, dtype=torch.float32, device=dev)
    if want_image:
        out["image"] = torch.zeros(views, height, width, int(channels), dtype=torch.uint8, device=dev)
    out["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    needed_t = torch.zeros(1, dtype=torch.int64, device=dev)
    needed = 0
    for attempt in range(2):
        need = lib.sixdgs_scene_depth_workspace_bytes(n, chunk, width, height, capacity)
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, chunk {chunk}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(workspace, need, dev)
        check(lib.sixdgs_scene_depth(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n, _p(cams),
                                     views, width, height, float(scale_modifier), _p(bg), chunk, capacity,
                                     *[_p(out.get(k)) for k, _ in DEPTH_MAPS], _p(out.get("points")), DEPTH_POINTS.get(points, 0),
                                     _p(out.get("image")), int(channels), _p(out["status"]), _p(needed_t), _p(ws), ws_bytes, _stream()),
              "scene_depth")
        if views == 0:
            break
        # the one host read of the call: the status word and the largest instance count seen
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = int(flags[1])
        if not retry or not int(flags[0]) & DEPTH_STATUS_CAPACITY:
            break
        if attempt == 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: scene_depth needs {needed} tile instances per chunk (limit 2^31 - 1): use a smaller chunk")
        capacity = needed
    out["instances_needed"] = needed
    out["max_instances"] = capacity
    return out


def photometric_loss_workspace_bytes(views: int, width: int, height: int, want_grad: bool = False) -> int:
    return int(_lib.load().sixdgs_photometric_loss_workspace_bytes(int(views), int(width), int(height), int(bool(want_grad))))


@_on_device
def photometric_loss(image: torch.Tensor, target: torch.Tensor, *, lambda_dssim: float = 0.2, grad_loss: Optional[torch.Tensor] = None,
                     want_grad: bool = False, want_parts: bool = False, workspace: Optional[torch.Tensor] = None,
                     profile: Optional[Profile] = None):
    """(1 - lambda) L1 + lambda (1 - SSIM) per view (sixdgs_photometric_loss in include/sixdgs.h defines it operation by operation).
    image fp32 [V,H,W,3|4] (4: raster_views' float image; its fourth channel is not read); target fp32 [V,H,W,3|4] or uint8 [V,H,W,3]
    (value u / 255); both contiguous and on one GPU.  Returns loss [V], then -- as far as asked for -- grad_image, the image's shape,
    = grad_loss[v] d loss_v / d image (grad_loss [V], None: ones; want_grad), and parts [V,2] = (l1, ssim) (want_parts)."""
    lam = _lambda(lambda_dssim)
    if not torch.is_tensor(image) or image.dim() != 4 or image.shape[3] not in (3, 4):
        raise ValueError(f"image must be a [views,height,width,3|4] tensor (got {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__})")
    if image.dtype != torch.float32:
        raise ValueError(f"image must be float32 (got {image.dtype})")
    if not image.is_contiguous():
        raise ValueError("image must be contiguous")
    views, height, width, stride = image.shape
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be positive (got {width} x {height})")
    target, target_is_u8, target_stride = _target_args(target, views, height, width)
    if grad_loss is not None:
        if not want_grad:
            raise ValueError("grad_loss without want_grad")
        if not torch.is_tensor(grad_loss) or tuple(grad_loss.shape) != (views,):
            raise ValueError(f"grad_loss must be a [{views}] tensor")
        grad_loss = _f32(grad_loss)
    image = image.detach()
    _need_gpu(image, target, grad_loss, workspace)
    lib = _lib.load()
    dev = image.device
    need = lib.sixdgs_photometric_loss_workspace_bytes(views, width, height, int(want_grad))
    if need == 0 and views > 0:
        raise ValueError(f"sizes outside the photometric loss's limits (views {views}, {width} x {height})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    loss = torch.empty(views, dtype=torch.float32, device=dev)
    parts = torch.empty(views, 2, dtype=torch.float32, device=dev) if want_parts else None
    grad = torch.empty_like(image) if want_grad else None
    check(lib.sixdgs_photometric_loss(_p(image), stride, _p(target), target_is_u8, target_stride, views, width, height, lam, _p(grad_loss),
                                      _p(loss), _p(parts), _p(grad), _p(ws), ws_bytes, _stream(), profile),
          "photometric_loss")
    out = [loss] + [o for o, want in ((grad, want_grad), (parts, want_parts)) if want]
    return out[0] if len(out) == 1 else tuple(out)


METRICS = ("l1", "ssim", "mse", "mse_r", "mse_g", "mse_b")      # the columns of sixdgs_image_metrics' rows
EVALUATE_STATUS_CAPACITY = 2


def image_metrics_workspace_bytes(views: int, width: int, height: int) -> int:
    return int(_lib.load().sixdgs_image_metrics_workspace_bytes(int(views), int(width), int(height)))


def _quantise(quantise) -> int:
    if not isinstance(quantise, (bool, int)) or int(quantise) not in (0, 1):
        raise ValueError(f"quantise must be a flag (got {quantise!r})")
    return int(quantise)


@_on_device
def image_metrics(image: torch.Tensor, target: torch.Tensor, *, quantise, want_render: bool = False, workspace: Optional[torch.Tensor] = None,
                  profile: Optional[Profile] = None):
    """L1, SSIM and the squared error per view (sixdgs_image_metrics in include/sixdgs.h defines them operation by operation).  image,
    target: photometric_loss's.  quantise False clamps the float inputs to [0, 1]; True passes them through the 8-bit round trip of a
    saved PNG.  Returns metrics fp32 [V,6] in the order of METRICS, and with want_render (metrics, render_u8 uint8 [V,H,W,3]): the
    image's bytes by the 8-bit rule."""
    q = _quantise(quantise)
    if not torch.is_tensor(image) or image.dim() != 4 or image.shape[3] not in (3, 4):
        raise ValueError(f"image must be a [views,height,width,3|4] tensor (got {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__})")
    if image.dtype != torch.float32:
        raise ValueError(f"image must be float32 (got {image.dtype})")
    if not image.is_contiguous():
        raise ValueError("image must be contiguous")
    views, height, width, stride = image.shape
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be positive (got {width} x {height})")
    target, target_is_u8, target_stride = _target_args(target, views, height, width)
    image = image.detach()
    _need_gpu(image, target, workspace)
    lib = _lib.load()
    dev = image.device
    need = lib.sixdgs_image_metrics_workspace_bytes(views, width, height)
    if need == 0 and views > 0:
        raise ValueError(f"sizes outside the metrics' limits (views {views}, {width} x {height})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    metrics = torch.empty(views, len(METRICS), dtype=torch.float32, device=dev)
    render = torch.empty(views, height, width, 3, dtype=torch.uint8, device=dev) if want_render else None
    check(lib.sixdgs_image_metrics(_p(image), stride, _p(target), target_is_u8, target_stride, views, width, height, q, _p(metrics), _p(render),
                                   _p(ws), ws_bytes, _stream(), profile),
          "image_metrics")
    return (metrics, render) if want_render else metrics


def evaluate_views_workspace_bytes(n: int, chunk: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_evaluate_views_workspace_bytes(int(n), int(chunk), int(width), int(height), int(max_instances)))


@_on_device
def evaluate_views_raw(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int,
                       target: torch.Tensor, *, quantise, chunk: int = 8, want_render: bool = False, scale_modifier: float = 1.0,
                       background=(1.0, 1.0, 1.0), scale_is_log: bool = True, opacity_is_logit: bool = True,
                       max_instances: Optional[int] = None, retry: bool = True, workspace: Optional[torch.Tensor] = None) -> dict:
    """Render the views cams [V,16] and measure them against target as ONE library call (sixdgs_evaluate_views in include/sixdgs.h):
    chunks of `chunk` views, each rasterised and measured on the device, nothing read back in between.  max_instances is the capacity
    of one chunk.  Returns a dict: metrics fp32 [V,6] (METRICS' order), status (int32 [1]; bit 1: a chunk did not fit the capacity and
    its rows are NaN), render (uint8 [V,height,width,3], with want_render), instances_needed and max_instances (ints).  The call
    reads status and instances_needed once at the end and -- with retry -- on bit 1 runs once more with the needed capacity."""
    q = _quantise(quantise)
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk must be a positive integer (got {chunk!r})")
    cams, width, height = _view_args(cams, width, height, background, scale_modifier)
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views = cams.shape[0]
    chunk = max(min(int(chunk), views), 1)
    capacity = _capacity(max_instances, n, chunk)
    target, target_is_u8, target_stride = _target_args(target, views, height, width)
    _need_gpu(*scene, cams, target, workspace)
    lib = _lib.load()
    dev = scene[0].device
    bg = _background(background, dev)
    out = {"metrics": torch.empty(views, len(METRICS), dtype=torch.float32, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}
    if want_render:
        out["render"] = torch.empty(views, height, width, 3, dtype=torch.uint8, device=dev)
    needed_t = torch.zeros(1, dtype=torch.int64, device=dev)
    needed = 0
    for attempt in range(2):
        need = lib.sixdgs_evaluate_views_workspace_bytes(n, chunk, width, height, capacity)
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, chunk {chunk}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(workspace, need, dev)
        check(lib.sixdgs_evaluate_views(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n, _p(cams),
                                        views, width, height, float(scale_modifier), _p(bg), _p(target), target_is_u8, target_stride, q, chunk,
                                        capacity, _p(out["metrics"]), _p(out.get("render")), _p(out["status"]), _p(needed_t), _p(ws), ws_bytes,
                                        _stream()),
              "evaluate_views")
        if views == 0:
            break
        # the one host read of the call: the status word and the largest instance count seen
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = int(flags[1])
        if not retry or not int(flags[0]) & EVALUATE_STATUS_CAPACITY:
            break
        if attempt == 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: evaluate_views needs {needed} tile instances per chunk (limit 2^31 - 1): use a smaller chunk")
        capacity = needed
    out["instances_needed"] = needed
    out["max_instances"] = capacity
    return out


# ---------------------------------------------------------------------------------------------
# pose refinement below the C ABI
# ---------------------------------------------------------------------------------------------
POSE_STATE = (("delta", 6, torch.float32), ("m", 6, torch.float32), ("v", 6, torch.float32), ("rows", 16, torch.float32),
              ("best_loss", 0, torch.float32), ("best_step", 0, torch.int32), ("best_rows", 16, torch.float32), ("status", 0, torch.int32))
POSE_STATUS_NOT_FINITE, POSE_STATUS_CAPACITY = 1, 2
REFINE_ATTEMPTS = 4                 # runs of refine_poses_raw before it gives up on the instance capacity


def _check_adam(lr, beta1, beta2, eps):
    if not (0.0 < float(lr) < float("inf")):
        raise ValueError(f"lr must be positive and finite (got {lr})")
    if not (0.0 <= float(beta1) < 1.0 and 0.0 <= float(beta2) < 1.0):
        raise ValueError(f"beta1 and beta2 must be in [0, 1) (got {beta1}, {beta2})")
    if not (0.0 <= float(eps) < float("inf")):
        raise ValueError(f"eps must be non-negative and finite (got {eps})")


def _check_rows(t, name, width=16):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != width or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 [views,{width}] tensor")


@_on_device
def pose_compose(start: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """rows [V,16] = the camera rows start [V,16] with the rigid motions delta [V,6] = (translation, axis-angle) applied after their
    w2c (sixdgs_pose_compose in include/sixdgs.h defines it operation by operation)."""
    _check_rows(start, "start")
    _check_rows(delta, "delta", 6)
    if delta.shape[0] != start.shape[0]:
        raise ValueError("start and delta disagree about the number of views")
    _need_gpu(start, delta)
    rows = torch.empty_like(start)
    check(_lib.load().sixdgs_pose_compose(_p(start), _p(delta), start.shape[0], _p(rows), _stream()), "pose_compose")
    return rows


@_on_device
def pose_state(start: torch.Tensor) -> dict:
    """The state sixdgs_pose_step starts from, for start [V,16]: delta = m = v = 0, rows = pose_compose(start, 0), best_loss = +inf,
    best_step = 0, best_rows = start, status = 0, instances_needed = 0 (int64 [1])."""
    _check_rows(start, "start")
    _need_gpu(start)
    views, dev = start.shape[0], start.device
    z = torch.zeros(views, 6, device=dev)
    return {"delta": z, "m": z.clone(), "v": z.clone(), "rows": pose_compose(start, z), "best_loss": torch.full((views,), float("inf"), device=dev),
            "best_step": torch.zeros(views, dtype=torch.int32, device=dev), "best_rows": start.clone(),
            "status": torch.zeros(views, dtype=torch.int32, device=dev), "instances_needed": torch.zeros(1, dtype=torch.int64, device=dev)}


@_on_device
def pose_step(start: torch.Tensor, loss: torch.Tensor, d_rows: Optional[torch.Tensor], state: dict, history_row: torch.Tensor, step: int, *,
              instances: Optional[torch.Tensor] = None, max_instances: int = RASTER_MAX_INSTANCES, evaluate_only: bool = False,
              lr: float = 2e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """Step `step` of a refinement (sixdgs_pose_step in include/sixdgs.h): records loss [V] of the iterate in state["rows"] into
    history_row [V], keeps the first minimum, and -- unless evaluate_only -- chains d_rows [V,16] to the 6-vector, takes one Adam step
    and writes the next iterate's rows.  `state` is pose_state's dict, UPDATED IN PLACE; instances: the int64 [1] count a rasteriser
    call left on the device, checked against max_instances."""
    _check_rows(start, "start")
    views = start.shape[0]
    if isinstance(step, bool) or int(step) != step or int(step) < 0:
        raise ValueError(f"step must be a non-negative integer (got {step})")
    _check_adam(lr, beta1, beta2, eps)
    if not 1 <= int(max_instances) <= RASTER_MAX_INSTANCES:
        raise ValueError(f"max_instances must be in [1, 2^31) (got {max_instances})")
    for name, t in (("loss", loss), ("history_row", history_row)):
        if not torch.is_tensor(t) or tuple(t.shape) != (views,) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 [{views}] tensor")
    if evaluate_only:
        d_rows = None
    else:
        _check_rows(d_rows, "d_rows")
        if d_rows.shape[0] != views:
            raise ValueError("start and d_rows disagree about the number of views")
    for name, width, dtype in POSE_STATE:
        t = state.get(name) if isinstance(state, dict) else None
        if (not torch.is_tensor(t) or tuple(t.shape) != ((views, width) if width else (views,)) or t.dtype != dtype or not t.is_contiguous()):
            raise ValueError(f"state[{name!r}] must be a contiguous {dtype} tensor of {views} views (ops.pose_state makes the dict)")
    needed = state.get("instances_needed")
    if not torch.is_tensor(needed) or tuple(needed.shape) != (1,) or needed.dtype != torch.int64:
        raise ValueError("state['instances_needed'] must be an int64 [1] tensor")
    if instances is not None and (not torch.is_tensor(instances) or tuple(instances.shape) != (1,) or instances.dtype != torch.int64):
        raise ValueError("instances must be an int64 [1] tensor")
    _need_gpu(start, loss, d_rows, history_row, instances, needed, *[state[name] for name, _, _ in POSE_STATE])
    check(_lib.load().sixdgs_pose_step(_p(start), _p(loss), _p(d_rows), _p(instances), int(max_instances), views, int(step), int(bool(evaluate_only)),
                                       float(lr), float(beta1), float(beta2), float(eps), _p(state["delta"]), _p(state["m"]), _p(state["v"]),
                                       _p(state["rows"]), _p(state["best_loss"]), _p(state["best_step"]), _p(state["best_rows"]), _p(history_row),
                                       _p(state["status"]), _p(needed), _stream()), "pose_step")


def refine_poses_workspace_bytes(n: int, views: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_refine_poses_workspace_bytes(int(n), int(views), int(width), int(height), int(max_instances)))


@_on_device
def refine_poses_raw(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, start_rows: torch.Tensor, width: int, height: int,
                     target: torch.Tensor, *, steps: int, lambda_dssim: float = 0.2, lr: float = 2e-3, beta1: float = 0.9, beta2: float = 0.999,
                     eps: float = 1e-8, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0), scale_is_log: bool = True,
                     opacity_is_logit: bool = True, max_instances: Optional[int] = None, retry: bool = True) -> dict:
    """Render-and-compare refinement of the camera rows start_rows [V,16] as ONE library call (sixdgs_refine_poses in include/sixdgs.h):
    steps + 1 evaluations and `steps` Adam updates, enqueued without a host read.  target: fp32 [V,height,width,3|4] or uint8
    [V,height,width,3].  Returns a dict: best_rows [V,16], best_loss [V], best_step [V] (int32), history [steps + 1,V], delta [V,6] (the
    last iterate's motion), status [V] (int32; bit 0: a loss or gradient was not finite, bit 1: the instance capacity was too small),
    instances_needed (int) and max_instances (int: the capacity of the run returned).  The call runs with raster_instances_estimate's capacity (or max_instances), reads status and
    instances_needed once at the end, and -- with retry -- on bit 1 runs again from the start with 5/4 of the needed capacity, at most
    REFINE_ATTEMPTS runs in all, then RuntimeError."""
    lam = _lambda(lambda_dssim)
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"steps must be a positive integer (got {steps})")
    _check_adam(lr, beta1, beta2, eps)
    start_rows, width, height = _view_args(start_rows, width, height, background, scale_modifier, "start_rows")
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    views, steps = start_rows.shape[0], int(steps)
    capacity = _capacity(max_instances, n, views)
    target, target_is_u8, target_stride = _target_args(target, views, height, width)
    _need_gpu(*scene, start_rows, target)
    lib = _lib.load()
    dev = scene[0].device
    bg = _background(background, dev)
    out = {"best_rows": torch.empty(views, 16, device=dev), "best_loss": torch.empty(views, device=dev),
           "best_step": torch.empty(views, dtype=torch.int32, device=dev), "history": torch.empty(steps + 1, views, device=dev),
           "delta": torch.empty(views, 6, device=dev), "status": torch.empty(views, dtype=torch.int32, device=dev)}
    needed_t = torch.zeros(1, dtype=torch.int64, device=dev)
    needed = 0
    for attempt in range(REFINE_ATTEMPTS):
        need = lib.sixdgs_refine_poses_workspace_bytes(n, views, width, height, capacity)
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(None, need, dev)
        check(lib.sixdgs_refine_poses(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n,
                                      _p(start_rows), views, width, height, float(scale_modifier), _p(bg), _p(target), target_is_u8,
                                      target_stride, lam, steps, float(lr), float(beta1), float(beta2), float(eps), capacity,
                                      _p(out["best_rows"]), _p(out["best_loss"]), _p(out["best_step"]), _p(out["history"]), _p(out["delta"]),
                                      _p(out["status"]), _p(needed_t), _p(ws), ws_bytes, _stream()),
              "refine_poses")
        if views == 0:
            break
        # the one host read of the call: every status word and the largest instance count seen
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = int(flags[-1])
        if not retry or not bool((flags[:-1] & POSE_STATUS_CAPACITY).any()):
            break
        if attempt == REFINE_ATTEMPTS - 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: refine_poses still needs {needed} tile instances after {attempt + 1} runs (limit 2^31 - 1): "
                               "refine fewer views at once")
        capacity = _grown(needed)
    out["instances_needed"] = needed
    out["max_instances"] = capacity
    return out


# a coarse-to-fine level schedule (csrc/pyramid_rules.h states the limits)
PYRAMID_MAX_LEVELS, PYRAMID_MAX_DOWNSCALE, PYRAMID_MAX_SIDE = 8, 256, 32768


def pyramid_geometry(width: int, height: int, downscale: int):
    """(w, h, crop_x, crop_y) of the level of `downscale` of a width x height query: w = width // d, h = height // d and the centred crop
    to a multiple of d (LEVEL GEOMETRY in include/sixdgs.h).  Needs no GPU."""
    d = int(downscale)
    w, h = int(width) // d, int(height) // d
    return w, h, (int(width) - w * d) // 2, (int(height) - h * d) // 2


def _host(ctype, values):
    """A host array of `ctype` for an entry point that reads it at the call -> (the array, which the caller keeps alive; its pointer)."""
    a = (ctype * len(values))(*values)
    return a, C.cast(a, C.c_void_p)


@_on_device
def target_pyramid(images_u8: torch.Tensor, downscales, *, composite: bool = False, background=(1.0, 1.0, 1.0), out=None) -> list:
    """The targets of a level schedule (sixdgs_target_pyramid in include/sixdgs.h): images_u8 uint8 [V,H,W,3|4] on the GPU and up to 8
    downscales d -> a list of fp32 [V,H // d,W // d,3], each pixel the mean of a d x d block of the centred crop, composited over
    `background` first when `composite` (which needs four channels).  One streaming kernel per level; the same bytes on every call.
    out: the tensors to write (contiguous fp32 of those shapes), else new ones."""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] not in (3, 4):
        raise ValueError("images_u8 must be a uint8 [V,H,W,3|4] tensor")
    if not images_u8.is_contiguous():
        raise ValueError("images_u8 must be contiguous")
    views, height, width, channels = (int(x) for x in images_u8.shape)
    downscales = list(downscales)
    if any(isinstance(d, bool) or int(d) != d for d in downscales):
        raise ValueError(f"downscales must be integers (got {downscales})")
    ds = [int(d) for d in downscales]
    if not 1 <= len(ds) <= PYRAMID_MAX_LEVELS:
        raise ValueError(f"1 to {PYRAMID_MAX_LEVELS} levels (got {len(ds)})")
    if composite and channels != 4:
        raise ValueError("compositing needs a four-channel image")
    if len(background) != 3:
        raise ValueError("background must have 3 entries")
    if not 1 <= width <= PYRAMID_MAX_SIDE or not 1 <= height <= PYRAMID_MAX_SIDE:
        raise ValueError(f"width and height must be in [1, {PYRAMID_MAX_SIDE}] (got {width} x {height})")
    shapes = []
    for d in ds:
        if not 1 <= d <= PYRAMID_MAX_DOWNSCALE:
            raise ValueError(f"a downscale must be in [1, {PYRAMID_MAX_DOWNSCALE}] (got {d})")
        w, h, _, _ = pyramid_geometry(width, height, d)
        if w < 1 or h < 1:
            raise ValueError(f"downscale {d} leaves nothing of a {width} x {height} image")
        shapes.append((views, h, w, 3))
    _need_gpu(images_u8)
    if out is None:
        out = [torch.empty(s, dtype=torch.float32, device=images_u8.device) for s in shapes]
    out = list(out)
    if len(out) != len(ds) or any(not torch.is_tensor(o) or tuple(o.shape) != s or o.dtype != torch.float32 or not o.is_contiguous()
                                  for o, s in zip(out, shapes)):
        raise ValueError(f"out must be contiguous float32 tensors of shapes {shapes}")
    _need_gpu(images_u8, *out)
    keep = [_host(C.c_float, [float(b) for b in background]), _host(C.c_int32, ds), _host(C.c_void_p, [o.data_ptr() for o in out])]
    check(_lib.load().sixdgs_target_pyramid(_p(images_u8), views, height, width, channels, int(bool(composite)), keep[0][1], len(ds),
                                            keep[1][1], keep[2][1], _stream()), "target_pyramid")
    return out


@_on_device
def pose_rebase(rows: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """rows_out [V,16] = (the 12 w2c entries of rows [V,16], intrinsics [V,4]): a copy of bits (sixdgs_pose_rebase).  It starts a level
    of a schedule from another level's camera."""
    _check_rows(rows, "rows")
    _check_rows(intrinsics, "intrinsics", 4)
    if intrinsics.shape[0] != rows.shape[0]:
        raise ValueError("rows and intrinsics disagree about the number of views")
    _need_gpu(rows, intrinsics)
    out = torch.empty_like(rows)
    check(_lib.load().sixdgs_pose_rebase(_p(rows), _p(intrinsics), rows.shape[0], _p(out), _stream()), "pose_rebase")
    return out


def refine_poses_levels_workspace_bytes(n: int, views: int, sizes, max_instances) -> int:
    """sixdgs_refine_poses_levels_workspace_bytes for levels of sizes [(width, height), ...] and their capacities; needs no GPU."""
    w, h, cap = _host(C.c_int32, [int(s[0]) for s in sizes]), _host(C.c_int32, [int(s[1]) for s in sizes]), _host(C.c_int64, [int(c) for c in max_instances])
    return int(_lib.load().sixdgs_refine_poses_levels_workspace_bytes(int(n), int(views), len(sizes), w[1], h[1], cap[1]))


@_on_device
def refine_poses_levels_raw(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, start_rows: torch.Tensor, levels, *,
                            lambda_dssim: float = 0.2, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, scale_modifier: float = 1.0,
                            background=(1.0, 1.0, 1.0), scale_is_log: bool = True, opacity_is_logit: bool = True, retry: bool = True) -> dict:
    """A coarse-to-fine schedule of render-and-compare refinement as ONE library call (sixdgs_refine_poses_levels in include/sixdgs.h).
    start_rows [V,16] carry the LAST level's intrinsics.  levels: up to 8 dicts, coarse to fine, each with width, height, steps, lr,
    target (fp32 [V,height,width,3], contiguous), intrinsics ([V,4]) and optionally max_instances (else raster_instances_estimate's).
    Returns a dict: out_rows [V,16] (the last level's best camera, or start_rows' bits where kept_input), loss_input [V] (the input's
    loss at the last level), kept_input [V] (int32), best_loss and best_step [L,V], history (a list of [steps_l + 1,V] views of one
    buffer), status [V] (int32, bits as refine_poses_raw's, carried across the levels), instances_needed and max_instances (lists of int
    per level).  Reads status and the counts once at the end and -- with retry -- on bit 1 runs again with 5/4 of what each overflowed
    level needed, at most REFINE_ATTEMPTS runs in all, then RuntimeError."""
    lam = _lambda(lambda_dssim)
    levels = [dict(lv) for lv in levels]
    if not 1 <= len(levels) <= PYRAMID_MAX_LEVELS:
        raise ValueError(f"1 to {PYRAMID_MAX_LEVELS} levels (got {len(levels)})")
    scene, n, n_coef = _scene(xyz, scale, rot, opacity, f_dc, f_rest)
    rows, views, capacities = None, 0, []
    for i, lv in enumerate(levels):
        steps = lv.get("steps")
        if steps is None or isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError(f"level {i}: steps must be a positive integer (got {steps})")
        _check_adam(lv.get("lr", float("nan")), beta1, beta2, eps)
        rows, lv["width"], lv["height"] = _view_args(start_rows, lv.get("width", 0), lv.get("height", 0), background, scale_modifier, "start_rows")
        views = rows.shape[0]
        lv["steps"], lv["lr"] = int(steps), float(lv["lr"])
        lv["target"], is_u8, stride = _target_args(lv.get("target"), views, lv["height"], lv["width"])
        if is_u8 or stride != 3:
            raise ValueError(f"level {i}: the target must be float32 with 3 channels")
        _check_rows(lv.get("intrinsics"), f"level {i}: intrinsics", 4)
        if lv["intrinsics"].shape[0] != views:
            raise ValueError(f"level {i}: intrinsics disagree about the number of views")
        capacities.append(_capacity(lv.get("max_instances"), n, views))
    start_rows = rows
    _need_gpu(*scene, start_rows, *[lv["target"] for lv in levels], *[lv["intrinsics"] for lv in levels])
    lib = _lib.load()
    dev = scene[0].device
    bg = _background(background, dev)
    k = len(levels)
    first = [0]
    for lv in levels:
        first.append(first[-1] + lv["steps"] + 1)
    out = {"out_rows": torch.empty(views, 16, device=dev), "loss_input": torch.empty(views, device=dev),
           "kept_input": torch.empty(views, dtype=torch.int32, device=dev), "best_loss": torch.empty(k, views, device=dev),
           "best_step": torch.empty(k, views, dtype=torch.int32, device=dev), "status": torch.empty(views, dtype=torch.int32, device=dev)}
    history = torch.empty(first[-1], views, device=dev)
    needed_t = torch.zeros(k, dtype=torch.int64, device=dev)
    needed = [0] * k
    h = {name: _host(ctype, [lv[name] for lv in levels]) for name, ctype in (("width", C.c_int32), ("height", C.c_int32), ("steps", C.c_int32),
                                                                                ("lr", C.c_float))}
    h_target = _host(C.c_void_p, [lv["target"].data_ptr() for lv in levels])
    h_intr = _host(C.c_void_p, [lv["intrinsics"].data_ptr() for lv in levels])
    for attempt in range(REFINE_ATTEMPTS):
        h_cap = _host(C.c_int64, capacities)
        need = lib.sixdgs_refine_poses_levels_workspace_bytes(n, views, k, h["width"][1], h["height"][1], h_cap[1])
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, views {views}, levels {[(lv['width'], lv['height']) for lv in levels]}, "
                             f"instances {capacities})")
        ws, ws_bytes = _workspace(None, need, dev)
        check(lib.sixdgs_refine_poses_levels(*_scene_args(scene, n_coef, scale_is_log, opacity_is_logit), int(sh_degree), int(n_coef), n,
                                             _p(start_rows), views, float(scale_modifier), _p(bg), lam, k, h["width"][1], h["height"][1],
                                             h["steps"][1], h["lr"][1], h_target[1], h_intr[1], h_cap[1], float(beta1), float(beta2), float(eps),
                                             _p(out["out_rows"]), _p(out["loss_input"]), _p(out["kept_input"]), _p(out["best_loss"]),
                                             _p(out["best_step"]), _p(needed_t), _p(history), _p(out["status"]), _p(ws), ws_bytes, _stream()),
              "refine_poses_levels")
        if views == 0:
            break
        # the one host read of the call: every status word and every level's largest instance count
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = [int(x) for x in flags[views:]]
        if not retry or not bool((flags[:views] & POSE_STATUS_CAPACITY).any()):
            break
        if attempt == REFINE_ATTEMPTS - 1 or max(needed) > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: refine_poses_levels still needs {needed} tile instances after {attempt + 1} runs (limit 2^31 - 1): "
                               "refine fewer views at once")
        capacities = [_grown(nd) if nd > cap else cap for nd, cap in zip(needed, capacities)]
    out["history"] = [history[first[i]:first[i + 1]] for i in range(k)]
    out["instances_needed"] = needed
    out["max_instances"] = list(capacities)
    return out


# ---------------------------------------------------------------------------------------------
# fitting a scene's Gaussians below the C ABI
# ---------------------------------------------------------------------------------------------
FIT_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")      # the order of sixdgs_gaussian_adam, of m / v and of group_mask
FIT_STATUS_NOT_FINITE, FIT_STATUS_CAPACITY = 1, 2


def _check_fit_hyper(beta1, beta2, eps):
    if not (0.0 <= float(beta1) < 1.0 and 0.0 <= float(beta2) < 1.0):
        raise ValueError(f"beta1 and beta2 must be in [0, 1) (got {beta1}, {beta2})")
    if not (0.0 <= float(eps) < float("inf")):
        raise ValueError(f"eps must be non-negative and finite (got {eps})")


def _check_rates(lrs):
    lrs = [float(x) for x in lrs]
    if len(lrs) != len(FIT_GROUPS) or not all(0.0 <= x < float("inf") for x in lrs):
        raise ValueError(f"lrs must be {len(FIT_GROUPS)} non-negative finite rates in the order {FIT_GROUPS} (got {lrs})")
    return lrs


def _fit_params(params, what="params"):
    """The six arrays of `params` (a dict by FIT_GROUPS' names) -> (n, n_coef); contiguous float32, agreeing about n."""
    if not isinstance(params, dict) or any(k not in params for k in FIT_GROUPS):
        raise ValueError(f"{what} must be a dict with the keys {FIT_GROUPS}")
    for k in FIT_GROUPS:
        t = params[k]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}[{k!r}] must be a contiguous float32 tensor")
    n, n_coef = _scene_shape(*[params[k] for k in SCENE_ARRAYS])
    if n_coef > 16:
        raise ValueError(f"f_rest holds {n_coef - 1} coefficients per channel (at most 15)")
    return n, n_coef


def gaussian_adam_state(params: dict) -> dict:
    """The state sixdgs_gaussian_adam starts from, for the six arrays of `params`: m = v = 0 (one buffer each, n (11 + 3 n_coef) floats,
    group after group in FIT_GROUPS' order) and status = 0 (int32 [1])."""
    n, n_coef = _fit_params(params)
    dev = params["xyz"].device
    size = n * (11 + 3 * n_coef)
    return {"m": torch.zeros(size, device=dev), "v": torch.zeros(size, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}


def gaussian_adam_slices(n: int, n_coef: int) -> dict:
    """name -> slice of m / v, in floats."""
    out, off = {}, 0
    for k, w in zip(FIT_GROUPS, (3, 3, 3 * (n_coef - 1), 1, 3, 4)):
        out[k] = slice(off, off + n * w)
        off += n * w
    return out


def gaussian_adam(params: dict, grads: dict, state: dict, step: int, lrs, *, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-15,
                  instances: Optional[torch.Tensor] = None, max_instances: int = RASTER_MAX_INSTANCES) -> None:
    """One Adam step (t = step + 1) over the six parameter arrays of `params`, IN PLACE, as one kernel launch (sixdgs_gaussian_adam in
    include/sixdgs.h).  params, grads: dicts by FIT_GROUPS' names; grads[k] None (or absent) freezes group k -- its parameters and its
    slices of m and v stay bit for bit.  lrs: six rates in FIT_GROUPS' order (0 is legal and still updates m and v).  state:
    gaussian_adam_state's dict, updated in place; status bit 0: a gradient entry was not finite and was left out; bit 1: the count in
    `instances` (int64 [1], what a rasteriser call left on the device) exceeded max_instances -- that call and every later one changes
    nothing."""
    _fit_params(params)
    return _gaussian_adam(params["xyz"], params, grads, state, step, lrs, beta1, beta2, eps, instances, max_instances)


@_on_device
def _gaussian_adam(anchor, params, grads, state, step, lrs, beta1, beta2, eps, instances, max_instances):
    """gaussian_adam with the device of `anchor` current (the dicts do not tell _on_device where the call runs)."""
    n, n_coef = _fit_params(params)
    if isinstance(step, bool) or int(step) != step or int(step) < 0:
        raise ValueError(f"step must be a non-negative integer (got {step})")
    lrs = _check_rates(lrs)
    _check_fit_hyper(beta1, beta2, eps)
    if not 1 <= int(max_instances) <= RASTER_MAX_INSTANCES:
        raise ValueError(f"max_instances must be in [1, 2^31) (got {max_instances})")
    if not isinstance(grads, dict) or any(k not in FIT_GROUPS for k in grads):
        raise ValueError(f"grads must be a dict with keys among {FIT_GROUPS}")
    g = []
    for k in FIT_GROUPS:
        t = grads.get(k)
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params[k].numel()):
            raise ValueError(f"grads[{k!r}] must be a contiguous float32 tensor of params[{k!r}]'s size")
        g.append(t)
    size = n * (11 + 3 * n_coef)
    for name in ("m", "v"):
        t = state.get(name) if isinstance(state, dict) else None
        if not torch.is_tensor(t) or tuple(t.shape) != (size,) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"state[{name!r}] must be a contiguous float32 [{size}] tensor (ops.gaussian_adam_state makes the dict)")
    status = state.get("status")
    if not torch.is_tensor(status) or tuple(status.shape) != (1,) or status.dtype != torch.int32:
        raise ValueError("state['status'] must be an int32 [1] tensor")
    if instances is not None and (not torch.is_tensor(instances) or tuple(instances.shape) != (1,) or instances.dtype != torch.int64):
        raise ValueError("instances must be an int64 [1] tensor")
    _need_gpu(*[params[k] for k in FIT_GROUPS], *g, state["m"], state["v"], status, instances)
    rates = (C.c_float * len(FIT_GROUPS))(*lrs)
    check(_lib.load().sixdgs_gaussian_adam(n, n_coef, int(step), *[_p(params[k] if params[k].numel() else None) for k in FIT_GROUPS],
                                           *[_p(t if t is not None and t.numel() else None) for t in g], _p(state["m"]), _p(state["v"]), rates,
                                           float(beta1), float(beta2), float(eps), _p(instances), int(max_instances), _p(status), _stream()),
          "gaussian_adam")


@_on_device
def opacity_reset(opacity: torch.Tensor, m_opacity: Optional[torch.Tensor] = None, v_opacity: Optional[torch.Tensor] = None, *,
                  ceiling: float = 0.01, opacity_is_logit: bool = True) -> None:
    """The reference's reset_opacity, IN PLACE (sixdgs_opacity_reset in include/sixdgs.h): opacity [N] or [N,1] becomes
    min(sigmoid(x), ceiling) in the form it came in, and m_opacity, v_opacity -- the opacity slices of Adam's m and v -- become zero."""
    if not (0.0 < float(ceiling) < 1.0):
        raise ValueError(f"ceiling must be in (0, 1) (got {ceiling})")
    for name, t in (("opacity", opacity), ("m_opacity", m_opacity), ("v_opacity", v_opacity)):
        if t is None and name != "opacity":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != opacity.numel():
            raise ValueError(f"{name} must be a contiguous float32 tensor of opacity's size")
    _need_gpu(opacity, m_opacity, v_opacity)
    check(_lib.load().sixdgs_opacity_reset(_p(opacity), opacity.numel(), int(bool(opacity_is_logit)), _p(m_opacity), _p(v_opacity),
                                           float(ceiling), _stream()), "opacity_reset")


def fit_scene_workspace_bytes(n: int, n_coef: int, batch: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_fit_scene_workspace_bytes(int(n), int(n_coef), int(batch), int(width), int(height), int(max_instances)))


def _fit_args(params, cams, width, height, target, views, lrs, sh_degrees, resets, groups, lambda_dssim, beta1, beta2, eps, reset_ceiling,
              scale_modifier, background, opacity_is_logit):
    """The checks fit_scene_raw and fit_scene_steps_raw share, before _need_gpu -> the arguments in the form the C call takes them."""
    n, n_coef = _fit_params(params)
    lam = _lambda(lambda_dssim)
    _check_fit_hyper(beta1, beta2, eps)
    if not (0.0 < float(reset_ceiling) < 1.0):
        raise ValueError(f"reset_ceiling must be in (0, 1) (got {reset_ceiling})")
    groups = tuple(groups)
    if not groups or any(k not in FIT_GROUPS for k in groups) or len(set(groups)) != len(groups):
        raise ValueError(f"groups must name some of {FIT_GROUPS}, each once (got {groups})")
    cams, width, height = _view_args(cams, width, height, background, scale_modifier)
    n_views = cams.shape[0]
    if n_views < 1:
        raise ValueError("cams must be a [views,16] tensor of at least one view")
    view_t = torch.as_tensor(views).detach().cpu()
    if view_t.dim() != 2 or view_t.shape[0] < 1 or view_t.shape[1] < 1 or view_t.dtype.is_floating_point or view_t.dtype == torch.bool:
        raise ValueError("views must be an integer [steps,batch] array")
    steps, batch = int(view_t.shape[0]), int(view_t.shape[1])
    if int(view_t.min()) < 0 or int(view_t.max()) >= n_views:
        raise ValueError(f"views must index the {n_views} cameras")
    view_t = view_t.to(torch.int32).contiguous()
    lr_t = torch.as_tensor(lrs, dtype=torch.float64).detach().cpu()
    if tuple(lr_t.shape) != (steps, len(FIT_GROUPS)) or not bool(torch.isfinite(lr_t).all()) or bool((lr_t < 0).any()):
        raise ValueError(f"lrs must be [{steps},{len(FIT_GROUPS)}] non-negative finite rates")
    lr_t = lr_t.to(torch.float32).contiguous()
    deg_t = torch.as_tensor(sh_degrees).detach().cpu()
    if tuple(deg_t.shape) != (steps,) or deg_t.dtype.is_floating_point or int(deg_t.min()) < 0 or (int(deg_t.max()) + 1) ** 2 > n_coef:
        raise ValueError(f"sh_degrees must be [{steps}] integers in [0, the degree {n_coef} coefficients allow]")
    deg_t = deg_t.to(torch.int32).contiguous()
    reset_t = torch.zeros(steps, dtype=torch.uint8) if resets is None else torch.as_tensor(resets).detach().cpu().to(torch.bool).to(torch.uint8).contiguous()
    if tuple(reset_t.shape) != (steps,):
        raise ValueError(f"resets must be [{steps}] flags")
    if bool(reset_t.any()) and not opacity_is_logit:
        raise ValueError("an opacity reset needs opacity_is_logit")
    target, target_is_u8, target_stride = _target_args(target, n_views, height, width)
    return (n, n_coef, lam, groups, cams, width, height, n_views, steps, batch, view_t, lr_t, deg_t, reset_t, target, target_is_u8,
            target_stride)


@_on_device
def fit_scene_raw(params: dict, cams: torch.Tensor, width: int, height: int, target: torch.Tensor, *, views, lrs, sh_degrees, resets=None,
                  groups=FIT_GROUPS, lambda_dssim: float = 0.2, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-15,
                  reset_ceiling: float = 0.01, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0), scale_is_log: bool = True,
                  opacity_is_logit: bool = True, max_instances: Optional[int] = None, retry: bool = True) -> dict:
    """Fit the six arrays of `params` (a dict by FIT_GROUPS' names, UPDATED IN PLACE) to posed views as ONE library call
    (sixdgs_fit_scene in include/sixdgs.h): per step a render of the step's views, the loss, the backward, one Adam step and -- where
    asked -- the opacity reset, enqueued without a host read.  cams [V,16]; target fp32 [V,height,width,3|4] or uint8 [V,height,width,3];
    views int [steps,batch] (indices into cams, duplicates allowed), lrs [steps,6] in FIT_GROUPS' order, sh_degrees [steps],
    resets [steps] (None: never); groups: the names that move (the others stay bit for bit and get no gradient).
    Returns a dict: history [steps,batch], m, v, status (int32 [1]; bit 0: a gradient entry was not finite and was left out, bit 1: the
    instance capacity was too small), instances_needed (int) and max_instances (int: the capacity of the run returned).  The call
    runs with raster_instances_estimate's capacity (or max_instances), reads status and instances_needed once at the end, and -- with
    retry -- on bit 1 puts back the copy of the scene it took before the call and runs once more with 5/4 of the needed capacity."""
    (n, n_coef, lam, groups, cams, width, height, n_views, steps, batch, view_t, lr_t, deg_t, reset_t, target, target_is_u8,
     target_stride) = _fit_args(params, cams, width, height, target, views, lrs, sh_degrees, resets, groups, lambda_dssim, beta1, beta2, eps,
                                reset_ceiling, scale_modifier, background, opacity_is_logit)
    capacity = _capacity(max_instances, n, batch)
    arrays = [params[k] for k in SCENE_ARRAYS]
    _need_gpu(*arrays, cams, target)
    lib = _lib.load()
    dev = cams.device
    bg = _background(background, dev)
    size = n * (11 + 3 * n_coef)
    out = {"history": torch.empty(steps, batch, device=dev), "m": torch.empty(size, device=dev), "v": torch.empty(size, device=dev),
           "status": torch.empty(1, dtype=torch.int32, device=dev)}
    needed_t = torch.zeros(1, dtype=torch.int64, device=dev)
    mask = sum(1 << FIT_GROUPS.index(k) for k in groups)
    saved = [t.clone() for t in arrays] if retry else None      # a run that overflowed has moved the scene up to that step
    needed = 0
    for attempt in range(2):
        need = lib.sixdgs_fit_scene_workspace_bytes(n, n_coef, batch, width, height, capacity)
        if need == 0:
            raise ValueError(f"sizes outside the rasteriser's limits (n {n}, batch {batch}, {width} x {height}, instances {capacity})")
        ws, ws_bytes = _workspace(None, need, dev)
        check(lib.sixdgs_fit_scene(*_scene_args(arrays, n_coef, scale_is_log, opacity_is_logit), n_coef, n, _p(cams), n_views, width, height,
                                   float(scale_modifier), _p(bg), _p(target), target_is_u8, target_stride, lam, steps, batch, _p(view_t),
                                   _p(lr_t), _p(deg_t), _p(reset_t), mask, float(beta1), float(beta2), float(eps), float(reset_ceiling),
                                   capacity, _p(out["m"]), _p(out["v"]), _p(out["history"]), _p(out["status"]), _p(needed_t), _p(ws), ws_bytes,
                                   _stream()),
              "fit_scene")
        # the one host read of the call: the status word and the largest instance count seen
        flags = torch.cat([out["status"].to(torch.int64), needed_t]).cpu()
        needed = int(flags[1])
        if not retry or not int(flags[0]) & FIT_STATUS_CAPACITY:
            break
        if attempt == 1 or needed > RASTER_MAX_INSTANCES:
            raise RuntimeError(f"6dgs_amd: fit_scene still needs {needed} tile instances after {attempt + 1} runs (limit 2^31 - 1): "
                               "fit fewer views at once")
        for t, s in zip(arrays, saved):
            t.copy_(s)
        capacity = _grown(needed)
    out["instances_needed"] = needed
    out["max_instances"] = capacity
    return out


# ---------------------------------------------------------------------------------------------
# adaptive density control below the C ABI
# ---------------------------------------------------------------------------------------------
DENSIFY_STATS = (("grad_accum", torch.float32), ("denom", torch.int32), ("max_radii", torch.int32))


def densify_stats_state(n: int, device) -> dict:
    """The statistics a densification round reads, zeroed: grad_accum float32 [n], denom int32 [n], max_radii int32 [n]."""
    return {k: torch.zeros(int(n), dtype=dt, device=device) for k, dt in DENSIFY_STATS}


def _check_stats(stats, n):
    if not isinstance(stats, dict):
        raise ValueError("stats must be the dict of ops.densify_stats_state")
    for k, dt in DENSIFY_STATS:
        t = stats.get(k)
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"stats[{k!r}] must be a contiguous {dt} [{n}] tensor (ops.densify_stats_state makes the dict)")


def densify_thresholds(*, grad_threshold, percent_dense, extent, min_opacity, scale_is_log: bool = True, opacity_is_logit: bool = True) -> dict:
    """The thresholds of a round in the domain the arrays are stored in, as sixdgs_densify forms them: each converted once, in double,
    from the float32 arguments and rounded to float32.  Keys grad, dense, world, opacity (Python floats holding float32 values)."""
    f = lambda x: C.c_float(float(x)).value
    dense, world, p = f(percent_dense) * f(extent), 0.1 * f(extent), f(min_opacity)
    if not (f(grad_threshold) > 0.0 and dense > 0.0 and 0.0 <= p < 1.0) or not all(math.isfinite(x) for x in (f(grad_threshold), dense)):
        raise ValueError("grad_threshold, percent_dense and extent must be positive and finite, min_opacity in [0, 1)")
    if scale_is_log:
        dense, world = math.log(dense), math.log(world)
    if opacity_is_logit:
        p = math.log(p / (1.0 - p)) if p > 0.0 else float("-inf")
    return {"grad": f(grad_threshold), "dense": f(dense), "world": f(world), "opacity": f(p)}


@_on_device
def densify_stats(state, bwd_workspace: torch.Tensor, radii: torch.Tensor, stats: dict, width: int, height: int, *, want_grad2d: bool = False,
                  status: Optional[torch.Tensor] = None):
    """Accumulate the densification statistics of one render pass IN PLACE (sixdgs_densify_stats in include/sixdgs.h): state = the
    (workspace, capacity) pair of raster_views(..., want_state=True, want_radii=True), bwd_workspace = the tensor
    raster_views_backward(..., workspace=...) ran in on the same arguments, radii int32 [V,N] the forward's.  Per visible (view,
    Gaussian): grad_accum += the norm of the NDC-position gradient, denom += 1, max_radii = max(max_radii, radius).  Returns grad2d
    float32 [V,N,2] -- the raw (du, dv), zeros where invisible -- with want_grad2d, else None."""
    if (not isinstance(state, (tuple, list)) or len(state) != 2 or not torch.is_tensor(state[0])
            or not 1 <= int(state[1]) <= RASTER_MAX_INSTANCES):
        raise ValueError("state must be the (workspace, capacity) pair of raster_views(..., want_state=True)")
    fwd_ws, capacity = state[0], int(state[1])
    if int(width) < 1 or int(height) < 1:
        raise ValueError(f"width and height must be positive (got {width} x {height})")
    if not torch.is_tensor(radii) or radii.dim() != 2 or radii.dtype != torch.int32 or not radii.is_contiguous():
        raise ValueError("radii must be a contiguous int32 [views,n] tensor")
    if not torch.is_tensor(bwd_workspace):
        raise ValueError("bwd_workspace must be the workspace tensor of raster_views_backward")
    views, n = int(radii.shape[0]), int(radii.shape[1])
    _check_stats(stats, n)
    if status is not None and (not torch.is_tensor(status) or tuple(status.shape) != (1,) or status.dtype != torch.int32):
        raise ValueError("status must be an int32 [1] tensor")
    _need_gpu(fwd_ws, bwd_workspace, radii, *[stats[k] for k, _ in DENSIFY_STATS], status)
    grad2d = torch.zeros(views, n, 2, device=radii.device) if want_grad2d else None
    check(_lib.load().sixdgs_densify_stats(n, views, int(width), int(height), capacity, _p(fwd_ws), fwd_ws.numel() * fwd_ws.element_size(),
                                           _p(bwd_workspace), bwd_workspace.numel() * bwd_workspace.element_size(), _p(radii),
                                           _p(stats["grad_accum"]), _p(stats["denom"]), _p(stats["max_radii"]), _p(grad2d), _p(status),
                                           _stream()),
          "densify_stats")
    return grad2d


def densify_workspace_bytes(n: int) -> int:
    return int(_lib.load().sixdgs_densify_workspace_bytes(int(n)))


def densify_buffers(params: dict, n_cap: int) -> dict:
    """Output buffers of n_cap rows for densify_raw: the six arrays in the shapes of `params`, m and v of n_cap (11 + 3 n_coef) floats."""
    n, n_coef = _fit_params(params)
    out = {k: torch.empty((int(n_cap), *params[k].shape[1:]), device=params[k].device) for k in FIT_GROUPS}
    for k in ("m", "v"):
        out[k] = torch.empty(int(n_cap) * (11 + 3 * n_coef), device=params["xyz"].device)
    return out


def densify_raw(params: dict, state: dict, stats: dict, noise: torch.Tensor, out: dict, *, grad_threshold: float, percent_dense: float,
                extent: float, min_opacity: float, prune_big: bool, screen_size: int = 0, scale_is_log: bool = True,
                opacity_is_logit: bool = True, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One densification round as ONE library call, out of place and without a host read (sixdgs_densify in include/sixdgs.h): from
    params (dict by FIT_GROUPS' names), state (gaussian_adam_state's dict: m, v, status), stats (densify_stats_state's dict) and noise
    float32 [n,2,3] (standard normals) into `out` (densify_buffers' dict; its row count is the capacity).  Returns counts, int64 [4] on
    the device: n_out, clones, split sources, candidates pruned.  The first n_out rows of the six arrays and the first
    n_out (11 + 3 n_coef) floats of out["m"], out["v"] are written, nothing else; if n_out exceeds the capacity only counts and bit 1
    of state["status"] are."""
    _fit_params(params)
    return _densify_raw(params["xyz"], params, state, stats, noise, out, grad_threshold, percent_dense, extent, min_opacity, prune_big,
                        screen_size, scale_is_log, opacity_is_logit, workspace)


@_on_device
def _densify_raw(anchor, params, state, stats, noise, out, grad_threshold, percent_dense, extent, min_opacity, prune_big, screen_size,
                 scale_is_log, opacity_is_logit, workspace):
    n, n_coef = _fit_params(params)
    densify_thresholds(grad_threshold=grad_threshold, percent_dense=percent_dense, extent=extent, min_opacity=min_opacity,
                       scale_is_log=scale_is_log, opacity_is_logit=opacity_is_logit)
    if isinstance(screen_size, bool) or int(screen_size) != screen_size or int(screen_size) < 0:
        raise ValueError(f"screen_size must be a non-negative integer (got {screen_size})")
    _check_stats(stats, n)
    size = n * (11 + 3 * n_coef)
    for name in ("m", "v"):
        t = state.get(name) if isinstance(state, dict) else None
        if not torch.is_tensor(t) or tuple(t.shape) != (size,) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"state[{name!r}] must be a contiguous float32 [{size}] tensor (ops.gaussian_adam_state makes the dict)")
    status = state.get("status")
    if not torch.is_tensor(status) or tuple(status.shape) != (1,) or status.dtype != torch.int32:
        raise ValueError("state['status'] must be an int32 [1] tensor")
    if not torch.is_tensor(noise) or tuple(noise.shape) != (n, 2, 3) or noise.dtype != torch.float32 or not noise.is_contiguous():
        raise ValueError(f"noise must be a contiguous float32 [{n},2,3] tensor")
    if not isinstance(out, dict) or any(k not in out for k in FIT_GROUPS + ("m", "v")):
        raise ValueError("out must be the dict of ops.densify_buffers")
    n_cap = int(out["xyz"].shape[0])
    for k in FIT_GROUPS:
        t = out[k]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n_cap, *params[k].shape[1:]):
            raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor of {n_cap} rows in the shape of params[{k!r}]")
    for k in ("m", "v"):
        t = out[k]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n_cap * (11 + 3 * n_coef):
            raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor of at least {n_cap * (11 + 3 * n_coef)} entries")
    _need_gpu(*[params[k] for k in FIT_GROUPS], state["m"], state["v"], status, *[stats[k] for k, _ in DENSIFY_STATS], noise,
              *[out[k] for k in FIT_GROUPS + ("m", "v")], workspace)
    lib = _lib.load()
    dev = params["xyz"].device
    ws, ws_bytes = _workspace(workspace, lib.sixdgs_densify_workspace_bytes(n), dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    some = lambda t: _p(t if t.numel() else None)
    check(lib.sixdgs_densify(n, n_coef, *[some(params[k]) for k in FIT_GROUPS], int(bool(scale_is_log)), int(bool(opacity_is_logit)),
                             some(state["m"]), some(state["v"]), some(stats["grad_accum"]), some(stats["denom"]), some(stats["max_radii"]),
                             some(noise), float(grad_threshold), float(percent_dense), float(extent), float(min_opacity), int(bool(prune_big)),
                             int(screen_size), n_cap, *[some(out[k]) for k in FIT_GROUPS], some(out["m"]), some(out["v"]), _p(counts),
                             _p(status), _p(ws), ws_bytes, _stream()),
          "densify")
    return counts


def densify(params: dict, state: dict, stats: dict, noise: torch.Tensor, *, grad_threshold: float, percent_dense: float, extent: float,
            min_opacity: float, prune_big: bool, screen_size: int = 0, scale_is_log: bool = True, opacity_is_logit: bool = True):
    """One densification round (densify_raw into buffers of 2 n rows, which always fit) -> (new params, new state, counts): dicts like
    the inputs at n_out rows -- views of the buffers --, the status tensor carried over, counts int64 [4] on the device.  One 8-byte
    host read: n_out."""
    n, n_coef = _fit_params(params)
    out = densify_buffers(params, 2 * n)
    counts = densify_raw(params, state, stats, noise, out, grad_threshold=grad_threshold, percent_dense=percent_dense, extent=extent,
                         min_opacity=min_opacity, prune_big=prune_big, screen_size=screen_size, scale_is_log=scale_is_log,
                         opacity_is_logit=opacity_is_logit)
    n_out = int(counts[0].item())
    size = n_out * (11 + 3 * n_coef)
    return ({k: out[k][:n_out] for k in FIT_GROUPS}, {"m": out["m"][:size], "v": out["v"][:size], "status": state["status"]}, counts)


def knn_workspace_bytes(n: int) -> int:
    return int(_lib.load().sixdgs_knn_workspace_bytes(int(n)))


@_on_device
def knn_mean_dist2(xyz: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mean squared distance of every point to its three nearest OTHER points (sixdgs_knn_mean_dist2 in include/sixdgs.h: exact, the
    bits of an fp32 brute force; the reference's distCUDA2) -> float32 [n].  xyz: contiguous float32 [n,3] on the GPU, finite, n == 0
    or n >= 4.  One stream-ordered call, no host read."""
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise ValueError("xyz must be a contiguous float32 [n,3] tensor")
    n = int(xyz.shape[0])
    if 1 <= n <= 3:
        raise ValueError(f"knn_mean_dist2 needs at least 4 points: every point has three neighbours (got {n})")
    if workspace is not None and (not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or not workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous uint8 tensor")
    _need_gpu(xyz, workspace)
    out = torch.empty(n, dtype=torch.float32, device=xyz.device)
    if n == 0:
        return out
    lib = _lib.load()
    ws, ws_bytes = _workspace(workspace, lib.sixdgs_knn_workspace_bytes(n), xyz.device)
    check(lib.sixdgs_knn_mean_dist2(n, _p(xyz.detach()), _p(out), _p(ws), ws_bytes, _stream()), "knn_mean_dist2")
    return out


def fit_scene_steps_workspace_bytes(n: int, n_coef: int, batch: int, width: int, height: int, max_instances: int) -> int:
    return int(_lib.load().sixdgs_fit_scene_steps_workspace_bytes(int(n), int(n_coef), int(batch), int(width), int(height), int(max_instances)))


@_on_device
def fit_scene_steps_raw(params: dict, cams: torch.Tensor, width: int, height: int, target: torch.Tensor, state: dict, *, views, lrs, sh_degrees,
                        resets=None, updates=None, stats_steps=None, stats: Optional[dict] = None, first_adam_step: int = 0,
                        groups=FIT_GROUPS, lambda_dssim: float = 0.2, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-15,
                        reset_ceiling: float = 0.01, scale_modifier: float = 1.0, background=(1.0, 1.0, 1.0), scale_is_log: bool = True,
                        opacity_is_logit: bool = True, max_instances: Optional[int] = None,
                        workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A segment of a fit as ONE library call with caller-kept state (sixdgs_fit_scene_steps in include/sixdgs.h): fit_scene_raw's
    loop on `params` IN PLACE, from and into `state` -- m, v, status (gaussian_adam_state's dict) and instances_needed (int64 [1]) --
    which the call does not zero and never reads back.  updates [steps] (None: all): a cleared flag makes no Adam update at that step,
    and Adam's counter, which starts at first_adam_step, does not advance.  stats_steps [steps] (None: none): a set flag accumulates
    the densification statistics of that step's pass into `stats` (densify_stats_state's dict).  Returns history [steps,batch]; the
    caller reads state["status"] when it wants to know about the capacity (bit 1) -- nothing is retried here."""
    (n, n_coef, lam, groups, cams, width, height, n_views, steps, batch, view_t, lr_t, deg_t, reset_t, target, target_is_u8,
     target_stride) = _fit_args(params, cams, width, height, target, views, lrs, sh_degrees, resets, groups, lambda_dssim, beta1, beta2, eps,
                                reset_ceiling, scale_modifier, background, opacity_is_logit)
    flags = []
    for name, f in (("updates", updates), ("stats_steps", stats_steps)):
        t = None if f is None else torch.as_tensor(f).detach().cpu().to(torch.bool).to(torch.uint8).contiguous()
        if t is not None and tuple(t.shape) != (steps,):
            raise ValueError(f"{name} must be [{steps}] flags")
        flags.append(t)
    update_t, stats_t = flags
    if isinstance(first_adam_step, bool) or int(first_adam_step) != first_adam_step or int(first_adam_step) < 0:
        raise ValueError(f"first_adam_step must be a non-negative integer (got {first_adam_step})")
    wants_stats = stats_t is not None and bool(stats_t.any())
    if wants_stats or stats is not None:
        _check_stats(stats, n)
    size = n * (11 + 3 * n_coef)
    for name, shape, dt in (("m", (size,), torch.float32), ("v", (size,), torch.float32), ("status", (1,), torch.int32),
                            ("instances_needed", (1,), torch.int64)):
        t = state.get(name) if isinstance(state, dict) else None
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"state[{name!r}] must be a contiguous {dt} {list(shape)} tensor")
    capacity = _capacity(max_instances, n, batch)
    arrays = [params[k] for k in SCENE_ARRAYS]
    st = [stats[k] for k, _ in DENSIFY_STATS] if stats is not None else [None] * 3
    _need_gpu(*arrays, cams, target, state["m"], state["v"], state["status"], state["instances_needed"], *st, workspace)
    lib = _lib.load()
    dev = cams.device
    bg = _background(background, dev)
    history = torch.empty(steps, batch, device=dev)
    mask = sum(1 << FIT_GROUPS.index(k) for k in groups)
    need = lib.sixdgs_fit_scene_steps_workspace_bytes(n, n_coef, batch, width, height, capacity)
    if need == 0:
        raise ValueError(f"sizes outside the rasteriser's limits (n {n}, batch {batch}, {width} x {height}, instances {capacity})")
    ws, ws_bytes = _workspace(workspace, need, dev)
    some = lambda t: _p(t if t is not None and t.numel() else None)
    check(lib.sixdgs_fit_scene_steps(*_scene_args(arrays, n_coef, scale_is_log, opacity_is_logit), n_coef, n, _p(cams), n_views, width, height,
                                     float(scale_modifier), _p(bg), _p(target), target_is_u8, target_stride, lam, steps, batch, _p(view_t),
                                     _p(lr_t), _p(deg_t), _p(reset_t), _p(update_t), _p(stats_t), int(first_adam_step), mask, float(beta1),
                                     float(beta2), float(eps), float(reset_ceiling), capacity, some(state["m"]), some(state["v"]), _p(history),
                                     _p(state["status"]), _p(state["instances_needed"]), *[some(t) for t in st], _p(ws), ws_bytes, _stream()),
          "fit_scene_steps")
    return history


# ---------------------------------------------------------------------------------------------
# scorer
# ---------------------------------------------------------------------------------------------
class PackedWeights:
    """Device copy of the scorer weights in the kernels' padded layout + the C struct of pointers."""

    KEYS = ("ray_preprocessor.mlp.0", "ray_preprocessor.mlp.2", "ray_preprocessor.mlp2.0", "ray_preprocessor.mlp2.2",
            "attention.k_proj", "attention.q_proj")

    @_on_device
    def __init__(self, state_dict, device):
        lib = _lib.load()
        srcs = []
        for k in self.KEYS:
            srcs.append(_f32(state_dict[k + ".weight"]).to(device))
            srcs.append(_f32(state_dict[k + ".bias"]).to(device))
        self._srcs = srcs
        self.buffer = torch.empty(lib.sixdgs_packed_weights_floats(), device=device)
        self.device = self.buffer.device
        self.struct = ScorerWeights()
        check(lib.sixdgs_pack_weights(*[_p(t) for t in srcs], _p(self.buffer), C.byref(self.struct), _stream()), "pack_weights")

    @property
    def ref(self):
        return C.byref(self.struct)


class KernelProfile:
    """Caller-owned HIP-event timing of the dominant kernel (see sixdgs_profile in include/sixdgs.h)."""

    def __init__(self):
        self.struct = Profile()
        self.struct.count = 0

    @property
    def ref(self):
        return C.byref(self.struct)

    def collect(self):
        """-> (milliseconds, algorithmic FLOP, algorithmic bytes, launches); waits for the recorded events."""
        ms, fl, by, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int(0)
        check(_lib.load().sixdgs_profile_collect(self.ref, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), "profile_collect")
        return ms.value, fl.value, by.value, n.value


@_on_device
def ray_encode(ori, dr, rgb) -> torch.Tensor:
    ori, dr, rgb = _f32(ori), _f32(dr), _f32(rgb)
    _need_gpu(ori, dr, rgb)
    x = torch.empty(ori.shape[0], RAY_IN_PAD, device=ori.device)
    check(_lib.load().sixdgs_ray_encode(_p(ori), _p(dr), _p(rgb), ori.shape[0], _p(x), _stream()), "ray_encode")
    return x


@_on_device
def linear(x, w, b=None, relu: bool = False, mma_mode: Optional[int] = None, split_k: Optional[int] = None) -> torch.Tensor:
    """y = x w^T + b (optionally ReLU).  split_k: None = automatic (K is cut into slices computed by separate workgroups when
    the output has too few 128x128 tiles to fill the 256 CUs and K is long), 1 = never, n = that many slices."""
    x, w = _f32(x), _f32(w)
    _need_gpu(x, w)
    b = _f32(b) if b is not None else None
    lib = _lib.load()
    m, k, n = x.shape[0], x.shape[1], w.shape[0]
    y = torch.empty(m, n, device=x.device)
    mode = _mma_mode if mma_mode is None else mma_mode
    if split_k is None:
        tiles = -(-m // 128) * -(-n // 128)
        split_k = 1 if (tiles >= 128 or k < 2048 or m == 0) else max(1, min(k // 256, -(-512 // tiles)))
    if split_k > 1:
        ws = torch.empty(lib.sixdgs_linear_splitk_workspace_bytes(m, n, split_k), dtype=torch.uint8, device=x.device)
        check(lib.sixdgs_linear_splitk(_p(x), m, k, x.stride(0), _p(w), w.stride(0), _p(b), n, int(relu), _p(y), y.stride(0), int(split_k),
                                       _p(ws), ws.numel(), _stream(), mode), "linear_splitk")
    else:
        check(lib.sixdgs_linear_ex(_p(x), m, k, x.stride(0), _p(w), w.stride(0), _p(b), n, int(relu), _p(y), y.stride(0), _stream(), mode),
              "linear")
    return y


TOK_ATTENTION_MAX_TOKENS = 288


def _tok_out_ok(y: torch.Tensor, m: int, n: int, what: str) -> None:
    """The output of a ViT stage kernel: the caller's `out` is written as it lies (any row stride the kernel accepts), so its shape is checked here --
    the kernels store m rows of n floats whatever the tensor holds."""
    if y.dtype != torch.float32 or tuple(y.shape) != (m, n) or (n > 1 and y.stride(1) != 1) or not y.is_cuda:
        raise RuntimeError(f"6dgs_amd: {what} needs a float32 GPU output [{m}, {n}] with unit column stride, got {y.dtype} {tuple(y.shape)} strides {tuple(y.stride())}")


@_on_device
def tok_attention(qkv: torch.Tensor, images: int, tokens: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T / 8) v per image and head on the QKV product's output [images * tokens, 3 * heads * 64] as it lies (q | k | v, head h at columns
    h * 64 of each) -> [images * tokens, heads * 64], token-major (sixdgs_tok_attention; head dimension 64, tokens <= 288)."""
    qkv = qkv.detach()
    if qkv.dtype != torch.float32 or qkv.dim() != 2 or qkv.shape[0] != images * tokens or qkv.shape[1] != 3 * heads * 64 or qkv.stride(1) != 1:
        raise RuntimeError(f"6dgs_amd: tok_attention needs float32 qkv [{images * tokens}, {3 * heads * 64}], got {qkv.dtype} {tuple(qkv.shape)}")
    _need_gpu(qkv)
    y = out if out is not None else torch.empty(images * tokens, heads * 64, device=qkv.device)
    _tok_out_ok(y, images * tokens, heads * 64, "tok_attention")
    check(_lib.load().sixdgs_tok_attention(_p(qkv), qkv.stride(0), int(images), int(tokens), int(heads), _p(y), y.stride(0), _stream()), "tok_attention")
    return y


@_on_device
def im2col(x: torch.Tensor, k: int, taps_major: bool = False) -> torch.Tensor:
    """[B, C, H, W] fp32 (ANY strides: a permuted view of a [B*H*W, C] GEMM output is read in place) -> the A matrix [B*ho*wo, C*k*k] of the valid
    k x k convolution (sixdgs_im2col): columns in conv.weight.view(out, -1) order -- torch.nn.functional.unfold + transpose + contiguous in one launch --
    or, taps_major, in (ky, kx, c) order for a weight permuted as weight.permute(0, 2, 3, 1).reshape(out, -1) (plain 16-byte copies when the input's
    channel stride is 1)."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError(f"6dgs_amd: im2col needs a float32 [B, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    x = x.detach()
    _need_gpu(x)
    b, c, h, w = x.shape
    if h < k or w < k:
        raise RuntimeError(f"6dgs_amd: im2col: a {k} x {k} window does not fit a {h} x {w} map")
    a = torch.empty(b * (h - k + 1) * (w - k + 1), c * k * k, device=x.device)
    check(_lib.load().sixdgs_im2col(_p(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), b, c, h, w, int(k), 1 if taps_major else 0, _p(a), _stream()),
          "im2col")
    return a


@_on_device
def u8_to_planar(images_u8: torch.Tensor, table256: torch.Tensor) -> torch.Tensor:
    """[B, H, W, 3] uint8 -> [B, 3, H, W] fp32 = table256[value] (sixdgs_u8_to_planar; H*W a multiple of 4)."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3 or (images_u8.shape[1] * images_u8.shape[2]) % 4:
        raise RuntimeError(f"6dgs_amd: u8_to_planar needs uint8 [B, H, W, 3] with H*W a multiple of 4, got {images_u8.dtype} {tuple(images_u8.shape)}")
    x = images_u8.contiguous()
    t = _f32(table256)
    _need_gpu(x, t)
    if t.numel() != 256:
        raise RuntimeError("6dgs_amd: u8_to_planar needs a 256-entry table")
    b, h, w, _ = x.shape
    out = torch.empty(b, 3, h, w, device=x.device)
    check(_lib.load().sixdgs_u8_to_planar(_p(x), b, h * w, _p(t), _p(out), _stream()), "u8_to_planar")
    return out


def image_prep_geometry(h: int, w: int, resize: int = 256, crop: int = 224):
    """The geometry of torchvision's Resize(resize) + CenterCrop(crop) on an h x w image, as BackboneWrapper applies them (backbone.py:52-77):
    -> (resized_h, resized_w, crop_top, crop_left)."""
    if h <= w:
        nh, nw = resize, int(resize * w / h)
    else:
        nh, nw = int(resize * h / w), resize
    return nh, nw, int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))


def image_prep_enabled() -> bool:
    """SIXDGS_IMAGE_PREP=0: uniform RGB batches go through sixdgs_u8_to_planar + PyTorch's antialiased resize, crop and normalisation as before round 6's last step."""
    return os.environ.get("SIXDGS_IMAGE_PREP", "1") != "0"


@_on_device
def image_prep(images_u8: torch.Tensor, table256: torch.Tensor, mean, std, resize: int = 256, crop: int = 224) -> Optional[torch.Tensor]:
    """[B, H, W, 3] uint8 -> [B, 3, crop, crop] fp32 = Normalize(CenterCrop(Resize_bicubic_antialias(table256[value]))) in one launch (sixdgs_image_prep);
    None when the kernel does not take the shape (the caller then uses PyTorch's kernels).  mean / std: three floats each."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise RuntimeError(f"6dgs_amd: image_prep needs uint8 [B, H, W, 3], got {images_u8.dtype} {tuple(images_u8.shape)}")
    x = images_u8.contiguous()
    t = _f32(table256)
    _need_gpu(x, t)
    b, h, w, _ = x.shape
    nh, nw, top, left = image_prep_geometry(h, w, resize, crop)
    if (nh, nw) == (h, w) or nh < crop or nw < crop or t.numel() != 256:
        return None
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    out = torch.empty(b, 3, crop, crop, device=x.device)
    st = _lib.load().sixdgs_image_prep(_p(x), b, h, w, _p(t), nh, nw, top, left, crop, m3, s3, _p(out), _stream())
    if st == -3:                  # SIXDGS_E_UNSUPPORTED: scale / window beyond the kernel's LDS
        return None
    check(st, "image_prep")
    return out


TOK_A_PLAIN, TOK_A_LAYERNORM = 0, 1
TOK_EPI_BIAS, TOK_EPI_GELU, TOK_EPI_RESID = 0, 1, 2


class TokWeights:
    """A dense layer's weight matrix [n, k] as sixdgs_tok_linear wants it: two scaled fp16 planes in the matrix pipe's operand order + reciprocal row
    scales (sixdgs_tok_pack; n a multiple of 128, k of 384).  Built once per weight tensor: `TokWeights.of(w)` keeps the pack on a side table keyed
    by the tensor OBJECT (weak reference), its storage address and its version counter, so an optimiser step, load_state_dict, .to() or a new tensor
    that happens to land on a freed tensor's address re-packs."""
    _cache: dict = {}

    def __init__(self, w: torch.Tensor):
        w = _f32(w)
        _need_gpu(w)
        self.n, self.k = int(w.shape[0]), int(w.shape[1])
        lib = _lib.load()
        self.planes = torch.empty(lib.sixdgs_tok_pack_bytes(self.n, self.k), dtype=torch.uint8, device=w.device)
        self.inv_scale = torch.empty(self.n, dtype=torch.float32, device=w.device)
        check(lib.sixdgs_tok_pack(_p(w), self.n, self.k, w.stride(0), _p(self.planes), _p(self.inv_scale), _stream()), "tok_pack")
        # the pack is kept for the life of the weight and may be read next from ANOTHER stream (a pipeline's image stream, a graph captured elsewhere):
        # finish it here, once per weight (48 x ~25 us for a ViT-S/14), instead of carrying an event through every later call
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(w.device).synchronize()

    @classmethod
    def of(cls, w: torch.Tensor) -> "TokWeights":
        import weakref
        key = id(w)
        hit = cls._cache.get(key)
        if hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.data_ptr():
            return hit[3]
        if w.dim() != 2:
            raise RuntimeError(f"6dgs_amd: a dense layer's weight is [n, k], got {tuple(w.shape)}")
        for k_ in [k_ for k_, v_ in cls._cache.items() if v_[0]() is None]:      # packs of tensors that are gone (an evaluation sweep loads a module per scene)
            del cls._cache[k_]
        with torch.cuda.device(w.device):
            tw = cls(w)
        cls._cache[key] = (weakref.ref(w), w._version, w.data_ptr(), tw)
        return tw


@_on_device
def tok_linear(x: torch.Tensor, w, b: Optional[torch.Tensor] = None, *, ln=None, epilogue: int = TOK_EPI_BIAS, residual: Optional[torch.Tensor] = None,
               gamma: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backbone stage's dense product with its neighbours folded in (include/sixdgs.h: sixdgs_tok_linear).  w: the layer's weight [n, k] (packed
    on first use, TokWeights.of) or a TokWeights.
      x [M, K] rows (row stride free);  ln=(weight, bias, eps): LayerNorm over K = 384 in front of the product;
      epilogue TOK_EPI_BIAS / _GELU / _RESID (residual [M, N] + gamma [N] * (. + b); out may be the residual tensor)."""
    tw = w if isinstance(w, TokWeights) else TokWeights.of(w)
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() != 2 or x.shape[1] != tw.k:
        raise RuntimeError(f"6dgs_amd: tok_linear needs x [M, {tw.k}], got {tuple(x.shape)}")
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    _need_gpu(x, tw.planes)
    b = _f32(b) if b is not None else None
    n, k = tw.n, tw.k
    a_mode, ln_w, ln_b, eps = TOK_A_PLAIN, None, None, 0.0
    if ln is not None:
        a_mode, ln_w, ln_b, eps = TOK_A_LAYERNORM, _f32(ln[0]), _f32(ln[1]), float(ln[2])
    m = x.shape[0]
    y = out if out is not None else torch.empty(m, n, device=x.device)
    _tok_out_ok(y, m, n, "tok_linear")
    res = None
    if residual is not None:
        if tuple(residual.shape) != (m, n):
            raise RuntimeError(f"6dgs_amd: tok_linear needs a residual [{m}, {n}], got {tuple(residual.shape)}")
        res = residual.detach()
        # a row-strided view (ldr > n) is read where it lies, like x: a copy here would also turn `out is residual` into an out-of-place call
        if res.dtype != torch.float32 or res.stride(1) != 1 or res.stride(0) % 4 != 0 or res.data_ptr() % 16 != 0:
            res = _f32(res)
    check(_lib.load().sixdgs_tok_linear(_p(x), m, k, x.stride(0), a_mode, _p(ln_w), _p(ln_b), eps, _p(tw.planes), _p(tw.inv_scale), _p(b), n, int(epilogue),
                                        _p(res), res.stride(0) if res is not None else 0, _p(_f32(gamma)) if gamma is not None else None, _p(y), y.stride(0),
                                        _stream()), "tok_linear")
    return y


@_on_device
def split_planes_f16(x: torch.Tensor):
    """fp32 [rows,384] -> (scaled fp16 planes as uint8 [rows,1536], reciprocal power-of-two scale of every 128-row tile)."""
    x = _f32(x)
    _need_gpu(x)
    out = torch.empty(x.shape[0], 1536, dtype=torch.uint8, device=x.device)
    scale = torch.empty((x.shape[0] + 127) // 128, device=x.device)
    check(_lib.load().sixdgs_split_planes_f16(_p(x), x.shape[0], x.stride(0), _p(out), _p(scale), _stream()), "split_planes_f16")
    return out, scale


# rays per launch of the ray-MLP chain: 2^20 (6.9 GB of workspace).  A persistent workgroup then walks ~32 tile passes per launch instead of 8, and
# the chain runs 3-4 % faster than with 2^18 (fewer launch tails); any chunking gives the same keys bit for bit.
RAY_KEYS_CHUNK = 1 << 20
RAY_KEYS_CHUNK_MIN = 1 << 16


class Arena:
    """ONE device buffer from which the big per-scene buffers are carved: key planes (1536 B per ray), the select workspace (20 B per ray and image), the
    ray-MLP chain's workspace, a streamed scene's U and chunk planes.  An evaluation sweep walks scenes of very different sizes
    (pretrain_eval_attention.py:224-247: 19 M to 392 M rays in the stand-in sweep): through PyTorch's caching allocator every larger scene meant a new
    100-200 GB hipMalloc (pages mapped and cleared at 30-75 GB/s: seconds) and, because a cached block that small tensors have split can neither be reused
    nor released, an `empty_cache()` between scenes that re-paid it for EVERY scene (round 4: 38 s of set-up against 28 s of evaluation).  The ABI's own
    rule -- the caller provides the workspace -- points at one allocation made once: a bump allocator, reset per scene, with scopes for what lives
    shorter (a chunk of a streamed scene).  Everything carved from it is used on ONE stream (reuse is ordered by the stream); the pipeline's image
    stream never touches it.  Opt-in: `with ops.use_arena(arena): ...` / `ops.set_arena(arena)`; without one the allocations go to torch as before."""

    def __init__(self, nbytes: int, device):
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.off, self.high = 0, 0
        self._owner = None          # weakref to the ONE module whose per-scene buffers live here (reset(owner) claims it)

    @property
    def capacity(self) -> int:
        return int(self.buf.numel())

    def take(self, nbytes: int, align: int = 4096) -> torch.Tensor:
        base = self.buf.data_ptr()
        off = (base + self.off + align - 1) // align * align - base          # the ADDRESS is aligned (kernels ask for 16 .. 256 B; 4 KB keeps pages apart)
        if off + int(nbytes) > self.buf.numel():
            raise RuntimeError(f"6dgs_amd: arena exhausted ({off + int(nbytes)} of {self.buf.numel()} bytes asked for)")
        self.off = off + int(nbytes)
        self.high = max(self.high, self.off)
        return self.buf[off:self.off]

    def mark(self) -> int:
        return self.off

    def release(self, mark: int) -> None:
        self.off = int(mark)

    def reset(self, owner=None) -> None:
        """Everything carved so far is handed out again.  `owner`: the module doing so -- an arena serves ONE IdentificationModule at a time (its key planes,
        workspaces and sample are dropped by that module before it resets); a reset by a second LIVE module while the first still exists would hand the
        first one's planes out again under its feet, so it is refused.  `release_owner()` passes the arena on."""
        if owner is not None:
            cur = self._owner() if self._owner is not None else None
            if cur is not None and cur is not owner:
                raise RuntimeError("6dgs_amd: this arena already serves another IdentificationModule (ops.Arena serves one module at a time: "
                                   "call arena.release_owner() once the first module's scene is done, or give the second module its own arena)")
            import weakref
            self._owner = weakref.ref(owner)
        self.off = 0

    def release_owner(self) -> None:
        self._owner = None


_arena: Optional[Arena] = None
ARENA_MIN_BYTES = 1 << 22          # smaller buffers stay with torch's allocator


def set_arena(arena: Optional[Arena]) -> Optional[Arena]:
    """Install (or, with None, remove) the arena the big buffers come from; returns the previous one."""
    global _arena
    prev, _arena = _arena, arena
    return prev


def get_arena() -> Optional[Arena]:
    return _arena


class arena_scope:
    """`with ops.arena_scope():` -- what is taken from the arena inside is given back at the end (no-op without an arena)."""

    def __enter__(self):
        self.m = _arena.mark() if _arena is not None else None
        return self

    def __exit__(self, *exc):
        if _arena is not None and self.m is not None:
            _arena.release(self.m)
        return False


def big_empty(shape, dtype, device) -> torch.Tensor:
    """torch.empty for the path's big buffers: from the arena when one is installed on this device (and the buffer is big), else from torch."""
    n = 1
    for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(d)
    nbytes = n * torch.empty(0, dtype=dtype).element_size()
    a = _arena
    if a is not None and nbytes >= ARENA_MIN_BYTES and a.buf.device == torch.device(device):
        return a.take(nbytes).view(dtype).view(shape)
    return torch.empty(shape, dtype=dtype, device=device)


def _free_bytes(dev) -> int:
    """Device memory a new tensor can still get: what the driver reports free + what PyTorch's caching allocator holds unused."""
    free = torch.cuda.mem_get_info(dev)[0]
    return int(free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))


def ray_keys_workspace_bytes(r: int, max_chunk: int = RAY_KEYS_CHUNK) -> int:
    """Transient workspace of one ray_keys call over r rays (callers that budget HBM: bench.py's residency guard, the streamed scorer)."""
    return int(_lib.load().sixdgs_ray_keys_workspace_bytes(int(r), int(max_chunk)))


@_on_device
def ray_keys(ori, dr, rgb, weights: PackedWeights, want_feat: bool = False, want_key: bool = True, max_chunk: int = RAY_KEYS_CHUNK,
             workspace: Optional[torch.Tensor] = None, profile: Optional["KernelProfile"] = None, want_planes: bool = False,
             norm_out: Optional[torch.Tensor] = None):
    """-> (feat | None, key | None)  or, with want_planes (F16X3 modes only), (feat | None, key | None, (uint8 [R,1536] scaled fp16 planes,
    inv_scale [ceil(R/128)])).
    norm_out (device scalar [1], scaled fp16 planes only): updated to max(norm_out, max_r |key row|) -- see key_norm_max."""
    ori, dr, rgb = _f32(ori), _f32(dr), _f32(rgb)
    _need_gpu(ori, dr, rgb)
    lib = _lib.load()
    r = ori.shape[0]
    dev = ori.device
    feat = torch.empty(r, D, device=dev) if want_feat else None
    key = torch.empty(r, D, device=dev) if want_key else None
    mode = effective_mma_mode()
    f16 = want_planes and mode in F16_MODES
    if want_planes and not f16:
        raise RuntimeError("6dgs_amd: key planes exist in the fp16 x 3 modes only (MMA_F32 / MMA_BF16X6 score on fp32 keys)")
    planes = big_empty((r, 1536), torch.uint8, dev) if want_planes else None
    inv = torch.empty((r + 127) // 128, device=dev) if f16 else None
    nbytes = lib.sixdgs_ray_keys_workspace_bytes(r, int(max_chunk))
    if workspace is None or workspace.numel() < nbytes:
        # 6560 B of transient workspace per ray of a chunk (6.9 GB at the default 2^20 rays): next to a scene that nearly fills the HBM the
        # chunk shrinks instead of the allocation failing -- any chunking gives the same keys bit for bit, smaller chunks are 3 % slower
        chunk = int(max_chunk)
        room = (_arena.capacity - _arena.off) if (_arena is not None and _arena.buf.device == dev) else 0.5 * _free_bytes(dev)
        while chunk > RAY_KEYS_CHUNK_MIN and nbytes > room:
            chunk //= 2
            nbytes = lib.sixdgs_ray_keys_workspace_bytes(r, chunk)
    if norm_out is not None and not f16:
        raise RuntimeError("6dgs_amd: norm_out needs scaled fp16 key planes (want_planes in MMA_F16X3 mode)")
    with arena_scope():         # the chain's workspace is transient: back to the arena when the call is enqueued (reuse is ordered by the stream)
        ws = workspace if workspace is not None and workspace.numel() >= nbytes else big_empty(nbytes, torch.uint8, dev)
        check(lib.sixdgs_ray_keys_ex(_p(ori), _p(dr), _p(rgb), r, weights.ref, _p(feat), _p(key), _p(planes), _p(inv), _p(norm_out), _p(ws), ws.numel(),
                                     _stream(), profile.ref if profile is not None else None, mode), "ray_keys")
    if want_planes:
        return feat, key, (planes, inv)
    return feat, key


@_on_device
def pad_tokens(token_list, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """list of [T_i, 398] -> tokens [B,256,398] (zero padded), n_tok int32 [B] (device)."""
    b = len(token_list)
    tok = torch.zeros(b, MAX_TOKENS, TOK_IN, device=device)
    n = torch.empty(b, dtype=torch.int32)
    for i, t in enumerate(token_list):
        if t.shape[0] > MAX_TOKENS or t.shape[1] != TOK_IN:
            raise RuntimeError(f"6dgs_amd: token block {tuple(t.shape)} does not fit [<=256, 398]")
        tok[i, : t.shape[0]] = t
        n[i] = t.shape[0]
    return tok, n.to(device)


@_on_device
def q_proj(tokens: torch.Tensor, n_tok: torch.Tensor, weights: PackedWeights) -> torch.Tensor:
    tokens = _f32(tokens)
    _need_gpu(tokens, n_tok)
    b = tokens.shape[0]
    q = torch.empty(b, MAX_TOKENS, D, device=tokens.device)
    check(_lib.load().sixdgs_q_proj(_p(tokens), _p(n_tok), b, weights.ref, _p(q), _stream()), "q_proj")
    return q


def score_topk_workspace_bytes(r: int, batch: int, topk: int = 100, planes: bool = False) -> int:
    """Workspace of the scorer for `batch` resident images.  planes=True: the call will run on pre-split key planes in the
    active MMA mode (24-bit logits in MMA_F16X3: 23 % smaller); False: enough for every mode."""
    if planes:
        return int(_lib.load().sixdgs_score_topk_workspace_bytes_ex(int(r), int(batch), int(topk), effective_mma_mode(), 1))
    return int(_lib.load().sixdgs_score_topk_workspace_bytes(int(r), int(batch), int(topk)))


@_on_device
def score_topk(q: torch.Tensor, n_tok: torch.Tensor, key: Optional[torch.Tensor], topk: int = 100, want_scores: bool = True,
               want_stats: bool = False, workspace: Optional[torch.Tensor] = None, images_in_flight: Optional[int] = None,
               profile: Optional["KernelProfile"] = None, n_tok_host=None, key_planes: Optional[torch.Tensor] = None,
               key_scale: Optional[torch.Tensor] = None):
    """key: fp32 [R,384] and/or key_planes: uint8 [R,1536] scaled fp16 planes + key_scale (the F16X3 modes: the DMA-fed kernels);
    MMA_F32 / MMA_BF16X6 score on the fp32 keys.  q fp32 [B,256,384]: rows at or beyond n_tok[b] are not read in any mode (they may hold
    anything, NaN and Inf included); stats rows there are unspecified.  Returns (idx [B,k], val [B,k], scores [B,R] | None, stats [B,256,2] | None);
    idx / val beyond min(R, k) are (-1, NaN)."""
    q = _f32(q)
    key = _f32(key) if key is not None else None
    _need_gpu(q, key, n_tok, key_planes)
    lib = _lib.load()
    r = key.shape[0] if key is not None else key_planes.shape[0]
    b, dev = q.shape[0], q.device
    idx = torch.empty(b, topk, dtype=torch.int64, device=dev)
    val = torch.empty(b, topk, device=dev)
    scores = torch.empty(b, r, device=dev) if want_scores else None
    stats = torch.empty(b, MAX_TOKENS, 2, device=dev) if want_stats else None
    if workspace is None:
        inflight = b if images_in_flight is None else max(1, min(b, images_in_flight))
        workspace = torch.empty(score_topk_workspace_bytes(r, inflight, topk, planes=key_planes is not None), dtype=torch.uint8, device=dev)
    h_n = None
    if profile is not None and n_tok_host is not None:
        h_n = (C.c_int32 * b)(*[int(v) for v in n_tok_host])
    mode = effective_mma_mode()
    if key_planes is not None and mode in F16_MODES:
        if key_planes.shape[1] != 1536 or key_scale is None:
            raise RuntimeError("6dgs_amd: key planes are not in the format of the active MMA mode (scaled fp16 planes [R,1536] + key_scale)")
    elif key_planes is not None:
        if key is None:
            raise RuntimeError("6dgs_amd: MMA_F32 / MMA_BF16X6 score on fp32 keys: pass `key` (key planes are the operand of the fp16 x 3 kernels only)")
        key_planes = key_scale = None
    check(lib.sixdgs_score_topk_ex(_p(q), _p(n_tok), h_n, b, _p(key), _p(key_planes), _p(key_scale), r, int(topk), _p(scores), _p(idx), _p(val), _p(stats),
                                   _p(workspace), workspace.numel(), _stream(), profile.ref if profile is not None else None,
                                   _mma_mode), "score_topk")
    return idx, val, scores, stats


MAX_TOPK = 1024                  # the largest k any top-k entry point takes (the C checks: topk <= 1024, one workgroup sorts the list)


def check_topk(k, what: str = "rays_to_output") -> int:
    """k as an int in [1, MAX_TOPK], or ValueError -- for callers that must refuse before any GPU work is enqueued."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_TOPK:
        raise ValueError(f"6dgs_amd: {what} = {k!r}: the top-k takes 1 <= k <= MAX_TOPK = {MAX_TOPK}")
    return int(k)


SELECT_MAX_CANDIDATES = 4096     # candidates re-scored exactly per image; an image with more falls back to the two-pass scorer
#                                  (a candidate budget, not a top-k limit: the select path needs room for k of them, k <= MAX_TOPK)
SELECT_SAMPLE_STRIDE = 16       # the pre-pass sees one ray in 16 ...
SELECT_SAMPLE_STRIDE_LARGE = 32  # ... one in 32 from SELECT_LARGE_RAYS rays (the sample is then still >= 0.5 M rays: its row sums are
SELECT_LARGE_RAYS = 16_000_000   # as representative as one in 16 of a scene half the size, and the pre-pass costs half) ...
SELECT_SAMPLE_STRIDE_HUGE = 64   # ... one in 64 from SELECT_HUGE_RAYS rays (>= 0.5 M sample rays again).  The sample only sets the
SELECT_HUGE_RAYS = 32_000_000    # exponent offsets and the width g_min / g_max of the bounds, never the answer
SELECT_MIN_RAYS = 1 << 20        # below this the two-pass scorer is as fast (its logits fit in cache-sized workspaces)
_select_enabled = True


def set_select_enabled(on: bool):
    """Whether top-k-only requests on fp16 key planes may take sixdgs_score_select (no logits through HBM)."""
    global _select_enabled
    _select_enabled = bool(on)


def select_enabled() -> bool:
    return _select_enabled


@_on_device
def select_sample_indices(r: int, device, stride: Optional[int] = None) -> torch.Tensor:
    """One ray of every `stride` consecutive ones (default: 16, 32 from SELECT_LARGE_RAYS rays, 64 from SELECT_HUGE_RAYS), at a position that varies
    pseudo-randomly from group to group (a fixed position would pick the same iso-cell direction of every ellipsoid):
    indices stride*i + (2654435761 i mod 2^32 >> 13) mod stride."""
    if stride is None:
        stride = SELECT_SAMPLE_STRIDE_HUGE if r >= SELECT_HUGE_RAYS else (SELECT_SAMPLE_STRIDE_LARGE if r >= SELECT_LARGE_RAYS else SELECT_SAMPLE_STRIDE)
    n = r // stride
    i = torch.arange(n, dtype=torch.int64, device=device)
    return i * stride + (((i * 2654435761) & 0xFFFFFFFF) >> 13) % stride


@_on_device
def key_norm_max(planes: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max_r |k_r| of the rows of scaled fp16 key planes as a device scalar [1] (rounded up: the select path's error bound is built
    on it, include/sixdgs.h).  `out`: accumulate into an existing scalar (scenes that go through in chunks)."""
    _need_gpu(planes, scale, out)
    if planes.shape[1] != 1536:
        raise RuntimeError("6dgs_amd: key_norm_max needs scaled fp16 key planes (MMA_F16X3)")
    if out is None:
        out = torch.zeros(1, device=planes.device)
    check(_lib.load().sixdgs_key_planes_norm_max(_p(planes), _p(scale), planes.shape[0], _p(out), _stream()), "key_planes_norm_max")
    return out


def score_select_workspace_bytes(r: int, batch: int, topk: int = 100, max_candidates: int = SELECT_MAX_CANDIDATES) -> int:
    return int(_lib.load().sixdgs_score_select_workspace_bytes(int(r), int(batch), int(topk), int(max_candidates)))


def select_sweep_plan(n_tok_host, batch: Optional[int] = None):
    """How the select sweep cuts a batch with these token counts (None: unknown, one image per 256-token tile) into launches:
    -> list of (tiles, images) per launch (include/sixdgs.h: sixdgs_select_sweep_plan; host arithmetic, no GPU needed)."""
    lib = _lib.load()
    b = len(n_tok_host) if n_tok_host is not None else int(batch)
    h_n = (C.c_int32 * b)(*[int(v) for v in n_tok_host]) if n_tok_host is not None else None
    cap = max(1, b)
    slots, imgs = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = lib.sixdgs_select_sweep_plan(h_n, b, slots, imgs, cap)
    if n < 0:
        check(n, "select_sweep_plan")
    return [(int(slots[i]), int(imgs[i])) for i in range(min(n, cap))]


@_on_device
def score_select(q: torch.Tensor, n_tok: torch.Tensor, key_planes: torch.Tensor, key_scale: torch.Tensor, sample_planes: torch.Tensor,
                 sample_scale: torch.Tensor, topk: int = 100, max_candidates: int = SELECT_MAX_CANDIDATES,
                 workspace: Optional[torch.Tensor] = None, profile: Optional["KernelProfile"] = None, n_tok_host=None,
                 key_norm: Optional[torch.Tensor] = None):
    """Top-k without materialised logits (include/sixdgs.h: sixdgs_score_select).  Returns (idx [B,k], val [B,k], status [B] int32 on
    the device: candidates examined, or -1 = this image needs the two-pass scorer).  key_norm: key_norm_max(key_planes, key_scale),
    computed here (one more pass over the planes) when not handed in -- callers with a key cache keep it beside the planes.
    n_tok_host: list of the token counts (must equal n_tok): masked views then share the sweep's 256-token tiles (token packing)."""
    q = _f32(q)
    _need_gpu(q, n_tok, key_planes, key_scale, sample_planes, sample_scale, key_norm)
    if key_norm is None:
        key_norm = key_norm_max(key_planes, key_scale)
    if key_planes.shape[1] != 1536 or sample_planes.shape[1] != 1536:
        raise RuntimeError("6dgs_amd: score_select needs scaled fp16 key planes (MMA_F16X3)")
    lib = _lib.load()
    b, dev, r, rs = q.shape[0], q.device, key_planes.shape[0], sample_planes.shape[0]
    idx = torch.empty(b, topk, dtype=torch.int64, device=dev)
    val = torch.empty(b, topk, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(score_select_workspace_bytes(r, b, topk, max_candidates), dtype=torch.uint8, device=dev)
    # the host copy of the token counts: with it the sweep PACKS the images of a launch by their token counts (round 5; include/sixdgs.h)
    h_n = (C.c_int32 * b)(*[int(v) for v in n_tok_host]) if n_tok_host is not None else None
    check(lib.sixdgs_score_select(_p(q), _p(n_tok), h_n, b, _p(key_planes), _p(key_scale), _p(key_norm), r, _p(sample_planes), _p(sample_scale), rs,
                                  int(topk), int(max_candidates), _p(idx), _p(val), _p(status), _p(workspace), workspace.numel(), _stream(),
                                  profile.ref if profile is not None else None), "score_select")
    return idx, val, status


class SelectStream:
    """The select path stage by stage (include/sixdgs.h: sixdgs_select_begin / _sweep / _candidates / _rescore) for ray sets that
    go through in chunks: begin(sample planes) -> sweep(chunk planes, ray offset) per chunk -> candidates() -> rescore(planes of
    the candidates).  Holds the caller-side buffers: ctok, gsum [B,256], U [B, R rounded up to 256]."""

    @_on_device
    def __init__(self, q: torch.Tensor, n_tok: torch.Tensor, r_total: int, topk: int = 100, max_candidates: int = SELECT_MAX_CANDIDATES,
                 n_tok_host=None):
        self.q, self.n_tok = _f32(q), n_tok
        _need_gpu(self.q, n_tok)
        self.b, self.dev = self.q.shape[0], self.q.device
        self.device = self.dev
        self.r, self.topk, self.cmax = int(r_total), int(topk), int(max_candidates)
        self.stride = (self.r + 255) // 256 * 256
        self.ctok = torch.empty(self.b, MAX_TOKENS, device=self.dev)
        self.gsum = torch.empty(self.b, MAX_TOKENS, device=self.dev)
        self.u = big_empty((self.b, self.stride), torch.float32, self.dev)
        self.utm = torch.empty(self.b, self.stride // 256, device=self.dev)        # the largest U of every 256-ray tile (candidate threshold)
        self.key_norm = torch.zeros(1, device=self.dev)        # max |k_r| over the chunks swept so far (the bound of the candidate stage)
        self.ws = torch.empty(1, dtype=torch.uint8, device=self.dev)
        self.h_n = (C.c_int32 * self.b)(*[int(v) for v in n_tok_host]) if n_tok_host is not None else None

    def _grow(self, need):
        if self.ws.numel() < need:
            self.ws = None
            self.ws = big_empty(need, torch.uint8, self.dev)       # (from an arena: the smaller predecessor stays taken until the caller's scope ends)

    def reserve(self, chunk_rows: int):
        """Grow the stage workspace ONCE to what sweep(chunk of `chunk_rows` rays), candidates() and rescore() will ask for -- callers that take the
        chunks' planes from an arena inside a per-chunk scope must not have the workspace grow (and be given back) inside such a scope."""
        lib = _lib.load()
        self._grow(max(lib.sixdgs_select_workspace_bytes(int(chunk_rows), self.b, self.topk, self.cmax),
                       lib.sixdgs_select_candidates_workspace_bytes(self.r, self.b, self.topk, self.cmax)))

    @_on_device
    def begin(self, sample_planes, sample_scale):
        _need_gpu(self.q, sample_planes, sample_scale)
        lib = _lib.load()
        self._grow(lib.sixdgs_select_workspace_bytes(sample_planes.shape[0], self.b, self.topk, self.cmax))
        check(lib.sixdgs_select_begin(_p(self.q), _p(self.n_tok), self.h_n, self.b, _p(sample_planes), _p(sample_scale), sample_planes.shape[0], self.r,
                                      _p(self.ctok), _p(self.gsum), _p(self.ws), self.ws.numel(), _stream()), "select_begin")

    @_on_device
    def sample_stats(self, sample_planes, sample_scale) -> torch.Tensor:
        """First half of begin(): (max, sumexp) [B,256,2] of the given sample -- ray-sharded scenes merge them across the shards."""
        _need_gpu(self.q, sample_planes, sample_scale)
        lib = _lib.load()
        self._grow(lib.sixdgs_select_workspace_bytes(sample_planes.shape[0], self.b, self.topk, self.cmax))
        stats = torch.empty(self.b, MAX_TOKENS, 2, device=self.dev)
        check(lib.sixdgs_select_sample_stats(_p(self.q), _p(self.n_tok), self.h_n, self.b, _p(sample_planes), _p(sample_scale), sample_planes.shape[0],
                                             _p(stats), _p(self.ws), self.ws.numel(), _stream()), "select_sample_stats")
        return stats

    @_on_device
    def prepare(self, stats: torch.Tensor, r_sample_total: int, r_total: int):
        """Second half of begin(): the (merged) sample statistics and the TOTAL sample / ray counts of the scene -> ctok; gsum = 0."""
        stats = _f32(stats)
        _need_gpu(self.q, stats)
        check(_lib.load().sixdgs_select_prepare(_p(stats), _p(self.n_tok), self.b, int(r_sample_total), int(r_total), _p(self.ctok), _p(self.gsum),
                                                _stream()), "select_prepare")

    @_on_device
    def topk_u(self, exact: bool = False) -> torch.Tensor:
        """The k largest TILE MAXIMA of U over the rays swept so far, per image, descending (the k largest U themselves for scenes of fewer than
        2 k tiles): the k-th of them is a lower bound of the k-th largest U, which is what the candidate threshold needs.  exact=True: the
        k largest U themselves (six passes over U instead of one over the tile maxima) -- the bound that does not degrade when the top
        rays sit in a few tiles."""
        lib = _lib.load()
        _need_gpu(self.q)
        self._grow(lib.sixdgs_select_candidates_workspace_bytes(self.r, self.b, self.topk, self.cmax))
        val = torch.empty(self.b, self.topk, device=self.dev)
        check(lib.sixdgs_select_topk_u(_p(self.u), self.stride, self.r, None if exact else _p(self.utm), self.b, self.topk, _p(val), _p(self.ws),
                                       self.ws.numel(), _stream()),
              "select_topk_u")
        return val

    @_on_device
    def sweep(self, planes, scale, ray_offset: int, profile: Optional["KernelProfile"] = None, update_norm: bool = True):
        """update_norm=False: the caller already folded these planes' largest key norm into self.key_norm (ray_keys(norm_out=...))."""
        if ray_offset % 256:
            raise RuntimeError("6dgs_amd: select sweep chunks must start at a multiple of 256 rays")
        _need_gpu(self.q, planes, scale)
        lib = _lib.load()
        rc = planes.shape[0]
        self._grow(lib.sixdgs_select_workspace_bytes(rc, self.b, self.topk, self.cmax))
        check(lib.sixdgs_select_sweep(_p(self.q), _p(self.n_tok), self.h_n, self.b, _p(planes), _p(scale), rc,
                                      _p(self.ctok), _p(self.gsum), C.c_void_p(self.u.data_ptr() + 4 * int(ray_offset)), self.stride,
                                      C.c_void_p(self.utm.data_ptr() + 4 * (int(ray_offset) // 256)),
                                      _p(self.ws), self.ws.numel(), _stream(), profile.ref if profile is not None else None), "select_sweep")
        if update_norm:
            key_norm_max(planes, scale, out=self.key_norm)

    @_on_device
    def candidates(self, uk: Optional[torch.Tensor] = None):
        """-> (cand [B,cmax] int64 ascending ray indices, count [B] int32 on the device).  uk [B]: the k-th largest U of the WHOLE
        scene (ray-sharded callers, from the merged topk_u lists); default: of this object's rays."""
        lib = _lib.load()
        _need_gpu(self.q)
        self._grow(lib.sixdgs_select_candidates_workspace_bytes(self.r, self.b, self.topk, self.cmax))
        cand = torch.zeros(self.b, self.cmax, dtype=torch.int64, device=self.dev)
        count = torch.empty(self.b, dtype=torch.int32, device=self.dev)
        uk = _f32(uk) if uk is not None else None
        check(lib.sixdgs_select_candidates(_p(self.u), self.stride, self.r, _p(self.utm), _p(self.q), _p(self.n_tok), self.b, _p(self.gsum), _p(self.key_norm),
                                           _p(uk), self.topk, self.cmax, _p(cand), _p(count), _p(self.ws), self.ws.numel(), _stream()), "select_candidates")
        return cand, count

    @_on_device
    def rescore(self, planes, scale, cand, count, compact: bool, allow_fewer: bool = False):
        """-> (idx [B,k], val [B,k], status [B] int32).  allow_fewer: fewer than k candidates is an answer (-1 / NaN padded), not a
        refusal -- a shard of a ray-sharded scene."""
        lib = _lib.load()
        _need_gpu(self.q, planes, scale, cand, count)
        idx = torch.empty(self.b, self.topk, dtype=torch.int64, device=self.dev)
        val = torch.empty(self.b, self.topk, device=self.dev)
        status = torch.empty(self.b, dtype=torch.int32, device=self.dev)
        self._grow(lib.sixdgs_select_candidates_workspace_bytes(self.r, self.b, self.topk, self.cmax))
        check(lib.sixdgs_select_rescore(_p(self.q), _p(self.n_tok), self.b, _p(planes), _p(scale), 1 if compact else 0, _p(self.ctok),
                                        _p(self.gsum), _p(cand), _p(count), self.r, self.topk, self.cmax, 1 if allow_fewer else 0, _p(idx), _p(val), _p(status),
                                        _p(self.ws), self.ws.numel(), _stream()), "select_rescore")
        return idx, val, status


@_on_device
def score_pass1(q: torch.Tensor, n_tok: torch.Tensor, key: Optional[torch.Tensor], workspace: torch.Tensor, topk: int = 100,
                key_planes: Optional[torch.Tensor] = None, key_scale: Optional[torch.Tensor] = None,
                profile: Optional["KernelProfile"] = None, n_tok_host=None) -> torch.Tensor:
    """First half of the ray-sharded scorer (include/sixdgs.h: sixdgs_score_pass1): logits of this shard for all images
    stay in `workspace` (score_topk_workspace_bytes(r, batch, topk) bytes); returns the shard's row statistics [B,256,2]."""
    q = _f32(q)
    key = _f32(key) if key is not None else None
    _need_gpu(q, key, n_tok, key_planes, workspace)
    r = key.shape[0] if key is not None else key_planes.shape[0]
    b = q.shape[0]
    stats = torch.empty(b, MAX_TOKENS, 2, device=q.device)
    h_n = (C.c_int32 * b)(*[int(v) for v in n_tok_host]) if (profile is not None and n_tok_host is not None) else None
    check(_lib.load().sixdgs_score_pass1(_p(q), _p(n_tok), h_n, b, _p(key), _p(key_planes), _p(key_scale), r, int(topk), _p(stats),
                                         _p(workspace), workspace.numel(), _stream(), profile.ref if profile is not None else None,
                                         _mma_mode), "score_pass1")
    return stats


@_on_device
def score_pass2(stats: torch.Tensor, n_tok: torch.Tensor, r: int, workspace: torch.Tensor, topk: int = 100, used_planes: bool = True,
                want_scores: bool = True):
    """Second half: global row statistics [B,256,2] -> (local idx [B,k], val [B,k], scores [B,r] | None) of this shard."""
    stats = _f32(stats)
    _need_gpu(stats, n_tok, workspace)
    b, dev = stats.shape[0], stats.device
    idx = torch.empty(b, topk, dtype=torch.int64, device=dev)
    val = torch.empty(b, topk, device=dev)
    scores = torch.empty(b, r, device=dev) if want_scores else None
    check(_lib.load().sixdgs_score_pass2(_p(stats), _p(n_tok), b, 1 if used_planes else 0, int(r), int(topk), _p(scores), _p(idx), _p(val),
                                         _p(workspace), workspace.numel(), _stream(), _mma_mode), "score_pass2")
    return idx, val, scores


def _check_scorer_operands(q: torch.Tensor, n_tok: torch.Tensor, k: torch.Tensor):
    """The operand contract of ray_attention_scores / score_backward: fp32 q [B,256,384] and key [R,384], int32 n_tok [B], contiguous, on one GPU."""
    _need_gpu(q, n_tok, k)
    if q.dtype != torch.float32 or k.dtype != torch.float32:
        raise RuntimeError(f"6dgs_amd: q and k must be float32 (got {q.dtype}, {k.dtype})")
    if q.dim() != 3 or tuple(q.shape[1:]) != (MAX_TOKENS, D):
        raise RuntimeError(f"6dgs_amd: q must be [B,{MAX_TOKENS},{D}] (got {tuple(q.shape)})")
    if k.dim() != 2 or k.shape[1] != D or k.shape[0] < 1:
        raise RuntimeError(f"6dgs_amd: k must be [R,{D}] with R >= 1 (got {tuple(k.shape)})")
    if n_tok.dtype != torch.int32 or tuple(n_tok.shape) != (q.shape[0],):
        raise RuntimeError(f"6dgs_amd: n_tok must be int32 [{q.shape[0]}] (got {n_tok.dtype} {tuple(n_tok.shape)})")
    if not (q.is_contiguous() and k.is_contiguous() and n_tok.is_contiguous()):
        raise RuntimeError("6dgs_amd: q, n_tok and k must be contiguous")


@_on_device
def score_backward(q: torch.Tensor, n_tok: torch.Tensor, k: torch.Tensor, row_stats: torch.Tensor, g: torch.Tensor, ray_groups: int = 1):
    """include/sixdgs.h: sixdgs_score_backward.  (dq [B,256,384], dk [R,384]) of scores[b][r] = sum_t softmax_r(q[b][t] . k[r] / sqrt(384))
    for the upstream gradient g [B,R], from the forward's row statistics [B,256,2]; dq rows at or beyond n_tok[b] are zeros.
    ray_groups: 1 (default) = sixdgs_score_backward; G > 1 splits each token tile's rays into G groups (sixdgs_score_backward_split: 2 x B x G
    workgroups instead of 2 x B, partial sums reduced in a fixed order, other rounding than G = 1); 0 = G chosen from the CU count, B and R."""
    ray_groups = int(ray_groups)
    if ray_groups < 0:
        raise ValueError(f"6dgs_amd: ray_groups must be >= 0 (got {ray_groups})")
    _check_scorer_operands(q, n_tok, k)
    b, r = q.shape[0], k.shape[0]
    if tuple(row_stats.shape) != (b, MAX_TOKENS, 2) or tuple(g.shape) != (b, r):
        raise RuntimeError(f"6dgs_amd: row_stats must be [{b},{MAX_TOKENS},2] and g [{b},{r}] (got {tuple(row_stats.shape)}, {tuple(g.shape)})")
    row_stats, g = _f32(row_stats), _f32(g)
    _need_gpu(row_stats, g)
    lib = _lib.load()
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    if ray_groups == 1:
        ws = torch.empty(max(1, lib.sixdgs_score_backward_workspace_bytes(b)), dtype=torch.uint8, device=q.device)
        check(lib.sixdgs_score_backward(_p(q), _p(n_tok), b, _p(k), r, _p(row_stats), _p(g), _p(dq), _p(dk), _p(ws), ws.numel(), _stream()),
              "score_backward")
    else:
        ws = torch.empty(max(1, lib.sixdgs_score_backward_split_workspace_bytes(b, r, ray_groups)), dtype=torch.uint8, device=q.device)
        check(lib.sixdgs_score_backward_split(_p(q), _p(n_tok), b, _p(k), r, _p(row_stats), _p(g), _p(dq), _p(dk), ray_groups, _p(ws), ws.numel(),
                                              _stream()), "score_backward_split")
    return dq, dk


@_on_device
def _ray_attention_forward(q: torch.Tensor, n_tok: torch.Tensor, k: torch.Tensor):
    """(scores [B,R], row statistics [B,256,2]) of the two-pass scorer, on the key's scaled fp16 planes in the F16X3 modes."""
    _check_scorer_operands(q, n_tok, k)
    b, r = q.shape[0], k.shape[0]
    planes = effective_mma_mode() in F16_MODES
    kp, ks = split_planes_f16(k) if planes else (None, None)
    ws = torch.empty(score_topk_workspace_bytes(r, b, 1, planes=planes), dtype=torch.uint8, device=q.device)
    stats = score_pass1(q, n_tok, k, ws, 1, key_planes=kp, key_scale=ks)
    _, _, scores = score_pass2(stats, n_tok, r, ws, 1, used_planes=planes)
    return scores, stats


class RayAttentionScores(torch.autograd.Function):
    """scores [B,R] = sum_t softmax_r(q[b][t] . k[r] / sqrt(384)) over the first n_tok[b] tokens.  Forward: the two-pass scorer
    (score_pass1 on the key's scaled fp16 planes, score_pass2); backward: sixdgs_score_backward from the saved row statistics (split over
    ray_groups groups of rays when ray_groups != 1: score_backward)."""

    @staticmethod
    def forward(ctx, q, n_tok, k, ray_groups=1):
        q, k = q.detach(), k.detach()
        scores, stats = _ray_attention_forward(q, n_tok, k)
        ctx.save_for_backward(q, n_tok, k, stats)
        ctx.ray_groups = ray_groups
        return scores

    @staticmethod
    def backward(ctx, g):
        q, n_tok, k, stats = ctx.saved_tensors
        dq, dk = score_backward(q, n_tok, k, stats, g.contiguous(), ray_groups=ctx.ray_groups)
        return dq if ctx.needs_input_grad[0] else None, None, dk if ctx.needs_input_grad[2] else None, None


def ray_attention_scores(q: torch.Tensor, n_tok: torch.Tensor, k: torch.Tensor, ray_groups: int = 1) -> torch.Tensor:
    """Differentiable scorer of training: q fp32 [B,256,384] (rows at or beyond n_tok[b] are ignored), n_tok int32 [B] on the device,
    k fp32 [R,384] -> scores [B,R]; gradients reach q and k (RayAttentionScores).  ray_groups: the backward's split over the rays
    (score_backward; 1 = the unsplit kernels, 0 = auto)."""
    if int(ray_groups) < 0:
        raise ValueError(f"6dgs_amd: ray_groups must be >= 0 (got {ray_groups})")
    return RayAttentionScores.apply(q, n_tok, k, int(ray_groups))


@_on_device
def topk(scores: torch.Tensor, k: int = 100):
    scores = _f32(scores)
    _need_gpu(scores)
    lib = _lib.load()
    s2 = scores.reshape(-1, scores.shape[-1])
    b, r = s2.shape
    idx = torch.empty(b, k, dtype=torch.int64, device=s2.device)
    val = torch.empty(b, k, device=s2.device)
    ws = torch.empty(lib.sixdgs_topk_workspace_bytes(r, b, k), dtype=torch.uint8, device=s2.device)
    check(lib.sixdgs_topk(_p(s2), r, b, int(k), _p(idx), _p(val), _p(ws), ws.numel(), _stream()), "topk")
    return idx.reshape(*scores.shape[:-1], k), val.reshape(*scores.shape[:-1], k)


# ---------------------------------------------------------------------------------------------
# DistanceBasedScoreLoss target scores
# ---------------------------------------------------------------------------------------------
@_on_device
def distance_target(rays_ori, rays_dir, pose, n_tokens: int, want_sum: bool = False):
    """Target scores [R] of distance_based_loss.py for the ground-truth c2w `pose` [4,4] (any device), summing to n_tokens."""
    rays_ori, rays_dir = _f32(rays_ori), _f32(rays_dir)
    _need_gpu(rays_ori, rays_dir)
    lib = _lib.load()
    r, dev = rays_ori.shape[0], rays_ori.device
    pose = _f32(pose.to(dev)).reshape(16)
    target = torch.empty(r, device=dev)
    tot = torch.zeros(1, device=dev) if want_sum else None
    ws = torch.empty(lib.sixdgs_distance_target_workspace_bytes(r), dtype=torch.uint8, device=dev)
    check(lib.sixdgs_distance_target(_p(rays_ori), _p(rays_dir), r, _p(pose), int(n_tokens), _p(target), _p(tot), _p(ws), ws.numel(),
                                     _stream()), "distance_target")
    return (target, tot) if want_sum else target


# ---------------------------------------------------------------------------------------------
# pose
# ---------------------------------------------------------------------------------------------
SOLVE_POSE_MAX_K = 256        # kMaxK of csrc/pose.hip
CONSENSUS_MAX_K = 1024        # kConsMaxK of csrc/pose_consensus.hip
POSE_PRIORS = {"uniform": 0, "score": 1}


@_on_device
def solve_pose(rays_ori, rays_dir, idx, val, up, gt_c2w=None):
    """Batched pose tail.  idx/val [B,k], up [B,3], gt_c2w [B,4,4] or None.
    Returns dict(c2w[B,4,4], status[B], w_final[B,k], n_kept[B], centre[B,3], errors[B,2]).
    k <= SOLVE_POSE_MAX_K (256: the kernel's per-image arrays); a longer top-k raises ValueError -- `solve_pose_consensus` takes up to 1024.
    Entries with idx < 0 or idx >= R are padding at any position: they are skipped, and w_final is 0 there."""
    if idx.dim() == 2 and idx.shape[1] > SOLVE_POSE_MAX_K:
        k = idx.shape[1]
        raise ValueError(f"6dgs_amd: solve_pose takes a top-k of at most {SOLVE_POSE_MAX_K} rays (got {k}); solve_pose_consensus takes up to "
                         f"{CONSENSUS_MAX_K}")
    rays_ori, rays_dir, val, up = _f32(rays_ori), _f32(rays_dir), _f32(val), _f32(up)
    idx = _i64(idx)
    _need_gpu(rays_ori, rays_dir, idx, val, up)
    b, k = idx.shape
    dev = idx.device
    gt = _f32(gt_c2w) if gt_c2w is not None else None
    c2w = torch.empty(b, 4, 4, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    wf = torch.empty(b, k, device=dev)
    nk = torch.empty(b, dtype=torch.int32, device=dev)
    ctr = torch.empty(b, 3, device=dev)
    err = torch.empty(b, 2, device=dev)
    check(_lib.load().sixdgs_solve_pose(_p(rays_ori), _p(rays_dir), rays_ori.shape[0], _p(idx), _p(val), k, _p(up), _p(gt), b,
                                        _p(c2w), _p(status), _p(wf), _p(nk), _p(ctr), _p(err), _stream()), "solve_pose")
    return dict(c2w=c2w, status=status, w_final=wf, n_kept=nk, centre=ctr, errors=err)


def _check_pose_operands(rays_ori, rays_dir, idx, val, up, gt_c2w):
    """Shapes, dtypes and devices of the pose solvers' operands, before anything is marshalled: no wrong-sized tensor reaches a kernel."""
    for name, t in (("rays_ori", rays_ori), ("rays_dir", rays_dir), ("idx", idx), ("val", val), ("up", up)):
        if not torch.is_tensor(t):
            raise TypeError(f"6dgs_amd: {name} must be a tensor (got {type(t).__name__})")
    if rays_ori.dim() != 2 or rays_ori.shape[1] != 3 or rays_dir.shape != rays_ori.shape:
        raise ValueError(f"6dgs_amd: rays_ori and rays_dir must both be [R,3] (got {tuple(rays_ori.shape)} and {tuple(rays_dir.shape)})")
    if idx.dim() != 2 or val.shape != idx.shape:
        raise ValueError(f"6dgs_amd: idx and val must both be [B,k] (got {tuple(idx.shape)} and {tuple(val.shape)})")
    if idx.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"6dgs_amd: idx must be an integer tensor (got {idx.dtype})")
    for name, t in (("rays_ori", rays_ori), ("rays_dir", rays_dir), ("val", val), ("up", up)):
        if not t.is_floating_point():
            raise TypeError(f"6dgs_amd: {name} must be a floating-point tensor (got {t.dtype})")
    b = idx.shape[0]
    if tuple(up.shape) != (b, 3):
        raise ValueError(f"6dgs_amd: up must be [B,3] = [{b},3] (got {tuple(up.shape)})")
    if gt_c2w is not None:
        if not torch.is_tensor(gt_c2w) or not gt_c2w.is_floating_point():
            raise TypeError("6dgs_amd: gt_c2w must be a floating-point tensor or None")
        if tuple(gt_c2w.shape) != (b, 4, 4):
            raise ValueError(f"6dgs_amd: gt_c2w must be [B,4,4] = [{b},4,4] (got {tuple(gt_c2w.shape)})")


@_on_device
def solve_pose_consensus(rays_ori, rays_dir, idx, val, up, gt_c2w=None, *, inlier_scale, prior="uniform"):
    """Batched consensus pose solver (include/sixdgs.h: sixdgs_solve_pose_consensus): every pair of the top-k rays proposes a camera
    centre, all rays vote, the best supported proposal is refined and the pose assembled as by `solve_pose`.  Tolerates a top-k in
    which most rays do not see the camera.  idx/val [B,k] with 2 <= k <= 1024, up [B,3], gt_c2w [B,4,4] or None; `inlier_scale`
    (tau > 0, scene units) is the residual at which a ray's vote has fallen to one half; prior "uniform" or "score" (votes weighted
    by val).  Returns the dict of `solve_pose` (status bit 3: no valid hypothesis, least-squares answer returned; n_kept = valid
    rays) plus support [B] (soft inlier share at the final centre, in [0,1]), n_inliers [B] (int32), rms [B], winner [B,2] (int32)."""
    _check_pose_operands(rays_ori, rays_dir, idx, val, up, gt_c2w)
    if prior not in POSE_PRIORS:
        raise ValueError(f"6dgs_amd: prior must be one of {sorted(POSE_PRIORS)} (got {prior!r})")
    tau = float(inlier_scale)
    if not (tau > 0.0 and tau < float("inf")):
        raise ValueError(f"6dgs_amd: inlier_scale must be a positive finite number (got {inlier_scale})")
    b, k = idx.shape
    if not 2 <= k <= CONSENSUS_MAX_K:
        raise ValueError(f"6dgs_amd: solve_pose_consensus takes a top-k of 2..{CONSENSUS_MAX_K} rays (got {k})")
    rays_ori, rays_dir, val, up = _f32(rays_ori), _f32(rays_dir), _f32(val), _f32(up)
    idx = _i64(idx)
    gt = _f32(gt_c2w) if gt_c2w is not None else None
    _need_gpu(rays_ori, rays_dir, idx, val, up, gt)
    dev = idx.device
    lib = _lib.load()
    c2w = torch.empty(b, 4, 4, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    wf = torch.empty(b, k, device=dev)
    nk = torch.empty(b, dtype=torch.int32, device=dev)
    ctr = torch.empty(b, 3, device=dev)
    err = torch.empty(b, 2, device=dev)
    sup = torch.empty(b, device=dev)
    nin = torch.empty(b, dtype=torch.int32, device=dev)
    rms = torch.empty(b, device=dev)
    win = torch.empty(b, 2, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.sixdgs_solve_pose_consensus_workspace_bytes(b, k)), 256), dtype=torch.uint8, device=dev)
    check(lib.sixdgs_solve_pose_consensus(_p(rays_ori), _p(rays_dir), rays_ori.shape[0], _p(idx), _p(val), k, _p(up), _p(gt), b, tau,
                                          POSE_PRIORS[prior], _p(c2w), _p(status), _p(wf), _p(nk), _p(ctr), _p(err), _p(sup), _p(nin),
                                          _p(rms), _p(win), _p(ws), ws.numel(), _stream()), "solve_pose_consensus")
    return dict(c2w=c2w, status=status, w_final=wf, n_kept=nk, centre=ctr, errors=err, support=sup, n_inliers=nin, rms=rms, winner=win)
