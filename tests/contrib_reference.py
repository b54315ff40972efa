"""Restatement in plain numpy of what sixdgs_raster_contrib defines (include/sixdgs.h), on tests/raster_reference.py's project, _instances
and _alpha: per view and Gaussian the sum and the maximum of w = alpha T over the pixels that ADD the Gaussian, the number of those
pixels, and the number of pixels the Gaussian STOPS; then the accumulation over the views.

It is parametrised by dtype like raster_reference: float64 is the reference; float32 is the same operations in the same order, every
intermediate rounded to fp32 -- including the summation tree of the definition (a tile's 256 pixels in 4 groups of 64 in rows-of-16
order, within a group x += x_(l xor s) for s = 32 .. 1, then the groups in order, then the tiles in rectangle order from 0) and the
chain over the views.  raster_reference's flags travel along: `undecidable` [V,H,W] marks the pixels at which a discrete decision lies
within its band of a threshold, `decidable` [V,n] the Gaussians whose own decisions (cull, radius, rectangle) do not.  Counts can be
compared for equality only where there is no undecidable pixel and every Gaussian is decidable.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as RR  # noqa: E402

TILE = RR.TILE
XOR_STEPS = (32, 16, 8, 4, 2, 1)
_LANE = np.arange(64)


def tile_tree(w):
    """w [G,256] (a tile's pixels in rows-of-16 order, zeros where a pixel does not add the Gaussian), any float dtype -> [G]: the
    definition's tree, every sum in w's dtype."""
    x = w.reshape(w.shape[0], 4, 64)
    for s in XOR_STEPS:
        x = x + x[:, :, _LANE ^ s]
    g = x[:, :, 0]
    return ((g[:, 0] + g[:, 1]) + g[:, 2]) + g[:, 3]


def _walk_tile(P, g, xs, ys, dt):
    """Step 11 for the pixels (xs, ys) of one tile over its Gaussians g in blending order -> (w [G,P], adds [G,P], stops [G,P]): w =
    alpha T with T the value before the Gaussian, where the pixel adds it (0 elsewhere); the one Gaussian per pixel that stops it."""
    thr = dt(1.0 / 255.0)
    power, alpha = RR._alpha(P, g, xs, ys, dt)
    valid = (power <= 0) & (alpha >= thr)
    a = np.where(valid, alpha, dt(0))
    tall = np.cumprod(np.concatenate([np.ones((1, xs.shape[0]), dt), dt(1) - a], axis=0), axis=0, dtype=dt)      # sequential products
    tb, tn = tall[:-1], tall[1:]
    stop_any = valid & (tn < dt(1e-4))
    before = (np.cumsum(stop_any, axis=0) - stop_any) == 0          # no stop in front of it: the walk gets to it
    stops = stop_any & before
    adds = valid & before & ~stop_any
    return np.where(adds, a * tb, dt(0)).astype(dt), adds, stops


def contrib_view(scene, row, width, height, dtype=np.float64, scale_modifier=1.0):
    """One view -> dict over the n Gaussians: weight, peak (dtype), pixels, stops (int64); pixel_sum [H,W] (dtype, the plain sum of w
    over the Gaussians a pixel added, in blending order) and pixel_adds [H,W] (how many those are); image_alpha [H,W], undecidable [H,W], decidable [n] from raster_reference."""
    dt = np.dtype(dtype).type
    ref = RR.reference_view(scene, row, width, height, dt, scale_modifier)
    P = RR.project(scene, row, width, height, dt, scale_modifier)
    n, gx, gy = P["n"], P["gx"], P["gy"]
    live = np.nonzero(P["live"])[0]
    tile, gid = RR._instances(P["rect"], live, gx)
    order = np.lexsort((gid, P["z"][gid], tile))
    tile_s, gid_s = tile[order], gid[order]
    weight, peak = np.zeros(n, dt), np.zeros(n, dt)
    pixels, stops = np.zeros(n, np.int64), np.zeros(n, np.int64)
    pixel_sum, pixel_adds = np.zeros((height, width), dt), np.zeros((height, width), np.int64)
    todo = np.arange(gx * gy)
    starts, ends = np.searchsorted(tile_s, todo, "left"), np.searchsorted(tile_s, todo, "right")
    for t, s0, s1 in zip(todo, starts, ends):          # ascending tile number: every Gaussian meets its tiles in rectangle order
        if s1 == s0:
            continue
        ty, tx = divmod(int(t), gx)
        ys, xs = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, height)), np.arange(tx * TILE, min((tx + 1) * TILE, width)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        g = gid_s[s0:s1]
        w, adds, stp = _walk_tile(P, g, xs, ys, dt)
        full = np.zeros((g.shape[0], TILE * TILE), dt)          # pixels outside the image count as 0
        full[:, (ys - ty * TILE) * TILE + (xs - tx * TILE)] = w
        weight[g] = weight[g] + (tile_tree(full) if dt is np.float32 else full.sum(axis=1))
        peak[g] = np.maximum(peak[g], w.max(axis=1))
        pixels[g] += adds.sum(axis=1)
        stops[g] += stp.sum(axis=1)
        pixel_sum[ys, xs] = np.cumsum(w, axis=0, dtype=dt)[-1]
        pixel_adds[ys, xs] = adds.sum(axis=0)
    return {"weight": weight, "peak": peak, "pixels": pixels, "stops": stops, "pixel_sum": pixel_sum, "pixel_adds": pixel_adds,
            "image_alpha": ref["image"][..., 3],
            "undecidable": ref["undecidable"], "decidable": ref["decidable"]}


def contrib_views(scene, rows, width, height, dtype=np.float64, **kw):
    """All views -> dict: the per-view arrays view_weight, view_peak [V,n] (dtype), view_pixels, view_stops [V,n] (int64), the
    accumulated weight ((0 + v0) + v1 ..., in dtype), peak, pixels, stops, seen [n] and inert [n]; pixel_sum, pixel_adds, image_alpha, undecidable
    [V,H,W]; decidable [V,n]."""
    dt = np.dtype(dtype).type
    per = [contrib_view(scene, row, width, height, dtype, **kw) for row in rows]
    out = {"view_" + k: np.stack([p[k] for p in per]) for k in ("weight", "peak", "pixels", "stops")}
    out.update({k: np.stack([p[k] for p in per]) for k in ("pixel_sum", "pixel_adds", "image_alpha", "undecidable", "decidable")})
    weight = np.zeros(out["view_weight"].shape[1], dt)
    for p in per:
        weight = weight + p["weight"]
    out.update(weight=weight, peak=out["view_peak"].max(axis=0), pixels=out["view_pixels"].sum(axis=0), stops=out["view_stops"].sum(axis=0),
               seen=(out["view_pixels"] > 0).sum(axis=0))
    out["inert"] = (out["pixels"] == 0) & (out["stops"] == 0)
    return out


_cache = {}


def case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree=3):
    """The scene, the camera rows and both restatements of one case, computed once per session and shared (read-only)."""
    key = (n, scene_seed, views, cam_seed, width, height, sh_degree)
    if key not in _cache:
        scene = syn.make_scene(n, scene_seed, sh_degree=sh_degree)
        rows = RR.camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height))
        _cache[key] = pair(scene, rows, width, height)
    return _cache[key]


def pair(scene, rows, width, height):
    """Both restatements of a scene's views, read-only, with the flags joined and the fp32 form's deviation from fp64."""
    r64 = contrib_views(scene, rows, width, height, np.float64)
    r32 = contrib_views(scene, rows, width, height, np.float32)
    out = {"scene": scene, "rows": rows, "r64": r64, "r32": r32, "undecidable": r64["undecidable"] | r32["undecidable"],
           "decidable": r64["decidable"] & r32["decidable"],
           "rounding": max(deviation(r32[k], r64[k]) for k in ("weight", "peak", "view_weight", "view_peak"))}
    for a in (out["undecidable"], out["decidable"], *r64.values(), *r32.values()):
        a.setflags(write=False)
    return out


def deviation(got, r64):
    """max |got - r64| / max(1, r64): the measure of the tests' bound."""
    r64 = np.asarray(r64, np.float64)
    return float((np.abs(np.asarray(got).astype(np.float64) - r64) / np.maximum(1.0, r64)).max()) if r64.size else 0.0


def bound(rounding):
    """raster_reference.bound's rule: 4 x the fp32 restatement's own deviation, never below its floor; a case whose bound passes
    raster_reference.ERROR_CEILING is not a fit case."""
    return RR.bound(rounding)


C0 = 0.28209479177387814
ROW = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 16.0, 16.0]], np.float32)       # identity pose, f = 20, 32 x 32
ROW_LONG = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 12.0, 8.0]], np.float32)   # the same at 24 x 16


def hand(xyz, sigma, o, colour=None):
    """A scene of isotropic-or-not Gaussians with given opacities (values in (0, 1)) and flat colours (SH degree 0), as
    tests/test_gpu_raster.py makes its hand cases."""
    n = len(xyz)
    sigma = np.asarray(sigma, np.float64)
    sigma = np.broadcast_to(sigma.reshape(n, 1) if sigma.ndim == 1 else sigma, (n, 3))
    o = np.asarray(o, np.float64).reshape(n, 1)
    colour = np.full((n, 3), 0.5) if colour is None else np.asarray(colour, np.float64)
    return {"xyz": np.asarray(xyz, np.float32).reshape(n, 3), "log_scale": np.log(sigma).astype(np.float32),
            "rot": np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (n, 1)), "opacity": np.log(o / (1 - o)).astype(np.float32),
            "f_dc": ((colour.reshape(n, 1, 3) - 0.5) / C0).astype(np.float32), "f_rest": np.zeros((n, 0, 3), np.float32), "sh_degree": 0}


def hand_one():
    """One isotropic Gaussian in front of the camera."""
    return hand([[0, 0, 2.0]], 0.2, [0.6])


def hand_saturation():
    """tests/test_gpu_raster.py's saturation case: three near-opaque Gaussians in a row and one behind.  On the middle pixels the third
    takes T below 1e-4 -- it stops them and is not added -- and the fourth is never reached."""
    return hand([[0, 0, 2.0], [0, 0, 2.1], [0, 0, 2.2], [0, 0, 2.3]], 5.0, [0.98] * 4)


def hand_nothing():
    """Behind the near plane (three ways), off-frame with an empty rectangle (two ways), and o < 1/255: none touches a pixel."""
    return hand([[0, 0, 0.19], [0, 0, 0.1], [0, 0, -1.0], [-12.0, 0, 2.0], [0, 30.0, 2.0], [0, 0, 2.0]], [0.05] * 5 + [0.2], [0.9] * 5 + [0.0035])


def hand_corner():
    """Centred on the image corner (u, v) = (0, 0): three quarters of its footprint are outside the image."""
    return hand([[-1.6, -1.6, 2.0]], 0.2, [0.6])


LONG_N, LONG_ADDS = 700, 302


def hand_long(sigma=77.77):
    """700 copies of one Gaussian, wide enough to be flat over a 24 x 16 image, o = 0.03: a list of three rounds.  Every pixel adds
    exactly the first 302 -- T falls below 1e-4 at the 303rd, which stops it --, so index k < 302 has weight a (1 - a)^k per pixel."""
    return hand([[1.4, 0, 2.0]] * LONG_N, sigma, [0.03] * LONG_N)


# (Gaussians, scene seed, views, camera seed, width, height, SH degree): no undecidable pixel in either restatement, every Gaussian decidable
CASES = ((300, 8, 3, 9, 40, 24, 0), (300, 8, 3, 9, 40, 24, 3), (400, 4, 2, 5, 33, 17, 3))
