"""Restatement in plain numpy of what sixdgs_raster_depth defines (include/sixdgs.h), on tests/raster_reference.py's project, _instances
and _alpha: per view and pixel the blend's depth channel D = sum (z alpha) T over the Gaussians the pixel ADDS, the depth and the index
of the first of them behind which T is below 0.5, 1 - T of the end of the walk, and the world point of the pixel's ray at either depth.

It is parametrised by dtype like raster_reference: float64 is the reference; float32 is the same operations in the same order, every
intermediate rounded to fp32 -- the products (z alpha) T, the running sum in blending order, the division expected / alpha and the
lift r, q = d r - t, X = W^T q with its dot products as (a + b) + c.  z is the p.z of the restatement's own precision: in fp32 the float
whose bits the rasteriser stores and sorts by.  `median_undecidable` [H,W] marks the pixels where some added Gaussian's T' lies within
MEDIAN_BAND of 0.5, so that rounding may legitimately hand the median to a neighbour; it joins raster_reference's `undecidable`.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrib_reference as CR  # noqa: E402
import raster_reference as RR  # noqa: E402

TILE = RR.TILE
MEDIAN_BAND = 1e-5
KINDS = ("median", "expected")


def _walk_tile(P, g, xs, ys, dt):
    """Step 11 for the pixels (xs, ys) of one tile over its Gaussians g in blending order, as contrib_reference._walk_tile takes it ->
    (expected, median, median_index, median_pos, alpha, near) per pixel; median_pos is the median's position in g (-1: none)."""
    thr = dt(1.0 / 255.0)
    ar = np.arange(xs.shape[0])
    power, alpha = RR._alpha(P, g, xs, ys, dt)
    valid = (power <= 0) & (alpha >= thr)
    a = np.where(valid, alpha, dt(0))
    tall = np.cumprod(np.concatenate([np.ones((1, xs.shape[0]), dt), dt(1) - a], axis=0), axis=0, dtype=dt)      # sequential products
    tb, tn = tall[:-1], tall[1:]
    stop_any = valid & (tn < dt(1e-4))
    before = (np.cumsum(stop_any, axis=0) - stop_any) == 0          # no stop in front of it: the walk gets to it
    stops = stop_any & before
    adds = valid & before & ~stop_any
    z = P["z"][g].astype(dt)[:, None]
    expected = np.cumsum(np.where(adds, (z * a) * tb, dt(0)), axis=0, dtype=dt)[-1]      # in blending order; a Gaussian not added adds + 0
    cross = adds & (tn < dt(0.5))
    has, pos = cross.any(axis=0), cross.argmax(axis=0)
    median = np.where(has, z[pos, 0], dt(0))
    index = np.where(has, g[pos], -1)
    t_fin = np.where(stops.any(axis=0), tb[stops.argmax(axis=0), ar], tall[-1])
    near = (adds & (np.abs(tn.astype(np.float64) - 0.5) <= MEDIAN_BAND)).any(axis=0)
    return expected, median, index, np.where(has, pos, -1), dt(1) - t_fin, near


def lift(row, xs, ys, d, valid, dt):
    """The world points [..., 3] of the pixels (xs, ys) at camera depth d, (0, 0, 0) where not valid: r = ((x + 0.5 - cx) / fx,
    (y + 0.5 - cy) / fy, 1), q = d r - t, X = W^T q."""
    m = np.asarray(row, np.float32).astype(dt)
    d = np.where(valid, d, dt(0)).astype(dt)
    qx = d * (((xs.astype(dt) + dt(0.5)) - m[14]) / m[12]) - m[3]
    qy = d * (((ys.astype(dt) + dt(0.5)) - m[15]) / m[13]) - m[7]
    qz = d - m[11]
    X = [(m[k] * qx + m[4 + k] * qy) + m[8 + k] * qz for k in range(3)]
    return np.where(valid[..., None], np.stack(X, axis=-1), dt(0)).astype(dt)


def depth_view(scene, row, width, height, dtype=np.float64, scale_modifier=1.0):
    """One view -> dict of [H,W] maps: expected, median, alpha (dtype), median_index, median_pos (int64), median_undecidable (bool);
    points_median, points_expected [H,W,3] (dtype); and z [n], the p.z of every Gaussian in dtype."""
    dt = np.dtype(dtype).type
    P = RR.project(scene, row, width, height, dt, scale_modifier)
    gx, gy = P["gx"], P["gy"]
    live = np.nonzero(P["live"])[0]
    tile, gid = RR._instances(P["rect"], live, gx)
    order = np.lexsort((gid, P["z"][gid], tile))
    tile_s, gid_s = tile[order], gid[order]
    out = {k: np.zeros((height, width), dt) for k in ("expected", "median", "alpha")}
    out["median_index"] = np.full((height, width), -1, np.int64)
    out["median_pos"] = np.full((height, width), -1, np.int64)
    out["median_undecidable"] = np.zeros((height, width), bool)
    todo = np.arange(gx * gy)
    starts, ends = np.searchsorted(tile_s, todo, "left"), np.searchsorted(tile_s, todo, "right")
    for t, s0, s1 in zip(todo, starts, ends):
        if s1 == s0:
            continue
        ty, tx = divmod(int(t), gx)
        ys, xs = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, height)), np.arange(tx * TILE, min((tx + 1) * TILE, width)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        for k, v in zip(("expected", "median", "median_index", "median_pos", "alpha", "median_undecidable"),
                        _walk_tile(P, gid_s[s0:s1], xs, ys, dt)):
            out[k][ys, xs] = v
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    seen = out["alpha"] > 0
    mean = np.divide(out["expected"], out["alpha"], out=np.zeros((height, width), dt), where=seen)
    out["points_median"] = lift(row, xs, ys, out["median"], out["median_index"] >= 0, dt)
    out["points_expected"] = lift(row, xs, ys, mean, seen, dt)
    out["z"] = P["z"].astype(dt)
    return out


def depth_views(scene, rows, width, height, dtype=np.float64, **kw):
    """All views -> dict of the stacked arrays of depth_view."""
    per = [depth_view(scene, row, width, height, dtype, **kw) for row in rows]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def deviation(got, r64, keep=None):
    """max |got - r64| / max(1, |r64|) over the pixels of keep ([V,H,W], None: all): the measure of the tests' bound."""
    got, r64 = np.asarray(got).astype(np.float64), np.asarray(r64, np.float64)
    if keep is not None:
        got, r64 = got[keep], r64[keep]
    return float((np.abs(got - r64) / np.maximum(1.0, np.abs(r64))).max()) if r64.size else 0.0


MEASURED = ("expected", "points_median", "points_expected")
_cache = {}


def pair(scene, rows, width, height, undecidable):
    """Both restatements of a scene's views, read-only; `undecidable` [V,H,W] is raster_reference's flag of the same views, in either
    precision.  With it: undecidable (joined with the median's band in either precision) and rounding, the fp32 form's largest
    deviation from fp64 over MEASURED outside the undecidable pixels."""
    r64 = depth_views(scene, rows, width, height, np.float64)
    r32 = depth_views(scene, rows, width, height, np.float32)
    und = undecidable | r64["median_undecidable"] | r32["median_undecidable"]
    each = {k: deviation(r32[k], r64[k], ~und) for k in MEASURED}
    out = {"scene": scene, "rows": rows, "r64": r64, "r32": r32, "undecidable": und, "deviations": each, "rounding": max(each.values())}
    for a in (und, *r64.values(), *r32.values()):
        a.setflags(write=False)
    return out


def case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree=3):
    """The scene, the camera rows and both restatements of one case, computed once per session and shared (read-only); the scene, the
    rows and raster_reference's flags are contrib_reference.case's, which the contribution tests share."""
    key = (n, scene_seed, views, cam_seed, width, height, sh_degree)
    if key not in _cache:
        c = CR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
        _cache[key] = pair(c["scene"], c["rows"], width, height, c["undecidable"])
    return _cache[key]


def bound(rounding):
    """raster_reference.bound's rule: 4 x the fp32 restatement's own deviation, never below its floor."""
    return RR.bound(rounding)


def tolerance(c, key):
    """What the GPU's `key` (one of MEASURED) may deviate from fp64 in case c: the rule's bound on the fp32 restatement's own deviation
    of that quantity, and never more than raster_reference.ERROR_CEILING.  The ceiling CAPS the tolerance instead of disqualifying the
    case: expected / alpha divides by 1 - T, whose fp32 cancellation error at faint pixels (alpha of a few 1e-3) is amplified by the
    division -- the restatement's own points_expected deviates 1.0e-5 .. 3.1e-5 on the cases below, so that 4 x it passes the ceiling
    on most of them, and the depth channel's on the largest (1.4e-5).  No comparison is ever looser than the ceiling; the host test
    asserts that the fp32 restatement itself stays inside it."""
    return min(bound(c["deviations"][key]), RR.ERROR_CEILING)


BIG = (3000, 9, 5, 10, 96, 64, 3)           # the contribution tests' batching scene
RAGGED = (400, 13, 2, 14, 33, 17, 3)        # ragged in both axes, a partial last tile
ROUNDS = (3000, 11, 1, 12, 48, 48, 3)       # more than 256 instances per tile: lists of several LDS rounds
# (Gaussians, scene seed, views, camera seed, width, height, SH degree) of every case the GPU tests run
CASES = CR.CASES + (RAGGED, ROUNDS, BIG)
