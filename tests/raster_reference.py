"""Restatement in plain numpy of the image sixdgs_raster_views defines (include/sixdgs.h), written from that text, step by step:

  1. p = W xyz + t; culled unless p.z > 0.2                     7. tile rectangle of (u - 0.5, v - 0.5) -+ radius, 16 x 16 tiles
  2. Sigma = R S S^T R^T                                          8. SH colour towards the camera (+ 0.5, clamped below at 0)
  3. cov = (J W) Sigma (J W)^T, + 0.3 on the diagonal             9. o = sigmoid(opacity)
  4. conic = (c, -b, a) / det                                    10. order: ascending p.z (its fp32 bits), equal -> smaller index
  5. radius = ceil(3 sqrt(lambda_max))                           11. front-to-back blend with the 1/255 and 1e-4 thresholds
  6. centre u, v; pixel centres at + 0.5

It is parametrised by dtype: float64 is the reference, float32 -- the same operations in the same order, every intermediate rounded
to fp32 -- is the yardstick for what rounding alone does to the image.  The inputs are the fp32 numbers the kernel gets, widened.

A pixel is UNDECIDABLE when a discrete decision that reaches it lies within a relative band of BAND of its threshold, so that fp32
rounding may legitimately take it the other way:
  * alpha against 1/255, T' against 1e-4 (and power against 0), for a Gaussian the pixel's blend gets to;
  * p.z against 0.2, 3 sqrt(lambda) against an integer or a tile-rectangle quotient against an integer, for a Gaussian whose alpha at
    the pixel is not below 1/255 and whose rectangle, taken at both ends of the band, does not agree about the pixel's tile;
  * two Gaussians of the pixel's tile that fp32 and fp64 depths order differently (equal bits in fp32 but not in fp64 included), when
    both have an alpha not below 1/255 at the pixel and the pixel's blend gets to one of them.
A Gaussian is decidable (radii, rectangle) when none of its own three decisions lies in the band.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from splat_reference import camera_rows  # noqa: E402,F401  (the camera row is the same)

BAND = 1e-4
TILE = 16
NEAR_Z = 0.2
MAX_UNDECIDABLE_SHARE = 2e-3          # of a case's pixels
MAX_UNDECIDABLE_SHARE_FULL = 5e-3     # of the full-size test's samples
ERROR_CEILING = 5e-5                  # no case's bound may exceed it
ERROR_FLOOR = 1e-6

# (Gaussians, scene seed, views, camera seed, width, height, SH degree)
CASES = ((2000, 3, 2, 4, 128, 128, 3), (5000, 7, 2, 8, 160, 120, 3), (3000, 11, 1, 12, 48, 48, 3), (400, 13, 2, 14, 33, 17, 3),
         (300, 2, 2, 3, 40, 24, 0), (300, 2, 2, 3, 40, 24, 3))


def _sh_colour(sh, deg, x, y, z):
    """[n,3]: the emitters' SH colour (device_math.h sh_channel, row a10); sh [n,16,3] zero-padded."""
    r = 0.28209479177387814 * sh[:, 0]
    x, y, z = x[:, None], y[:, None], z[:, None]
    if deg > 0:
        c1 = 0.4886025119029199
        r = ((r - (c1 * y) * sh[:, 1]) + (c1 * z) * sh[:, 2]) - (c1 * x) * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = ((((r + (1.0925484305920792 * xy) * sh[:, 4]) + (-1.0925484305920792 * yz) * sh[:, 5]) +
              (0.31539156525252005 * ((2.0 * zz - xx) - yy)) * sh[:, 6]) + (-1.0925484305920792 * xz) * sh[:, 7]) + \
            (0.5462742152960396 * (xx - yy)) * sh[:, 8]
    if deg > 2:
        r = ((((((r + ((-0.5900435899266435 * y) * (3.0 * xx - yy)) * sh[:, 9]) + ((2.890611442640554 * xy) * z) * sh[:, 10]) +
                ((-0.4570457994644658 * y) * ((4.0 * zz - xx) - yy)) * sh[:, 11]) +
               ((0.3731763325901154 * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy)) * sh[:, 12]) +
              ((-0.4570457994644658 * x) * ((4.0 * zz - xx) - yy)) * sh[:, 13]) + ((1.445305721320277 * z) * (xx - yy)) * sh[:, 14]) + \
            ((-0.5900435899266435 * x) * (xx - 3.0 * yy)) * sh[:, 15]
    return np.maximum(r + 0.5, 0.0)


def _rotmat(q):
    """[n,3,3] of (w,x,y,z), normalised twice as device_math.h quat_to_rotmat does."""
    q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    r, x, y, z = q.T
    one = np.ones_like(r)
    return np.stack([one - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), one - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), one - 2 * (x * x + y * y)], axis=-1).reshape(-1, 3, 3)


def _depth(xyz, row, dt):
    m = np.asarray(row, np.float32).astype(dt)
    x = np.asarray(xyz, np.float32).astype(dt)
    return ((m[8] * x[:, 0] + m[9] * x[:, 1]) + m[10] * x[:, 2]) + m[11]


def _tile_bound(q, g):
    """clamp(int(q), 0, g), int() truncating towards zero."""
    return np.clip(np.trunc(np.clip(q, -1.0, g + 1.0)).astype(np.int64), 0, g)


def project(scene, row, width, height, dt, scale_modifier=1.0, scale_is_log=True, opacity_is_logit=True):
    """Steps 1-9 for one view, over the Gaussians with p.z above the band below 0.2.  Returns a dict of arrays over ALL n Gaussians.
    scale_is_log / opacity_is_logit off: scene["log_scale"] / scene["opacity"] hold the raw scales / opacities, used as they are.
    scene["sh_degree"] may be below the degree scene["f_rest"] stores: the coefficients past it are not evaluated."""
    dt = np.dtype(dt).type
    f = lambda a: np.asarray(a, np.float32).astype(dt)      # noqa: E731
    n = scene["xyz"].shape[0]
    gx, gy = -(-width // TILE), -(-height // TILE)
    m = f(row)
    fx, fy, cx, cy = m[12], m[13], m[14], m[15]
    z_all = _depth(scene["xyz"], row, dt)
    ids = np.nonzero(z_all > NEAR_Z * (1 - BAND))[0]
    out = {"n": n, "gx": gx, "gy": gy, "z": z_all, "ids": ids}
    xyz = f(scene["xyz"])[ids]
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pz = z_all[ids]
    px = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    py = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    # 2. Sigma = M M^T, M = R S
    s = f(scene["log_scale"])[ids]
    s = dt(scale_modifier) * (np.exp(s) if scale_is_log else s)
    M = _rotmat(f(scene["rot"])[ids]) * s[:, None, :]
    S = np.empty((ids.shape[0], 3, 3), dt)
    for r in range(3):
        for c in range(3):
            S[:, r, c] = (M[:, r, 0] * M[:, c, 0] + M[:, r, 1] * M[:, c, 1]) + M[:, r, 2] * M[:, c, 2]
    # 3. cov = T Sigma T^T, T = J W
    limx, limy = dt(1.3) * (dt(width) / (dt(2) * fx)), dt(1.3) * (dt(height) / (dt(2) * fy))
    tx = np.minimum(limx, np.maximum(-limx, px / pz)) * pz
    ty = np.minimum(limy, np.maximum(-limy, py / pz)) * pz
    j00, j02, j11, j12 = fx / pz, -(fx * tx) / (pz * pz), fy / pz, -(fy * ty) / (pz * pz)
    T0 = np.stack([j00 * m[k] + j02 * m[8 + k] for k in range(3)], axis=1)
    T1 = np.stack([j11 * m[4 + k] + j12 * m[8 + k] for k in range(3)], axis=1)
    v0 = np.stack([(S[:, r, 0] * T0[:, 0] + S[:, r, 1] * T0[:, 1]) + S[:, r, 2] * T0[:, 2] for r in range(3)], axis=1)
    v1 = np.stack([(S[:, r, 0] * T1[:, 0] + S[:, r, 1] * T1[:, 1]) + S[:, r, 2] * T1[:, 2] for r in range(3)], axis=1)
    a = ((T0[:, 0] * v0[:, 0] + T0[:, 1] * v0[:, 1]) + T0[:, 2] * v0[:, 2]) + dt(0.3)
    b = (T1[:, 0] * v0[:, 0] + T1[:, 1] * v0[:, 1]) + T1[:, 2] * v0[:, 2]
    c = ((T1[:, 0] * v1[:, 0] + T1[:, 1] * v1[:, 1]) + T1[:, 2] * v1[:, 2]) + dt(0.3)
    # 4., 5.
    det = a * c - b * b
    ok = det != 0
    dets = np.where(ok, det, dt(1))
    conic = np.stack([c / dets, -b / dets, a / dets], axis=1)
    mid = dt(0.5) * (a + c)
    q3 = dt(3) * np.sqrt(mid + np.sqrt(np.maximum(dt(0.1), mid * mid - det)))
    # 6., 7.: the rectangle as defined, and at both ends of the band (radius and quotients)
    u, v = fx * px / pz + cx, fy * py / pz + cy
    um, vm = u - dt(0.5), v - dt(0.5)
    radius = np.ceil(q3)
    r_lo, r_hi = np.ceil(q3 * dt(1 - BAND)), np.ceil(q3 * dt(1 + BAND))

    def bounds(cm, g):
        lo = lambda r: (cm - r) / dt(16)                    # noqa: E731
        hi = lambda r: ((cm + r) + dt(15)) / dt(16)         # noqa: E731
        c0 = [_tile_bound(lo(r) * dt(1 + sg * BAND), g) for r in (r_lo, r_hi) for sg in (-1, 1)]
        c1 = [_tile_bound(hi(r) * dt(1 + sg * BAND), g) for r in (r_lo, r_hi) for sg in (-1, 1)]
        return _tile_bound(lo(radius), g), _tile_bound(hi(radius), g), np.min(c0, 0), np.max(c0, 0), np.min(c1, 0), np.max(c1, 0)

    x0, x1, x0a, x0b, x1a, x1b = bounds(um, gx)
    y0, y1, y0a, y0b, y1a, y1b = bounds(vm, gy)
    near_ok = np.abs(pz - dt(NEAR_Z)) > NEAR_Z * BAND
    vis = (pz > dt(NEAR_Z)) & ok
    live = vis & (x1 > x0) & (y1 > y0)
    # 8., 9.
    t0, t1, t2 = m[3], m[7], m[11]
    cc = (-((m[0] * t0 + m[4] * t1) + m[8] * t2), -((m[1] * t0 + m[5] * t1) + m[9] * t2), -((m[2] * t0 + m[6] * t1) + m[10] * t2))
    dx, dy, dz = X - cc[0], Y - cc[1], Z - cc[2]
    nrm = np.maximum(np.sqrt((dx * dx + dy * dy) + dz * dz), dt(1e-12))
    sh = np.zeros((ids.shape[0], 16, 3), dt)
    sh[:, :1] = f(scene["f_dc"])[ids].reshape(-1, 1, 3)
    rest = f(scene["f_rest"])[ids]
    sh[:, 1:1 + rest.shape[1]] = rest
    colour = _sh_colour(sh, int(scene["sh_degree"]), dx / nrm, dy / nrm, dz / nrm).astype(dt)
    op = f(scene["opacity"]).reshape(-1)[ids]
    o = dt(1) / (dt(1) + np.exp(-op)) if opacity_is_logit else op

    def full(vals, fill=0):
        arr = np.full((n,) + vals.shape[1:], fill, vals.dtype)
        arr[ids] = vals
        return arr

    zero = np.zeros_like(x0)
    out.update(conic=full(conic), u=full(u), v=full(v), colour=full(colour), o=full(o), live=full(live, False),
               radii=full(np.where(live, radius, 0).astype(np.int64)),
               rect=full(np.stack([np.where(live, x0, zero), np.where(live, y0, zero), np.where(live, x1, zero), np.where(live, y1, zero)], 1)),
               outer=full(np.stack([x0a, y0a, x1b, y1b], 1)), inner=full(np.stack([x0b, y0b, x1a, y1a], 1)),
               near_ok=full(near_ok, True))
    inner_empty = (x1a <= x0b) | (y1a <= y0b)
    outer_empty = (x1b <= x0a) | (y1b <= y0a)
    same = ((x0a == x0b) & (x1a == x1b) & (y0a == y0b) & (y1a == y1b)) | (inner_empty & outer_empty)
    out["decidable"] = full(near_ok & ok & same & ((r_lo == r_hi) | outer_empty), True)
    return out


def _instances(rect, ids, gx):
    """(tile, Gaussian) of every tile of rect[ids] = (x0, y0, x1, y1), in index order, each Gaussian's in rectangle order."""
    x0, y0, x1, y1 = (rect[ids, k] for k in range(4))
    w = np.maximum(x1 - x0, 0)
    cnt = w * np.maximum(y1 - y0, 0)
    who = np.repeat(np.arange(ids.shape[0]), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ww = np.maximum(w[who], 1)
    return (y0[who] + k // ww) * gx + x0[who] + k % ww, ids[who]


def _alpha(P, g, xs, ys, dt):
    """power and unclamped-by-T alpha of Gaussians g [G] at pixels (xs, ys) [P] -> [G,P]."""
    dx = (P["u"][g, None] - xs[None, :].astype(dt)) - dt(0.5)
    dy = (P["v"][g, None] - ys[None, :].astype(dt)) - dt(0.5)
    con = P["conic"][g]
    power = dt(-0.5) * ((con[:, 0:1] * dx) * dx + (con[:, 2:3] * dy) * dy) - (con[:, 1:2] * dx) * dy
    with np.errstate(over="ignore"):
        alpha = np.minimum(dt(0.99), P["o"][g, None] * np.exp(power))
    return power, alpha


ROUND = 256


def _blend_tile(P, g, maybe, swapped, xs, ys, background, dt):
    """Step 11 for the pixels (xs, ys) of one tile; g: its Gaussians in blending order; maybe: Gaussians whose presence in the tile is
    in doubt; swapped [G]: positions of g where the other precision's depth order has another Gaussian (runs of them are permuted
    among themselves).  The Gaussians are taken in rounds, every product and sum in blending order, until every pixel has stopped.
    -> rgba [P,4], undecidable [P]."""
    npx = xs.shape[0]
    und = np.zeros(npx, bool)
    thr = dt(1.0 / 255.0)
    ar = np.arange(npx)
    T, C = np.ones(npx, dt), [np.zeros(npx, dt) for _ in range(3)]
    stopped = np.zeros(npx, bool)
    zstop = np.full(npx, np.inf)                     # depth of the Gaussian that stopped the pixel
    c0, G = 0, g.shape[0]
    while c0 < G and not stopped.all():
        c1 = min(c0 + ROUND, G)
        while c1 < G and swapped[c1 - 1] and swapped[c1]:          # a permuted run stays in one round
            c1 += 1
        gg = g[c0:c1]
        power, alpha = _alpha(P, gg, xs, ys, dt)
        valid = (power <= 0) & (alpha >= thr)
        a = np.where(valid, alpha, dt(0))
        tall = np.cumprod(np.concatenate([T[None], dt(1) - a], axis=0), axis=0, dtype=dt)      # sequential products, from the T so far
        tb, tn = tall[:-1], tall[1:]                                                           # T before / T' after each Gaussian
        stop = valid & (tn < dt(1e-4)) & ~stopped[None]
        reached = ((np.cumsum(stop, axis=0) - stop) == 0) & ~stopped[None]      # the blend gets to it (the stopping one included)
        active = reached & ~stop
        for ch in range(3):
            C[ch] = np.cumsum(np.concatenate([C[ch][None], (P["colour"][gg, ch:ch + 1] * a) * tb * active], axis=0), axis=0, dtype=dt)[-1]
        newstop = stop.any(0)
        first = stop.argmax(0)
        T = np.where(stopped, T, np.where(newstop, tb[first, ar], tn[-1]))
        zstop = np.where(newstop, P["z"][gg][first].astype(np.float64), zstop)
        near = (np.abs(alpha - thr) <= thr * BAND) | (power > -1e-6)
        near |= valid & (np.abs(tn - dt(1e-4)) <= 1e-4 * BAND)
        und |= (near & reached).any(0)
        sw = swapped[c0:c1]
        if sw.any():
            # a permuted run changes a pixel only if the blend gets to it and two of its members contribute there
            pos = np.nonzero(sw)[0]
            run = np.cumsum(np.concatenate([[True], np.diff(pos) > 1]))
            counts = (power[pos] <= 0) & (alpha[pos] >= thr * dt(1 - BAND))
            for r in np.unique(run):
                sel = run == r
                und |= (counts[sel].sum(0) >= 2) & reached[pos[sel]].any(0)
        stopped |= newstop
        c0 = c1
    if maybe.shape[0]:
        # a Gaussian whose presence is in doubt matters where it would contribute and the blend gets as far as its depth
        _, am = _alpha(P, maybe, xs, ys, dt)
        und |= ((am >= thr * dt(1 - BAND)) & (P["z"][maybe].astype(np.float64)[:, None] <= zstop[None, :] * (1 + 1e-6))).any(0)
    bg = np.asarray(background, np.float32).astype(dt)
    return np.concatenate([np.stack(C, axis=1) + T[:, None] * bg[None, :], (dt(1) - T)[:, None]], axis=1), und


def reference_view(scene, row, width, height, dtype=np.float64, scale_modifier=1.0, background=(1.0, 1.0, 1.0), tiles=None,
                   scale_is_log=True, opacity_is_logit=True):
    """One view -> dict: image [H,W,4] (dtype), undecidable [H,W], radii [n], rect [n,4], decidable [n], instances (int), and
    instances_lo / instances_hi (what the count may be once the undecidable rectangles are taken either way).
    tiles: only these tile numbers are blended (the others keep the background and are marked in `blended` [H,W] as False)."""
    dt = np.dtype(dtype).type
    P = project(scene, row, width, height, dt, scale_modifier, scale_is_log, opacity_is_logit)
    other = np.float32 if dt is np.float64 else np.float64
    z_other = _depth(scene["xyz"], row, other).astype(np.float64)
    z_own = P["z"].astype(np.float64)
    gx, gy = P["gx"], P["gy"]
    live = np.nonzero(P["live"])[0]
    count = lambda r: int((np.maximum(r[:, 2] - r[:, 0], 0) * np.maximum(r[:, 3] - r[:, 1], 0)).sum())      # noqa: E731
    doubt = P["ids"][~P["decidable"][P["ids"]]]
    if tiles is not None:       # only the Gaussians whose rectangle holds a wanted tile (counted through an integral image of the tiles)
        wanted = np.zeros((gy + 1, gx + 1), np.int64)
        wanted[1:, 1:][np.asarray(tiles) // gx, np.asarray(tiles) % gx] = 1
        wanted = wanted.cumsum(0).cumsum(1)
        holds = lambda r: (wanted[r[:, 3], r[:, 2]] - wanted[r[:, 1], r[:, 2]] - wanted[r[:, 3], r[:, 0]] + wanted[r[:, 1], r[:, 0]]) > 0   # noqa: E731
        live_t, doubt = live[holds(P["rect"][live])], doubt[holds(np.maximum(P["outer"][doubt], 0))]
    else:
        live_t = live
    tile, gid = _instances(P["rect"], live_t, gx)
    res = {"instances": count(P["rect"][live]), "instances_lo": count(P["inner"][P["ids"]][P["near_ok"][P["ids"]] & (P["z"][P["ids"]] > NEAR_Z)]),
           "instances_hi": count(P["outer"][P["ids"]]), "radii": P["radii"], "rect": P["rect"], "decidable": P["decidable"]}
    # Gaussians in doubt: outer rectangle minus inner rectangle (all of the outer one when p.z is in the band)
    dtile, dgid = _instances(P["outer"], doubt, gx)
    ty_, tx_ = dtile // gx, dtile % gx
    inn = P["inner"][dgid]
    in_inner = (tx_ >= inn[:, 0]) & (tx_ < inn[:, 2]) & (ty_ >= inn[:, 1]) & (ty_ < inn[:, 3]) & P["near_ok"][dgid]
    dtile, dgid = dtile[~in_inner], dgid[~in_inner]
    if tiles is not None:
        keep = np.isin(tile, tiles)
        tile, gid = tile[keep], gid[keep]
        keep = np.isin(dtile, tiles)
        dtile, dgid = dtile[keep], dgid[keep]
    order = np.lexsort((gid, z_own[gid], tile))
    order_other = np.lexsort((gid, z_other[gid], tile))
    tile_s, gid_s = tile[order], gid[order]
    swapped = gid_s != gid[order_other]
    dorder = np.argsort(dtile, kind="stable")
    dtile, dgid = dtile[dorder], dgid[dorder]
    image = np.empty((height, width, 4), dt)
    image[..., :3] = np.asarray(background, np.float32).astype(dt)
    image[..., 3] = 0
    und = np.zeros((height, width), bool)
    blended = np.zeros((height, width), bool)
    todo = np.arange(gx * gy) if tiles is None else np.unique(np.asarray(tiles))
    starts, ends = np.searchsorted(tile_s, todo, "left"), np.searchsorted(tile_s, todo, "right")
    dstarts, dends = np.searchsorted(dtile, todo, "left"), np.searchsorted(dtile, todo, "right")
    for t, s0, s1, d0, d1 in zip(todo, starts, ends, dstarts, dends):
        ty, tx = divmod(int(t), gx)
        ys, xs = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, height)), np.arange(tx * TILE, min((tx + 1) * TILE, width)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        g = gid_s[s0:s1]
        rgba, u_ = _blend_tile(P, g, dgid[d0:d1], swapped[s0:s1], xs, ys, background, dt)
        image[ys, xs] = rgba
        und[ys, xs] = u_
        blended[ys, xs] = True
    res.update(image=image, undecidable=und, blended=blended)
    return res


def reference_views(scene, rows, width, height, dtype=np.float64, **kw):
    """All views -> dict of stacked arrays (image [V,H,W,4], undecidable [V,H,W], radii [V,n], rect [V,n,4], decidable [V,n]) and the
    summed instance counts."""
    per = [reference_view(scene, row, width, height, dtype, **kw) for row in rows]
    out = {k: np.stack([p[k] for p in per]) for k in ("image", "undecidable", "radii", "rect", "decidable")}
    for k in ("instances", "instances_lo", "instances_hi"):
        out[k] = sum(p[k] for p in per)
    return out


_cache = {}


def raw_scene(scene, scale_is_log=True, opacity_is_logit=True):
    """The scene with its scales / opacities stored raw where the switch is off: exp / sigmoid of the stored fp32 numbers taken in fp64
    and rounded to the fp32 the kernel gets (still under the keys "log_scale" / "opacity")."""
    out = dict(scene)
    if not scale_is_log:
        out["log_scale"] = np.exp(scene["log_scale"].astype(np.float64)).astype(np.float32)
    if not opacity_is_logit:
        out["opacity"] = (1.0 / (1.0 + np.exp(-scene["opacity"].astype(np.float64)))).astype(np.float32)
    return out


def measure(scene, rows, width, height, **kw):
    """Both restatements of a scene (kw: scale_modifier, scale_is_log, opacity_is_logit), frozen -> the dict case() returns."""
    r64 = reference_views(scene, rows, width, height, np.float64, background=BACKGROUND, **kw)
    r32 = reference_views(scene, rows, width, height, np.float32, background=BACKGROUND, **kw)
    und = r64["undecidable"] | r32["undecidable"]
    dec = r64["decidable"] & r32["decidable"]
    diff = np.abs(r32["image"].astype(np.float64) - r64["image"])[~und]
    for a in (und, dec, *r64.values(), *r32.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return {"scene": scene, "rows": rows, "r64": r64, "r32": r32, "undecidable": und, "decidable": dec,
            "rounding": float(diff.max()) if diff.size else 0.0}


def case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree=3, *, stored_degree=None, scale_is_log=True, opacity_is_logit=True,
         scale_modifier=1.0):
    """The scene, the camera rows and both restatements of one case, computed once per session and shared (read-only).
    stored_degree D >= sh_degree: the scene is make_scene's of degree D, rendered at sh_degree.  scale_is_log / opacity_is_logit off:
    the scene is raw_scene's."""
    stored = sh_degree if stored_degree is None else stored_degree
    assert stored >= sh_degree
    key = (n, scene_seed, views, cam_seed, width, height, sh_degree, stored, bool(scale_is_log), bool(opacity_is_logit), float(scale_modifier))
    if key not in _cache:
        scene = raw_scene(syn.make_scene(n, scene_seed, sh_degree=stored), scale_is_log, opacity_is_logit)
        scene["sh_degree"] = np.int64(sh_degree)
        rows = camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height))
        _cache[key] = measure(scene, rows, width, height, scale_modifier=scale_modifier, scale_is_log=scale_is_log,
                              opacity_is_logit=opacity_is_logit)
    return _cache[key]


BACKGROUND = (0.25, 0.5, 1.0)


def bound(rounding):
    """The GPU image's tolerance against fp64: 4 x what fp32 rounding alone does in the restatement (another summation order and the
    hardware's exp), never below ERROR_FLOOR; a case whose bound would pass ERROR_CEILING is not a fit case."""
    return max(4.0 * rounding, ERROR_FLOOR)
