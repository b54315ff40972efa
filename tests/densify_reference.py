"""Adaptive density control (include/sixdgs.h: sixdgs_densify_stats / sixdgs_densify) restated in numpy and torch for the tests.

  thresholds, classify, round_np   one round: the rules in fp32 bit for bit (comparisons on stored values with thresholds converted
                                   once in double), the candidate order, the compaction, m / v; children's positions in fp32 or fp64
                                   (the expf of a child's position is the one function no restatement has to the bit)
  stats_update                     the statistics update from a given grad2d [V,N,2] and radii [V,N], in fp32 bit for bit
  grad2d                           dL / d(u, v) per (view, Gaussian) by autograd of tests/raster_backward_reference.py's restatement,
                                   with u, v of RB._project retained as leaves
  train_walk                       a literal walk of the reference's train.py:152-184 -> what happens at every iteration"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")
KEEP, CLONE, SPLIT = 0, 1, 2
LOG_SPLIT = np.float32(0.470003629)
F = np.float32


def group_widths(n_coef):
    return (3, 3, 3 * (n_coef - 1), 1, 3, 4)


def thresholds(grad_threshold, percent_dense, extent, min_opacity, scale_is_log=True, opacity_is_logit=True):
    """Each threshold converted once, in double, from the float32 arguments into the stored domain, rounded to float32."""
    dense, world, p = float(F(percent_dense)) * float(F(extent)), 0.1 * float(F(extent)), float(F(min_opacity))
    if scale_is_log:
        dense, world = math.log(dense), math.log(world)
    if opacity_is_logit:
        p = math.log(p / (1.0 - p)) if p > 0 else -math.inf
    return {"grad": F(grad_threshold), "dense": F(dense), "world": F(world), "opacity": F(p)}


def classify(grad_accum, denom, scale, t):
    """-> (avg fp32 [n], cls [n]): avg = denom > 0 ? grad_accum / denom : 0; clone / split by avg >= grad and max scale > dense."""
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.where(denom > 0, grad_accum.astype(F) / denom.astype(F), F(0)).astype(F)
    big = scale.max(axis=1) > t["dense"]
    sel = avg >= t["grad"]
    return avg, np.where(sel & big, SPLIT, np.where(sel, CLONE, KEEP))


def rotmat(q, dt):
    """device_math.h quat_to_rotmat in its operation order, in dt."""
    q = q.astype(dt)
    sq = lambda a: np.sqrt(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]) + a[:, 3] * a[:, 3])  # noqa: E731
    q = q / np.maximum(sq(q), dt(1e-12))[:, None]
    q = q / sq(q)[:, None]
    r, x, y, z = q.T
    one, two = dt(1), dt(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y), two * (x * y + r * z),
                     one - two * (x * x + z * z), two * (y * z - r * x), two * (x * z - r * y), two * (y * z + r * x),
                     one - two * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def child_xyz(xyz, rot, scale, z, scale_is_log, dt):
    """xyz + R (sigma * z) in dt, the 3-term products added in index order."""
    R = rotmat(rot, dt)
    s = scale.astype(dt)
    y = (np.exp(s) if scale_is_log else s) * z.astype(dt)
    return xyz.astype(dt) + ((R[:, :, 0] * y[:, None, 0] + R[:, :, 1] * y[:, None, 1]) + R[:, :, 2] * y[:, None, 2])


def child_scale(scale, scale_is_log):
    return (scale - LOG_SPLIT if scale_is_log else scale / F(1.6)).astype(F)


def round_np(params, m, v, stats, noise, t, prune_big, screen_size=0, scale_is_log=True, dt=np.float32):
    """One round on numpy arrays: params by GROUPS' names, m / v flat (group after group), stats the three arrays, t = thresholds().
    -> dict: the six arrays, m, v (flat, at n_out), counts (n_out, clones, splits, pruned), cls, avg, src [n_out] (source index),
    seg [n_out] (0 original, 1 clone, 2 / 3 child copy 0 / 1), child_xyz64 [n_out,3] (fp64 positions; NaN where not a child)."""
    n = params["xyz"].shape[0]
    n_coef = 1 + params["f_rest"].shape[1]
    avg, cls = classify(stats["grad_accum"], stats["denom"], params["scale"], t)
    split, clone = np.nonzero(cls == SPLIT)[0], np.nonzero(cls == CLONE)[0]
    src = np.concatenate([np.nonzero(cls != SPLIT)[0], clone, split, split]).astype(np.int64)
    seg = np.concatenate([np.zeros(n - split.size), np.ones(clone.size), np.full(split.size, 2), np.full(split.size, 3)]).astype(np.int64)
    cand = {k: params[k][src].copy() for k in GROUPS}
    child = seg >= 2
    cand["scale"][child] = child_scale(params["scale"][src[child]], scale_is_log)
    pos64 = np.full((src.size, 3), np.nan)
    if child.any():
        s, j = src[child], seg[child] - 2
        cand["xyz"][child] = child_xyz(params["xyz"][s], params["rot"][s], params["scale"][s], noise[s, j], scale_is_log, dt).astype(F)
        pos64[child] = child_xyz(params["xyz"][s], params["rot"][s], params["scale"][s], noise[s, j], scale_is_log, np.float64)
    radius = np.where(seg == 0, stats["max_radii"][src], 0)
    prune = cand["opacity"].reshape(-1) < t["opacity"]
    if prune_big:
        prune = prune | (cand["scale"].max(axis=1) > t["world"])
        if screen_size > 0:
            prune = prune | (radius > screen_size)
    keep = ~prune
    out = {k: cand[k][keep] for k in GROUPS}
    n_out = int(keep.sum())
    ms, vs, off = [], [], 0
    for k, w in zip(GROUPS, group_widths(n_coef)):
        for flat, dst in ((m, ms), (v, vs)):
            rows = flat[off:off + n * w].reshape(n, w)[src]
            rows[seg != 0] = 0
            dst.append(rows[keep].reshape(-1))
        off += n * w
    out.update(m=np.concatenate(ms).astype(F), v=np.concatenate(vs).astype(F), cls=cls, avg=avg, src=src[keep], seg=seg[keep],
               child_xyz64=pos64[keep], counts=(n_out, int(clone.size), int(split.size), int(src.size - n_out)))
    return out


def stats_update(stats, grad2d, radii, width, height):
    """The three statistics after one sixdgs_densify_stats call, from grad2d [V,N,2] fp32 and radii [V,N]: views in ascending order,
    a (view, Gaussian) with radius > 0 adds sqrt((0.5 W du)^2 + (0.5 H dv)^2) in fp32, 1 and takes the larger radius."""
    acc, den, rad = stats["grad_accum"].astype(F).copy(), stats["denom"].astype(np.int32).copy(), stats["max_radii"].astype(np.int32).copy()
    hw, hh = F(0.5) * F(width), F(0.5) * F(height)
    for view in range(grad2d.shape[0]):
        vis = radii[view] > 0
        a, b = hw * grad2d[view, :, 0].astype(F), hh * grad2d[view, :, 1].astype(F)
        g = np.sqrt(a * a + b * b).astype(F)
        acc = np.where(vis, acc + g, acc).astype(F)
        den = den + vis.astype(np.int32)
        rad = np.where(vis, np.maximum(rad, radii[view]), rad).astype(np.int32)
    return {"grad_accum": acc, "denom": den, "max_radii": rad}


def grad2d(scene, rows, width, height, dtype, g, background=RR.BACKGROUND):
    """dL / d(u, v) of L = sum(g * image_f32) for every (view, Gaussian) -> [V,N,2] in `dtype`, zeros where the Gaussian is not live:
    RB.render's loop with u, v of RB._project detached into leaves, so that their gradients are the sums over the instances."""
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    npdt = np.float64 if dt == torch.float64 else np.float32
    t = {k: torch.from_numpy(np.array(scene[k], np.float32)).to(dt) for k in RB.NAMES[:-1]}
    cams = torch.from_numpy(np.array(rows, np.float32)).to(dt)
    sc = {k: np.asarray(scene[k], np.float32) for k in RB.NAMES[:-1]}
    sc["sh_degree"] = int(scene["sh_degree"])
    bg = torch.tensor(np.asarray(background, np.float32).astype(npdt))
    gw = torch.from_numpy(np.array(g, np.float32)).to(dt)
    n = sc["xyz"].shape[0]
    out = np.zeros((rows.shape[0], n, 2), npdt)
    for vw in range(rows.shape[0]):
        P = RR.project(sc, np.asarray(rows[vw], np.float32), width, height, npdt, 1.0)
        gx, gy = P["gx"], P["gy"]
        live = np.nonzero(P["live"])[0]
        where = np.full(n, -1, np.int64)
        where[live] = np.arange(live.shape[0])
        conic, u, v, colour, o = RB._project(t, cams[vw], torch.from_numpy(live), width, height, sc["sh_degree"], 1.0)
        u, v = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
        tile, gid = RR._instances(P["rect"], live, gx)
        order = np.lexsort((gid, P["z"][gid], tile))
        tile, gid = tile[order], where[gid[order]]
        starts, ends = np.searchsorted(tile, np.arange(gx * gy), "left"), np.searchsorted(tile, np.arange(gx * gy), "right")
        loss = torch.zeros((), dtype=dt)
        for tl in range(gx * gy):
            ty_, tx_ = divmod(tl, gx)
            ys, xs = np.meshgrid(np.arange(ty_ * RR.TILE, min((ty_ + 1) * RR.TILE, height)),
                                 np.arange(tx_ * RR.TILE, min((tx_ + 1) * RR.TILE, width)), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            rgba = RB._blend_tile(conic, u, v, colour, o, gid[starts[tl]:ends[tl]], xs, ys, bg)
            loss = loss + (rgba * gw[vw][torch.from_numpy(ys), torch.from_numpy(xs)]).sum()
        if live.size and loss.requires_grad:
            loss.backward()
            out[vw, live, 0] = u.grad.numpy()
            out[vw, live, 1] = v.grad.numpy()
    return out


def train_walk(iterations, densify_from_iter, densify_until_iter, densification_interval, opacity_reset_interval, white_background=False):
    """train.py:152-184 walked literally for iteration = 1 .. iterations -> lists of the iterations that accumulate statistics, that
    densify (with the size threshold's truth value), that reset the opacity, and that step the optimiser on anything: a densifying
    iteration's fresh parameters carry no gradient, so torch's Adam steps nothing there."""
    stats, rounds, size_threshold, resets, steps = [], [], [], [], []
    for iteration in range(1, iterations + 1):
        has_grad = True
        if iteration < densify_until_iter:
            stats.append(iteration)
            if iteration > densify_from_iter and iteration % densification_interval == 0:
                rounds.append(iteration)
                size_threshold.append(bool(20 if iteration > opacity_reset_interval else None))
                has_grad = False
            if iteration % opacity_reset_interval == 0 or (white_background and iteration == densify_from_iter):
                resets.append(iteration)
        if iteration < iterations and has_grad:
            steps.append(iteration)
    return {"stats": stats, "round": rounds, "prune_big": size_threshold, "reset": resets, "update": steps}


OPTS = dict(grad_threshold=2e-4, percent_dense=0.01, extent=3.0, min_opacity=0.005)       # t_dense at sigma 0.03, t_world at 0.3


def random_case(n, n_coef, seed, scale_is_log=True, opacity_is_logit=True):
    """A scene of n Gaussians around OPTS' thresholds with its optimiser state, statistics and noise, all float32 / int32: sigma
    log-uniform in [0.002, 0.8] (clone and split sources, children above and below t_world), opacity in [0.001, 0.9] (some below
    min_opacity), denom in [0, 4] with zeros, the average gradient uniform in [0, 6e-4]."""
    rng = np.random.default_rng(seed)
    sigma = np.exp(rng.uniform(np.log(0.002), np.log(0.8), (n, 1))) * rng.uniform(0.7, 1.3, (n, 3))
    o = rng.uniform(0.001, 0.9, n)
    denom = rng.integers(0, 5, n).astype(np.int32)
    params = {"xyz": rng.standard_normal((n, 3)), "f_dc": rng.standard_normal((n, 1, 3)), "f_rest": rng.standard_normal((n, n_coef - 1, 3)),
              "opacity": (np.log(o / (1 - o)) if opacity_is_logit else o).reshape(n, 1), "scale": np.log(sigma) if scale_is_log else sigma,
              "rot": rng.standard_normal((n, 4))}
    params = {k: np.ascontiguousarray(a, F) for k, a in params.items()}
    size = n * (11 + 3 * n_coef)
    stats = {"grad_accum": (np.maximum(denom, 1) * rng.uniform(0, 6e-4, n)).astype(F), "denom": denom,
             "max_radii": rng.integers(0, 40, n).astype(np.int32)}
    return {"params": params, "m": rng.standard_normal(size).astype(F), "v": np.abs(rng.standard_normal(size)).astype(F), "stats": stats,
            "noise": rng.standard_normal((n, 2, 3)).astype(F)}


def xyz_bound(r32, r64):
    """The bound on children's positions against fp64, by the project's bounds() rule: (scale, y, max(FACTOR y, FLOOR scale)) with
    y the fp32 restatement's own error."""
    scale = float(np.abs(r64).max()) if r64.size else 0.0
    y = float(np.abs(r32.astype(np.float64) - r64).max()) if r64.size else 0.0
    return scale, y, max(RB.FACTOR * y, RB.FLOOR * scale)
