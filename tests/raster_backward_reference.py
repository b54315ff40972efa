"""Restatement in torch of steps 1-11 of sixdgs_raster_views (include/sixdgs.h), in the operation order of tests/raster_reference.py,
so that torch.autograd on the CPU gives the gradients sixdgs_raster_views_backward defines: float64 is the reference, float32 the
yardstick for what rounding alone does to a gradient.

The discrete parts are not differentiated and come from raster_reference of the same dtype: which Gaussians are live and their tile
rectangles (RR.project), the instances (RR._instances) and their order (a lexsort on tile, depth, index).  Every tile's pixels are
blended Gaussian by Gaussian; the continuous clamps are torch.clamp / torch.minimum / torch.maximum, the two skips and the stop are
torch.where on decisions taken in the same dtype.

The test loss is sum(g * image_f32) with g standard-normal fp32 from default_rng(1), SET TO ZERO on every pixel RR.case marks
undecidable in either precision: a pixel's decisions reach no other pixel, so a legitimately flipped decision changes no gradient."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as RR  # noqa: E402

NAMES = ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest", "cams")
# the four cases of the issue: partial tiles on both axes and two views; SH degree 0 with an empty f_rest; SH degree 3; up to 894
# instances in one tile (four staging rounds, walked backwards)
CASES = ((400, 13, 2, 14, 33, 17, 3), (300, 2, 2, 3, 40, 24, 0), (300, 2, 2, 3, 40, 24, 3), (3000, 11, 1, 12, 48, 48, 3))
FACTOR = 8.0               # two fp32 evaluations in different summation orders, each within y of fp64, and not at the same entry
FLOOR = 1e-6               # of max |g64|
CEILING = 1e-4             # of max |g64|: a case whose bound passes it is not a fit case


def _sh_colour(sh, deg, x, y, z):
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
    return torch.clamp(r + 0.5, min=0.0)


def _rotmat(q):
    q = q / torch.clamp(torch.sqrt((q * q).sum(-1, keepdim=True)), min=1e-12)
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    r, x, y, z = q.unbind(-1)
    one = torch.ones_like(r)
    return torch.stack([one - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), one - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), one - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def _project(t, m, live, width, height, sh_degree, scale_modifier, scale_is_log=True, opacity_is_logit=True):
    """Steps 1-6, 8, 9 for the live Gaussians of one view, differentiable -> conic [L,3], u, v, colour [L,3], o."""
    fx, fy, cx, cy = m[12], m[13], m[14], m[15]
    xyz = t["xyz"][live]
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pz = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    px = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    py = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    sc = t["log_scale"][live]
    s = scale_modifier * (torch.exp(sc) if scale_is_log else sc)
    M = _rotmat(t["rot"][live]) * s[:, None, :]
    S = [[(M[:, r, 0] * M[:, c, 0] + M[:, r, 1] * M[:, c, 1]) + M[:, r, 2] * M[:, c, 2] for c in range(3)] for r in range(3)]
    limx, limy = 1.3 * (width / (2 * fx)), 1.3 * (height / (2 * fy))
    tx = torch.minimum(limx, torch.maximum(-limx, px / pz)) * pz
    ty = torch.minimum(limy, torch.maximum(-limy, py / pz)) * pz
    j00, j02, j11, j12 = fx / pz, -(fx * tx) / (pz * pz), fy / pz, -(fy * ty) / (pz * pz)
    T0 = [j00 * m[k] + j02 * m[8 + k] for k in range(3)]
    T1 = [j11 * m[4 + k] + j12 * m[8 + k] for k in range(3)]
    v0 = [(S[r][0] * T0[0] + S[r][1] * T0[1]) + S[r][2] * T0[2] for r in range(3)]
    v1 = [(S[r][0] * T1[0] + S[r][1] * T1[1]) + S[r][2] * T1[2] for r in range(3)]
    a = ((T0[0] * v0[0] + T0[1] * v0[1]) + T0[2] * v0[2]) + 0.3
    b = (T1[0] * v0[0] + T1[1] * v0[1]) + T1[2] * v0[2]
    c = ((T1[0] * v1[0] + T1[1] * v1[1]) + T1[2] * v1[2]) + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], dim=1)
    u, v = fx * px / pz + cx, fy * py / pz + cy
    t0, t1, t2 = m[3], m[7], m[11]
    cc = (-((m[0] * t0 + m[4] * t1) + m[8] * t2), -((m[1] * t0 + m[5] * t1) + m[9] * t2), -((m[2] * t0 + m[6] * t1) + m[10] * t2))
    dx, dy, dz = X - cc[0], Y - cc[1], Z - cc[2]
    nrm = torch.clamp(torch.sqrt((dx * dx + dy * dy) + dz * dz), min=1e-12)
    rest = t["f_rest"][live]
    sh = torch.cat([t["f_dc"][live].reshape(-1, 1, 3), rest, torch.zeros(live.shape[0], 15 - rest.shape[1], 3, dtype=xyz.dtype)], dim=1)
    colour = _sh_colour(sh, sh_degree, dx / nrm, dy / nrm, dz / nrm)
    op = t["opacity"].reshape(-1)[live]
    o = 1 / (1 + torch.exp(-op)) if opacity_is_logit else op
    return conic, u, v, colour, o


def _blend_tile(conic, u, v, colour, o, g, xs, ys, bg):
    """Step 11 for the pixels (xs, ys) of one tile, Gaussian by Gaussian in the order g -> rgba [P,4]."""
    dt = conic.dtype
    xs, ys = torch.from_numpy(xs).to(dt), torch.from_numpy(ys).to(dt)
    T = torch.ones(xs.shape[0], dtype=dt)
    C = [torch.zeros(xs.shape[0], dtype=dt) for _ in range(3)]
    stopped = torch.zeros(xs.shape[0], dtype=torch.bool)
    zero = torch.zeros((), dtype=dt)
    top = torch.tensor(0.99, dtype=dt)
    for j in g.tolist():
        dx, dy = (u[j] - xs) - 0.5, (v[j] - ys) - 0.5
        power = -0.5 * ((conic[j, 0] * dx) * dx + (conic[j, 2] * dy) * dy) - (conic[j, 1] * dx) * dy
        alpha = torch.minimum(top, o[j] * torch.exp(torch.where(power <= 0, power, zero)))
        valid = (power <= 0) & (alpha >= 1.0 / 255.0)
        Tn = T * (1 - alpha)
        stopped = stopped | (valid & (Tn < 1e-4))
        act = valid & ~stopped
        for ch in range(3):
            C[ch] = C[ch] + torch.where(act, (colour[j, ch] * alpha) * T, zero)
        T = torch.where(act, Tn, T)
        if bool(stopped.all()):
            break
    return torch.stack([C[0] + T * bg[0], C[1] + T * bg[1], C[2] + T * bg[2], 1 - T], dim=1)


def render(t, rows, width, height, sh_degree, background=RR.BACKGROUND, scale_modifier=1.0, scale_is_log=True, opacity_is_logit=True):
    """image_f32 [V,H,W,4] of the tensors t (xyz, log_scale, rot, opacity, f_dc, f_rest) and rows [V,16], all of one dtype.
    scale_is_log / opacity_is_logit off: t["log_scale"] / t["opacity"] hold the raw values (RR.project)."""
    dt = rows.dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    scene = {k: t[k].detach().numpy().astype(np.float32) for k in NAMES[:-1]}
    scene["sh_degree"] = sh_degree
    bg = torch.tensor(np.asarray(background, np.float32).astype(npdt))
    images = []
    for vw in range(rows.shape[0]):
        row = rows[vw].detach().numpy().astype(np.float32)
        P = RR.project(scene, row, width, height, npdt, scale_modifier, scale_is_log, opacity_is_logit)
        gx, gy = P["gx"], P["gy"]
        live = np.nonzero(P["live"])[0]
        where = np.full(P["n"], -1, np.int64)
        where[live] = np.arange(live.shape[0])
        conic, u, v, colour, o = _project(t, rows[vw], torch.from_numpy(live), width, height, sh_degree, scale_modifier,
                                          scale_is_log, opacity_is_logit)
        tile, gid = RR._instances(P["rect"], live, gx)
        order = np.lexsort((gid, P["z"][gid], tile))
        tile, gid = tile[order], where[gid[order]]
        image = torch.zeros(height, width, 4, dtype=dt)
        starts, ends = np.searchsorted(tile, np.arange(gx * gy), "left"), np.searchsorted(tile, np.arange(gx * gy), "right")
        for tl in range(gx * gy):
            ty_, tx_ = divmod(tl, gx)
            ys, xs = np.meshgrid(np.arange(ty_ * RR.TILE, min((ty_ + 1) * RR.TILE, height)),
                                 np.arange(tx_ * RR.TILE, min((tx_ + 1) * RR.TILE, width)), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            image[torch.from_numpy(ys), torch.from_numpy(xs)] = _blend_tile(conic, u, v, colour, o, gid[starts[tl]:ends[tl]], xs, ys, bg)
        images.append(image)
    return torch.stack(images)


def gradients(scene, rows, width, height, dtype, g, background=RR.BACKGROUND, scale_modifier=1.0, scale_is_log=True, opacity_is_logit=True):
    """-> dict: image [V,H,W,4] and the gradient of sum(g * image) by each of NAMES, as numpy arrays of `dtype`."""
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    t = {k: torch.from_numpy(np.ascontiguousarray(scene[k], np.float32)).to(dt).requires_grad_(True) for k in NAMES[:-1]}
    cams = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(dt).requires_grad_(True)
    image = render(t, cams, width, height, int(scene["sh_degree"]), background, scale_modifier, scale_is_log, opacity_is_logit)
    (image * torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(dt)).sum().backward()
    out = {k: (t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])).numpy() for k in NAMES[:-1]}
    out["cams"] = (cams.grad if cams.grad is not None else torch.zeros_like(cams)).numpy()
    out["image"] = image.detach().numpy()
    return out


def loss_weights(shape, und):
    """The loss weights: standard-normal fp32, zero on the undecidable pixels."""
    g = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    g[und] = 0
    return g


def bounds(g64, g32):
    """Per array: (scale = max |g64|, y = max |g32 - g64|, bound = max(FACTOR y, FLOOR scale))."""
    out = {}
    for k in NAMES:
        scale = float(np.abs(g64[k]).max()) if g64[k].size else 0.0
        y = float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) if g64[k].size else 0.0
        out[k] = (scale, y, max(FACTOR * y, FLOOR * scale))
    return out


_cache = {}


def measure(rr, width, height, **kw):
    """Of an RR.measure / RR.case result rr (kw: the switches it was made with): the loss weights and both restatements' gradients,
    frozen -> the dict case() returns."""
    views = rr["rows"].shape[0]
    g = loss_weights((views, height, width, 4), rr["undecidable"])
    g64 = gradients(rr["scene"], rr["rows"], width, height, np.float64, g, **kw)
    g32 = gradients(rr["scene"], rr["rows"], width, height, np.float32, g, **kw)
    for a in (g, *g64.values(), *g32.values()):
        a.setflags(write=False)
    return {"scene": rr["scene"], "rows": rr["rows"], "rr": rr, "g": g, "g64": g64, "g32": g32, "bounds": bounds(g64, g32)}


def case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree=3, *, stored_degree=None, scale_is_log=True, opacity_is_logit=True,
         scale_modifier=1.0):
    """RR.case of the same arguments, the loss weights and both restatements' gradients, computed once per session (read-only)."""
    kw = dict(scale_is_log=bool(scale_is_log), opacity_is_logit=bool(opacity_is_logit), scale_modifier=float(scale_modifier))
    key = (n, scene_seed, views, cam_seed, width, height, sh_degree, sh_degree if stored_degree is None else stored_degree, *kw.values())
    if key not in _cache:
        _cache[key] = measure(RR.case(syn, *key[:7], stored_degree=stored_degree, **kw), width, height, **kw)
    return _cache[key]


# the parameterisations sixdgs_raster_views accepts beyond the stored-log, stored-logit, modifier-1, full-degree corner of CASES: all on
# 300 Gaussians, 2 views, 40 x 24 (partial tiles on both axes).  (name, positional arguments of case(), keyword arguments of case())
PARAM_BASE = (300, 2, 2, 3, 40, 24)
PARAM_CASES = (
    ("degree 0 of 16", PARAM_BASE + (0,), dict(stored_degree=3)),
    ("degree 1 of 4", PARAM_BASE + (1,), {}),
    ("degree 1 of 16", PARAM_BASE + (1,), dict(stored_degree=3)),
    ("degree 2 of 9", PARAM_BASE + (2,), {}),
    ("degree 2 of 16", PARAM_BASE + (2,), dict(stored_degree=3)),
    ("raw scale", PARAM_BASE + (3,), dict(scale_is_log=False)),
    ("raw opacity", PARAM_BASE + (3,), dict(opacity_is_logit=False)),
    ("raw scale, raw opacity, degree 1 of 16", PARAM_BASE + (1,), dict(stored_degree=3, scale_is_log=False, opacity_is_logit=False)),
    ("modifier 0.5", PARAM_BASE + (3,), dict(scale_modifier=0.5)),
    ("modifier 1.7", PARAM_BASE + (3,), dict(scale_modifier=1.7)),
    ("raw scale, modifier 0.5", PARAM_BASE + (3,), dict(scale_is_log=False, scale_modifier=0.5)),
    ("raw scale, modifier 1.7", PARAM_BASE + (3,), dict(scale_is_log=False, scale_modifier=1.7)),
)
