"""Adam over a scene's six parameter groups and the opacity reset (include/sixdgs.h: sixdgs_gaussian_adam / sixdgs_opacity_reset)
restated in numpy, parametrised by dtype.  fp64 is the reference of the tests; the fp32 restatement follows the header's operation
order and its own distance from fp64 sets the bounds.

Bound rule, pose_step_reference.bounds' (imported, not restated): per array scale = max |x64|, y = max |x32 - x64| of the
restatement alone, bound = max(8 y, 1e-6 scale), and a case is fit only when bound <= 1e-4 scale."""
import numpy as np

from pose_step_reference import CEILING, adam_constants, bounds  # noqa: F401

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")
STATUS_NOT_FINITE, STATUS_CAPACITY = 1, 2
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-15)
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)          # the reference's defaults, six different rates


def widths(n_coef):
    return (3, 3, 3 * (n_coef - 1), 1, 3, 4)


def slices(n, n_coef):
    out, off = {}, 0
    for k, w in zip(GROUPS, widths(n_coef)):
        out[k] = slice(off, off + n * w)
        off += n * w
    return out


def adam_step(params, grads, m, v, step, lrs, dtype, hyper=HYPER, rounded=True):
    """One step on params (dict name -> flat array of dtype, in place), m, v (flat, in place) -> the status bits.  grads[k] None:
    frozen.  An entry whose gradient is not finite keeps p, m, v and sets bit 0."""
    n_coef = 1 + params["f_rest"].size // max(params["xyz"].size, 1)
    sl = slices(params["xyz"].size // 3, n_coef)
    status = 0
    for k, lr in zip(GROUPS, lrs):
        g = grads.get(k)
        if g is None or params[k].size == 0:
            continue
        lr_, beta1, beta2, eps, c1, c2 = (dtype(x) for x in adam_constants(step, lr, rounded=rounded, **hyper))
        g32 = np.asarray(g, np.float32).reshape(-1)
        ok = np.isfinite(g32)
        if not ok.all():
            status |= STATUS_NOT_FINITE
        g = np.where(ok, g32, np.float32(0)).astype(dtype)
        p, mm, vv = params[k].reshape(-1), m[sl[k]], v[sl[k]]
        m1 = beta1 * mm + (dtype(1.0) - beta1) * g
        v1 = beta2 * vv + (dtype(1.0) - beta2) * (g * g)
        with np.errstate(all="ignore"):
            p1 = p - (lr_ / c1) * (m1 / (np.sqrt(v1) / c2 + eps))
        params[k].reshape(-1)[...] = np.where(ok, p1, p)
        m[sl[k]] = np.where(ok, m1, mm)
        v[sl[k]] = np.where(ok, v1, vv)
    return status


def reset(x, ceiling, dtype, is_logit=True):
    """min(sigmoid(x), ceiling) stored back as a logit (is_logit) or min(x, ceiling) itself."""
    x = np.asarray(x, dtype)
    a = dtype(1.0) / (dtype(1.0) + np.exp(-x)) if is_logit else x
    o = np.minimum(a, dtype(ceiling))
    return np.log(o / (dtype(1.0) - o)) if is_logit else o


def random_case(n, n_coef, seed, steps=3):
    """(params, m, v, grads): float32 arrays of a plausible scene, a random optimiser state (v > 0) and `steps` gradient dicts of
    mixed magnitudes."""
    rng = np.random.default_rng(1000 * n + 10 * n_coef + seed)
    size = n * (11 + 3 * n_coef)
    params = {k: (rng.standard_normal(n * w) * s).astype(np.float32)
              for (k, w), s in zip(zip(GROUPS, widths(n_coef)), (1.0, 0.5, 0.1, 2.0, 1.0, 1.0))}
    params["scale"] -= np.float32(4.0)
    mag = 10.0 ** rng.uniform(-5, -1, size)
    m = (rng.standard_normal(size) * mag).astype(np.float32)
    v = ((rng.uniform(0.5, 2.0, size) * mag) ** 2).astype(np.float32)
    grads = []
    for _ in range(steps):
        g, off = {}, 0
        for k, w in zip(GROUPS, widths(n_coef)):
            g[k] = (rng.standard_normal(n * w) * mag[off:off + n * w] * rng.uniform(0.5, 2.0, n * w)).astype(np.float32)
            off += n * w
        grads.append(g)
    return params, m, v, grads


def run(params, m, v, grads, dtype, lrs=LRS, hyper=HYPER, first_step=0):
    """`len(grads)` steps on copies in dtype -> (params, m, v, status)."""
    p = {k: a.astype(dtype) for k, a in params.items()}
    m, v, status = m.astype(dtype), v.astype(dtype), 0
    for i, g in enumerate(grads):
        status |= adam_step(p, g, m, v, first_step + i, lrs, dtype, hyper)
    return p, m, v, status
