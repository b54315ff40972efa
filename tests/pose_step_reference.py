"""The pose arithmetic of render-and-compare refinement (include/sixdgs.h: sixdgs_pose_compose / sixdgs_pose_step) restated in numpy,
parametrised by dtype: compose, its chain rule to the 6-vector, Adam and the bookkeeping of the best iterate.  fp64 is the reference of
the tests; the fp32 restatement follows the header's operation order and its own distance from fp64 sets the bounds.

Bound rule, photometric_reference.bounds': per array scale = max |x64|, y = max |x32 - x64| of the restatement alone,
bound = max(8 y, 1e-6 scale), and a case is fit only when bound <= 1e-4 scale.

The fp64 restatement evaluates a, b, c to fp64's precision (the series to 12 terms below theta^2 = 1); the fp32 one is the header's
six-term Horner with fp32 coefficients, so the series' truncation (below 2e-10) is part of y."""
import math

import numpy as np

from photometric_reference import CEILING, FACTOR, FLOOR, bounds  # noqa: F401

SERIES_BELOW = 1.0                  # theta^2: ps::kSeriesBelow of csrc/pose_step.h
STATUS_NOT_FINITE, STATUS_CAPACITY = 1, 2
# the issue's list: 0, tiny, small, just below and just above the series threshold (theta = 1), 0.3, 1, 3
THETAS = (0.0, 1e-7, 1e-4, 1e-2, 1.0 - 1e-6, 1.0 + 1e-6, 0.3, 1.0, 3.0)
ADAM = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def coeffs(x, dtype):
    """a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3 of x = th^2 (array of dtype) -> three arrays."""
    x = np.asarray(x, dtype)
    terms = 6 if dtype == np.float32 else 12
    out = []
    for off in (1, 2, 3):
        fact = [dtype(math.factorial(2 * k + off)) for k in range(terms)]
        p = np.full_like(x, dtype((-1) ** (terms - 1)) / fact[terms - 1])
        for k in range(terms - 2, -1, -1):
            p = dtype((-1) ** k) / fact[k] + x * p
        out.append(p)
    big = x >= dtype(SERIES_BELOW)
    if big.any():
        xs = np.where(big, x, dtype(1.0))
        th = np.sqrt(xs)
        s, h = np.sin(th), np.sin(dtype(0.5) * th)
        closed = (s / th, (dtype(2.0) * (h * h)) / xs, (th - s) / (xs * th))
        out = [np.where(big, c, o) for c, o in zip(closed, out)]
    return out


def _theta2(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def _mm(a, b):
    """a [..., 3, 3] @ b [..., 3, k]: three terms added in index order."""
    return (a[..., :, 0, None] * b[..., 0, None, :] + a[..., :, 1, None] * b[..., 1, None, :]) + a[..., :, 2, None] * b[..., 2, None, :]


def _hat(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1), np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def delta_rotation(w, dtype):
    a, b, c = coeffs(_theta2(w), dtype)
    K = _hat(w)
    eye = np.broadcast_to(np.eye(3, dtype=dtype), K.shape)
    return (eye + a[..., None, None] * K) + b[..., None, None] * _mm(K, K), (a, b, c)


def compose(start, delta, dtype):
    """start [V,16], delta [V,6] -> rows [V,16] in dtype."""
    start, delta = np.asarray(start, dtype), np.asarray(delta, dtype)
    dR, _ = delta_rotation(delta[:, 3:], dtype)
    moved = _mm(dR, start[:, :12].reshape(-1, 3, 4))
    moved[..., 3] = moved[..., 3] + delta[:, :3]
    return np.concatenate([moved.reshape(-1, 12), start[:, 12:]], 1)


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def chain(start, delta, d_rows, dtype):
    """d L / d delta [V,6] from d L / d rows [V,16]."""
    start, delta, d_rows = (np.asarray(x, dtype) for x in (start, delta, d_rows))
    w = delta[:, 3:]
    dR, (_, b, c) = delta_rotation(w, dtype)
    G, M0 = d_rows[:, :12].reshape(-1, 3, 4), start[:, :12].reshape(-1, 3, 4)
    A = ((G[:, :, None, 0] * M0[:, None, :, 0] + G[:, :, None, 1] * M0[:, None, :, 1]) + G[:, :, None, 2] * M0[:, None, :, 2]) + G[:, :, None, 3] * M0[:, None, :, 3]
    M = _mm(A, np.swapaxes(dR, -1, -2))
    tau = np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], -1)
    k1 = _cross(w, tau)
    k2 = _cross(w, k1)
    return np.concatenate([G[:, :, 3], (tau - b[:, None] * k1) + c[:, None] * k2], 1)


def adam_constants(step, lr, beta1, beta2, eps, rounded=True):
    """(lr, beta1, beta2, eps, c1, c2) of Adam's step t = step + 1; rounded: the header's floats (c1, c2 formed in double from the
    float arguments, then rounded), otherwise plain doubles as torch.optim.Adam forms them."""
    if rounded:
        lr, beta1, beta2, eps = (float(np.float32(x)) for x in (lr, beta1, beta2, eps))
    t = step + 1
    c1, c2 = 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)
    if rounded:
        c1, c2 = float(np.float32(c1)), float(np.float32(c2))
    return lr, beta1, beta2, eps, c1, c2


def adam(g, delta, m, v, step, dtype, hyper=ADAM, rounded=True):
    """One Adam step on arrays of dtype -> (delta, m, v)."""
    lr, beta1, beta2, eps, c1, c2 = (dtype(x) for x in adam_constants(step, rounded=rounded, **hyper))
    g = np.asarray(g, dtype)
    m = beta1 * m + (dtype(1.0) - beta1) * g
    v = beta2 * v + (dtype(1.0) - beta2) * (g * g)
    delta = delta - (lr / c1) * (m / (np.sqrt(v) / c2 + eps))
    return delta, m, v


def new_state(start, dtype):
    start = np.asarray(start, np.float32)
    views = start.shape[0]
    z = np.zeros((views, 6), dtype)
    return dict(delta=z.copy(), m=z.copy(), v=z.copy(), rows=compose(start, z, dtype), best_loss=np.full(views, np.inf, dtype),
                best_step=np.zeros(views, np.int32), best_rows=start.astype(dtype), status=np.zeros(views, np.int32),
                instances_needed=np.zeros(1, np.int64))


def step(state, start, loss, d_rows, step_index, dtype, *, count=0, max_instances=1 << 30, evaluate_only=False, hyper=ADAM):
    """sixdgs_pose_step on the state dict (updated in place) -> the history row [V]."""
    s = state
    views = s["delta"].shape[0]
    loss = np.asarray(loss, np.float32).astype(dtype)
    s["instances_needed"][0] = max(int(s["instances_needed"][0]), int(count))
    if count > max_instances:
        s["status"] |= STATUS_CAPACITY
    row = np.full(views, np.nan, dtype)
    live = (s["status"] & STATUS_CAPACITY) == 0
    row[live] = loss[live]
    with np.errstate(invalid="ignore"):
        better = live & (loss < s["best_loss"])
    s["best_loss"] = np.where(better, loss, s["best_loss"])
    s["best_step"] = np.where(better, np.int32(step_index), s["best_step"])
    s["best_rows"] = np.where(better[:, None], s["rows"], s["best_rows"])
    ok = np.isfinite(loss)
    if not evaluate_only:
        ok = ok & np.isfinite(np.asarray(d_rows, np.float32)[:, :12]).all(1)
    s["status"] = np.where(live & ~ok, s["status"] | STATUS_NOT_FINITE, s["status"]).astype(np.int32)
    move = live & ((s["status"] & STATUS_NOT_FINITE) == 0)
    if evaluate_only or not move.any():
        return row
    with np.errstate(all="ignore"):
        g = chain(start, s["delta"], np.where(move[:, None], np.asarray(d_rows, np.float32), 0.0), dtype)
        delta, m, v = adam(g, s["delta"], s["m"], s["v"], step_index, dtype, hyper)
    for k, new in (("delta", delta), ("m", m), ("v", v)):
        s[k] = np.where(move[:, None], new, s[k])
    s["rows"] = np.where(move[:, None], compose(start, s["delta"], dtype), s["rows"])
    return row


def random_views(views, theta, seed, translation=0.1):
    """start rows (a random rotation, a translation of a few units, plausible intrinsics), a delta whose axis-angle has length
    theta, and a gradient d_rows [V,16] of mixed magnitudes."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((views, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w_, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y), 2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x),
                  2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)], 1).reshape(views, 3, 3)
    t = rng.uniform(-3, 3, (views, 3, 1))
    K = np.stack([rng.uniform(50, 900, views), rng.uniform(50, 900, views), rng.uniform(20, 400, views), rng.uniform(20, 400, views)], 1)
    start = np.concatenate([np.concatenate([R, t], 2).reshape(views, 12), K], 1).astype(np.float32)
    axis = rng.standard_normal((views, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    delta = np.concatenate([rng.uniform(-translation, translation, (views, 3)), axis * theta], 1).astype(np.float32)
    d_rows = (rng.standard_normal((views, 16)) * 10.0 ** rng.uniform(-3, 0, (views, 1))).astype(np.float32)
    return start, delta, d_rows
