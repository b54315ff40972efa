"""A plain restatement of the least-squares pose tail (sixdgs_solve_pose in include/sixdgs.h) and the seeded case generator of
tests/test_pose_tail_host.py and tests/test_gpu_pose_tail.py -- a helper of those two, not a test.  Imports without a GPU.

pose_tail(): entries with idx < 0 or idx >= R are padding at whatever position they sit and are stripped first.  The duplicate-origin
filter is PyTorch's own CPU torch.unique + torch.isin(assume_unique=True) on the fp32 origins, as the pipeline this project follows
runs it: PyTorch is the definition of that step, its choice between the two isin algorithms included, and nothing of it is
re-implemented here.  Everything after the filter is fp64 numpy, from the header's words: the unweighted least-squares centre (NaN
when the determinant of the 3x3 system is below 1e-7), exclude_negatives and the renormalised weights, the watch direction,
make_rotation_mat(-watch, up), the singular (determinant below 1e-7 -> I) and NaN (-> I4) fall-backs, the pose errors.  For every
threshold it also returns the fp64 quantity the decision rests on, so a test can tell a disagreement from a decision inside rounding.

CENTRE_C is the constant of the centre bound |c - c_64|_inf <= CENTRE_C cond(A) max(1, |c_64|_inf): four times the worst value of the
CPU oracle (fp32, sums in index order -- the order the kernel adds in) against this restatement over cases(), measured by
tests/test_pose_tail_host.py::test_reference_against_the_oracle_over_the_generator (worst 9.41e-07 of cond(A) max(1, |c|), so
CENTRE_C = 3.8e-06); that test fails when the measurement moves away from the constant."""
import functools
import math

import numpy as np
import torch

MAX_K = 256
R = 600
KS = (1, 2, 3, 63, 64, 65, 100, 101, 127, 128, 129, 191, 192, 193, 255, 256)
KINDS = ("plain", "behind", "fewdup", "heavydup", "straddle", "alphabet", "allbehind", "parallel", "upsing")
CENTRE_C = 3.8e-06
FRONT_MARGIN = 1e-4           # a kept ray whose fp64 |(c - o).d| is below this may fall on either side of exclude_negatives in fp32
SKIP_SHARE = 0.01             # at most this share of the generator's cases may be undecided in any of these ways


def small_set_threshold(kv):
    """torch.isin runs its small-set algorithm when test.numel() < this (elements.numel() = 3 kv), the sort-based one otherwise."""
    return int(10.0 * (3 * kv) ** 0.145)


def origin_filter(rows):
    """rows: fp32 [n,3].  -> (keep [n] bool, number of origins that occur once)."""
    if len(rows) == 0:
        return np.zeros(0, bool), 0
    t = torch.from_numpy(np.ascontiguousarray(rows, np.float32))
    uniq, counts = torch.unique(t, return_counts=True, dim=0)
    mask = torch.isin(t, uniq[counts == 1], assume_unique=True).any(dim=1)
    return mask.numpy().astype(bool), int((counts == 1).sum())


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def pose_tail(ori, dir, idx, val, up, gt=None):
    """One image.  ori, dir [R,3] fp32; idx [k]; val [k]; up [3]; gt [4,4] or None.  -> dict, per-ray entries at the ORIGINAL positions:
    valid, keep [k] bool; n_valid, n_once, n_kept; sorting (the isin algorithm PyTorch's rule picks for these counts); centre [3];
    w_final [k] (0 where not kept; NaN on the kept rays when the weights sum to 0); c2w [4,4]; singular_rotation, nan_pose, nan_centre and
    status (bits 0, 1, 2); cond (2-norm condition number of the 3x3 system); errors (translation, degrees) or None; and the deciding
    quantities det_centre, det_rotation, cross_norm (|up x -watch| before it is normalised) and front [k] ((c - o).d, NaN where not kept)."""
    ori32, dir32 = np.ascontiguousarray(ori, np.float32), np.ascontiguousarray(dir, np.float32)
    idx = np.asarray(idx, np.int64)
    k = len(idx)
    valid = (idx >= 0) & (idx < len(ori32))
    pos = np.nonzero(valid)[0]
    mask, n_once = origin_filter(ori32[idx[pos]])
    kept = pos[mask]
    keep = np.zeros(k, bool)
    keep[kept] = True
    m = len(kept)
    o, d = ori32[idx[kept]].astype(np.float64), dir32[idx[kept]].astype(np.float64)
    w = np.asarray(val, np.float32)[kept].astype(np.float64)
    up = np.asarray(up, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        w0 = w / w.sum()
        P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
        A = P.sum(0)
        q = np.einsum("nij,nj->ni", P, o).sum(0)
        det_c = float(np.linalg.det(A))
        cond = float(np.linalg.cond(A)) if m else float("inf")
        nan_centre = not det_c >= 1e-7
        c = np.full(3, np.nan) if nan_centre else np.linalg.solve(A, q)
        front = ((c[None] - o) * d).sum(1)
        w1 = w0 * (front > 0)
        wf = w1 / w1.sum()
        watch = np.array([math.fsum(d[:, a] * wf) for a in range(3)]) if m else np.zeros(3)
        watch = watch / math.sqrt(math.fsum(x * x for x in watch)) if np.isfinite(watch).all() else np.full(3, np.nan)
        neg = -watch
        xa = _cross(up, neg)
        cross_norm = float(np.sqrt((xa * xa).sum()))
        xa = xa / cross_norm
        ya = _cross(neg, xa)
        ya = ya / np.sqrt((ya * ya).sum())
        Rw = np.stack([xa, ya, neg])
        det_r = float(np.linalg.det(Rw)) if np.isfinite(Rw).all() else float("nan")
        singular = bool(det_r < 1e-7)
        if singular:
            Rw = np.eye(3)
        Ri = np.linalg.inv(Rw) if np.isfinite(Rw).all() else np.full((3, 3), np.nan)
        c2w = np.eye(4)
        c2w[:3, :3] = Ri
        c2w[:3, 3] = c
        nan_pose = bool(np.isnan(c2w).any())
        if nan_pose:
            c2w = np.eye(4)
        errors = None
        if gt is not None:
            g = np.asarray(gt, np.float64)
            ca = min(max((np.trace(g[:3, :3] @ np.linalg.inv(c2w[:3, :3])) - 1.0) / 2.0, -1.0), 1.0)
            errors = (float(np.linalg.norm(g[:3, 3] - c2w[:3, 3])), float(np.degrees(np.arccos(ca))))
    w_final, front_k = np.zeros(k), np.full(k, np.nan)
    w_final[kept], front_k[kept] = wf, front
    return dict(valid=valid, keep=keep, n_valid=len(pos), n_once=n_once, n_kept=m, sorting=not 3 * n_once < small_set_threshold(max(len(pos), 1)),
                centre=c, w_final=w_final, c2w=c2w, singular_rotation=singular, nan_pose=nan_pose, nan_centre=nan_centre,
                status=int(singular) | int(nan_pose) << 1 | int(nan_centre) << 2, cond=cond, errors=errors, det_centre=det_c, det_rotation=det_r,
                cross_norm=cross_norm, front=front_k)


def _clear(x, thr=1e-7):
    """x < thr is decided the same way with x a factor of 2 off (a NaN is never below thr, in any precision)."""
    return x != x or x > 2 * thr or x < thr / 2


def centre_is_decided(ref):
    """The determinant of the 3x3 system is clear of 1e-7 by a factor of 2: a NaN centre is one in fp32 too."""
    return _clear(ref["det_centre"])


def status_is_decided(ref):
    """Both determinants are clear of their threshold by a factor of 2."""
    return _clear(ref["det_centre"]) and _clear(ref["det_rotation"])


def weights_are_decided(ref):
    """No kept ray sits within FRONT_MARGIN of the plane that exclude_negatives cuts at."""
    f = ref["front"][ref["keep"]]
    return ref["nan_centre"] or not (np.abs(f) < FRONT_MARGIN).any()


# ---- the case generator ---------------------------------------------------------------------------------------------------------------

def straddle_counts(k):
    """(u_small, u_sorting): the largest number of once-only origins for which a list of k valid rays is on the small-set side, and one
    more -- each moved to the nearest count a list of k rays can have (k - u duplicated rays: never exactly one)."""
    u = (small_set_threshold(k) - 1) // 3                 # 3 u < threshold
    lo, hi = min(u, k), min(u + 1, k)
    lo = lo - 1 if k - lo == 1 else lo
    hi = hi + 1 if k - hi == 1 else hi
    return max(lo, 0), hi


def _scene(g):
    c = g.normal(size=3) * 2.0
    ori = g.normal(size=(R, 3))
    return c, ori


def _aim(g, c, ori, noise=0.05):
    d = c[None] - ori + g.normal(size=ori.shape) * noise
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _case(kind, k, j, note=""):
    g = np.random.default_rng([2025, KINDS.index(kind), k, j // 2 if kind == "straddle" else j])
    c, ori = _scene(g)
    idx = g.choice(R, size=k, replace=False).astype(np.int64)
    val = np.sort(g.random(k) + 0.05)[::-1].copy()
    up = g.normal(size=3)
    up /= np.linalg.norm(up)
    flip = np.zeros(R, bool)
    if kind == "behind":
        flip = g.random(R) < 0.15
    elif kind == "fewdup":
        for _ in range(int(g.integers(1, 6))):
            a, b = g.integers(0, k, size=2)
            ori[idx[b]] = ori[idx[a]]                       # among the selected rays, so that the copies meet in the list
    elif kind == "heavydup":
        pts = g.normal(size=(int(g.integers(1, 12)), 3))
        dup = g.random(R) < 0.9
        ori[dup] = pts[g.integers(0, len(pts), size=int(dup.sum()))]
    elif kind == "straddle":
        # lists j = 2p and 2p + 1 are one pair: the same rays, order and weights, u_small and u_sorting once-only origins -- where those
        # are one apart the two lists differ in ONE origin.  The other origins are copies in groups of >= 3 (2 when only 2 rays are left).
        u_lo, u_hi = straddle_counts(k)
        u = (u_lo, u_hi)[j % 2]
        order, sel, pts = g.permutation(k), g.normal(size=(k, 3)), g.normal(size=(max(k // 3, 1), 3))
        groups = max((k - u_hi) // 3, 1)
        sel[u:] = pts[(k - 1 - np.arange(u, k)) % groups]
        ori[idx[order]] = sel
        note = f"u={u}"
    elif kind == "alphabet":
        letters = g.integers(-3, 4, size=(R, 3)).astype(np.float64)
        if j % 3 == 1:
            ori[:, 0] = letters[:, 0]                       # coincidences through one coordinate only
        elif j % 3 == 2:
            ori[idx[: (k + 1) // 2]] = letters[idx[: (k + 1) // 2]]      # half the list on the lattice, half off it
        else:
            ori = letters
    d = _aim(g, c, ori)
    if kind == "allbehind":
        flip[:] = True
    d[flip] *= -1
    if kind == "parallel":
        d[:] = (0.0, 0.0, 1.0)
    if kind == "upsing":
        # Rays through c in the x-z plane, in adjacent pairs (s, 0, z), (-s, 0, z) of equal weight (an odd k ends on (0, 0, 1)): the
        # x sum of the watch direction cancels exactly pair by pair in any precision, y is 0, so the watch direction is exactly (0, 0, 1)
        # = up, up x -watch is exactly 0 and the x axis 0 / 0.  Origins 1..3 behind c along each ray: every ray clearly in front.
        ang = g.uniform(0.2, 1.2, size=(k + 1) // 2)
        s32, z32 = np.sin(ang).astype(np.float32), np.cos(ang).astype(np.float32)
        dsel = np.zeros((k, 3), np.float32)
        dsel[0::2, 0], dsel[0::2, 2] = s32[: len(dsel[0::2])], z32[: len(dsel[0::2])]
        dsel[1::2, 0], dsel[1::2, 2] = -s32[: len(dsel[1::2])], z32[: len(dsel[1::2])]
        if k % 2:
            dsel[-1] = (0.0, 0.0, 1.0)
        ori[idx] = c[None] - g.uniform(1.0, 3.0, size=(k, 1)) * dsel.astype(np.float64)
        d[idx] = dsel
        val[:] = 1.0
        up = np.array([0.0, 0.0, 1.0])
    gt = np.eye(4)
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, cc, dd = q
    gt[:3, :3] = [[a * a + b * b - cc * cc - dd * dd, 2 * (b * cc - a * dd), 2 * (b * dd + a * cc)],
                  [2 * (b * cc + a * dd), a * a - b * b + cc * cc - dd * dd, 2 * (cc * dd - a * b)],
                  [2 * (b * dd - a * cc), 2 * (cc * dd + a * b), a * a - b * b - cc * cc + dd * dd]]
    gt[:3, 3] = c + g.normal(size=3) * 0.1
    f = np.float32
    return dict(kind=kind, k=k, j=j, note=note, ori=ori.astype(f), dir=d.astype(f), idx=idx, val=val.astype(f), up=up.astype(f), gt=gt.astype(f))


PER_KIND = dict(plain=4, behind=4, fewdup=4, heavydup=5, straddle=4, alphabet=6, allbehind=1, parallel=1, upsing=1)


def cases(k):
    """The cases of one k: every kind, PER_KIND of each (30 in all), each with its own 600 rays.  Seeded: the same lists on every call."""
    return [_case(kind, k, j) for kind in KINDS for j in range(PER_KIND[kind])]


def stack(cs):
    """The cases of one k as one batched call: the ray sets concatenated, the indices offset.  -> ori, dir [n R,3], idx, val [n,k], up, gt."""
    ori = np.concatenate([c["ori"] for c in cs])
    dr = np.concatenate([c["dir"] for c in cs])
    idx = np.stack([c["idx"] + i * R for i, c in enumerate(cs)])
    return ori, dr, idx, np.stack([c["val"] for c in cs]), np.stack([c["up"] for c in cs]), np.stack([c["gt"] for c in cs])


@functools.lru_cache(maxsize=None)
def reference_cases(k):
    """(cases(k), their pose_tail results): computed once per process and shared by every test that needs them; treat as read-only."""
    cs = cases(k)
    return cs, [pose_tail(c["ori"], c["dir"], c["idx"], c["val"], c["up"], c["gt"]) for c in cs]


def undecided(ref):
    """A case some check is skipped for: a status decision or an exclude_negatives decision inside rounding."""
    return not status_is_decided(ref) or not weights_are_decided(ref)
