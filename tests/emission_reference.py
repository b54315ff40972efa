"""What scene emission should produce, stated in float64 numpy from the mathematics.

This module is the independent reference of tests/test_emission_reference_host.py (CPU) and
tests/test_gpu_emission_edges.py (GPU).  It shares no code and no operation order with
6dgs_amd/csrc/device_math.h or oracle/sixdgs_oracle.c: neighbour lists are judged by fp64 distances,
normals come from numpy.linalg.eigh, ring geometry from the closed forms, the spherical harmonics
from their closed-form constants.

Reference quirks the kernels reproduce on purpose (each is visible in the oracle function named):
  * the arc-length table of a ring is sampled with the ring's own cell step, and its integrand uses
    the un-squared semi axes (o_quadricell_centers);
  * the look-up finds the largest column c with table[1 + c] < theta in the table WITHOUT its leading
    zero and then reads table[c] of the table WITH it, i.e. the entry before the last entry below
    theta (o_quadricell_centers);
  * the hemisphere mask is normal.x * p_world.x > 0, not a dot product (o_mask_and_compute_rays);
  * the Rodrigues matrix of a normal that is exactly +-z is NaN (o_rotate_isocell).
One rule is the product's own: an ellipsoid that asks for more than MAX_RINGS rings emits nothing
(k_quadricell), where the reference would run out of memory.

Tolerances.  A float result of a kernel is compared with fp64 within
    (existing kernel-vs-oracle tolerance) + (largest deviation of the fp32 CPU oracle from this module),
the second term measured by tests/test_emission_reference_host.py on the case lists below and rounded up
to one significant digit (profiles/emission_edges.md has the measurements).  Neither term comes from a kernel.
"""
import numpy as np

# ---- existing kernel-vs-oracle tolerances (tests/test_gpu_parity.py) ---------------------------------
KERNEL_ORI = 2e-6          # x magnitude (largest semi axis + |centre|)
KERNEL_DIR = 1e-6
KERNEL_RGB = 2e-6
KERNEL_NORMAL = 2e-4       # test_a4_normals_knn
# ---- measured fp32-oracle-vs-fp64 deviations, rounded up to one significant digit ----------------------
# (largest figure over the case lists below and the goldens g1-g4; the golden's own fp32 arithmetic sets it where noted)
ORACLE_CELLS = 2e-6        # quadricell cells, relative to the largest semi axis (1.41e-6 at 40 000 target cells)
ORACLE_QC_ORI = 6e-7       # quadricell ray origins, relative to (largest semi axis + |centre|) (5.68e-7)
ORACLE_QC_DIR = 6e-6       # quadricell ray directions (5.03e-6 on the (0.3, 1, 2) ellipsoid at 40 000: the table's angle error, ~6e-7
#                            rad x the largest semi axis, is divided by |p|, down to the smallest semi axis)
ORACLE_RGB = 8e-7          # SH colour on given directions, degrees 0..3 (2.95e-7; g4, whose coefficients reach 4: 7.23e-7)
ORACLE_ISO_DIRS = 9e-7     # iso-cell distribution (6.62e-7; g3: 8.13e-7)
ORACLE_ISO_ROT = 4e-7      # iso-cell directions rotated onto a normal, polar angles down to 1e-3 from +-z (3.72e-7)
ORACLE_ISO_ORI = 2e-7      # iso-cell ray origins, relative to (largest semi axis + |centre|) (1.57e-7)
ORACLE_NORMAL = 9e-5       # kNN normals up to sign where the eigen-gap is > GAP_MIN, beyond the row's eps_term (8.52e-5; with the
#                            term left in, 1.20e-3 on a row of the 262 145-point cloud whose eigenvalues are (0.024, 0.031, 0.038))
# ---- resulting tolerances ---------------------------------------------------------------------------
TOL_CELLS = KERNEL_ORI + ORACLE_CELLS
TOL_QC_ORI = KERNEL_ORI + ORACLE_QC_ORI
TOL_QC_DIR = KERNEL_DIR + ORACLE_QC_DIR
TOL_RGB = KERNEL_RGB + ORACLE_RGB
TOL_ISO_DIRS = KERNEL_DIR + ORACLE_ISO_DIRS
TOL_ISO_ROT = KERNEL_DIR + ORACLE_ISO_ROT
TOL_ISO_ORI = KERNEL_ORI + ORACLE_ISO_ORI
TOL_NORMAL = KERNEL_NORMAL + ORACLE_NORMAL    # + the row's eps_term (below)
TOL_ELLIPSOID_EQ = 1e-5    # |(x/a)^2 + (y/b)^2 + (z/c)^2 - 1| of every emitted cell
# ---- conditions (not measurements) ---------------------------------------------------------------------
KNN_SLACK = 1e-6           # relative slack on fp64 squared distances
GAP_MIN = 1e-2             # normals are compared where (l1 - l0) / l2 exceeds this
VOTE_MARGIN = 1e-4         # sign vote is borderline when some |projection| < VOTE_MARGIN * sqrt(l2)
# Reference quirk (o_sym_eig_3x3 / eig_ev0, sym_eig_3x3.py:112-143): the eigenvector of l0 is the largest cross product of two rows of
# A - l0 I, and eps = 2^-23 x sign is ADDED to each of its components before it is normalised -- in absolute units.  The cross products
# are (l1 - l0)(l2 - l0) long at most and the largest at least 1/sqrt(3) of that, so the normal turns by up to 3 eps / ((l1 - l0)(l2 - l0)):
# 1.2e-3 for a neighbourhood whose eigenvalues are (0.024, 0.031, 0.038), 1e-5 where they are ten times larger.  pca_normal returns this
# as eps_term, and a normal is compared within tolerance + eps_term of its row.
# Reference quirk (o_sym_eig_3x3, sym_eig_3x3.py:246-307): the eigenvalues are blended towards the sorted DIAGONAL of the matrix with
# weight exp(-(p1 / (6 eps))^2), p1 = sum of the squared upper off-diagonal entries and eps = 2^-23 -- in absolute units, whatever the
# scale of the cloud.  Below p1 = 4 * 6 eps the weight exceeds 1e-7 and the normal is no longer the PCA normal; such rows count
# with the small-gap rows (CAP_SMALL_GAP covers both).  mixed_cloud spreads its clouds so that neighbourhoods stay out of that regime.
BLEND_P1_MIN = 4 * 6 * 2.0 ** -23
TABLE_TIE = 1e-6           # a cell is ambiguous when its angle is within TABLE_TIE * 2 pi of a table entry
TABLE_EXACT = 1e-10        # ... and a tie when within TABLE_EXACT * 2 pi: equal, up to fp64's rounding of a 1000-term sum
FLOOR_TIE = 1e-4           # an ellipsoid's counts are ambiguous when a floored quotient is this near an integer
HEMI_TIE = 1e-6            # a cell is borderline when |n.x * p_world.x| < HEMI_TIE * |p|
MAX_RINGS = 4096
CAP_AMBIGUOUS_SMALL, CAP_AMBIGUOUS = 0.05, 0.01      # share of a case's cells, target_points <= 64 / above
CAP_BORDERLINE = 0.005
CAP_COUNT_FALLBACK = 0.02
CAP_SMALL_GAP = 0.10
MIN_CHECKED = 32


# =====================================================================================================
# kNN and normals
# =====================================================================================================
def _d2(q, c):
    d = q[:, None, 0] - c[None, :, 0]
    out = d * d
    for a in (1, 2):
        d = q[:, None, a] - c[None, :, a]
        out += d * d
    return out


def knn_accept(query, cloud, knn, k, chunk=1 << 16):
    """Per query: is knn[q] an acceptable answer to "the k nearest cloud points, nearest first, ties lowest index first"?

    All of: positions >= min(k, E) hold -1 and the others valid indices; indices distinct; every listed fp64 squared distance
    <= the min(k, E)-th smallest * (1 + KNN_SLACK); ascending within the same slack; a cloud point that coincides exactly with a
    listed neighbour and has a lower index is listed, before it."""
    query, cloud, knn = np.asarray(query, np.float64), np.asarray(cloud, np.float64), np.asarray(knn, np.int64)
    nq, e = query.shape[0], cloud.shape[0]
    m = min(int(k), e)
    assert knn.shape == (nq, k)
    ok = (knn[:, m:] == -1).all(1) & (knn[:, :m] >= 0).all(1) & (knn[:, :m] < e).all(1)
    lst = np.clip(knn[:, :m], 0, e - 1)
    srt = np.sort(lst, 1)
    ok &= (srt[:, 1:] != srt[:, :-1]).all(1)
    # One pass over the cloud in chunks: every point at most as far as the farthest LISTED neighbour (plus the slack) -- a short list
    # per query that holds the true k nearest whenever the listed entries are distinct valid points.
    nb = cloud[lst]                                                             # [nq, m, 3]
    got = ((query[:, None, :] - nb) ** 2).sum(-1)
    reach = np.where(ok, got.max(1), -1.0) * (1 + KNN_SLACK)
    cand = [[] for _ in range(nq)]
    for c0 in range(0, e, chunk):
        qi, ci = np.nonzero(_d2(query, cloud[c0:c0 + chunk]) <= reach[:, None])
        for a, b in zip(qi.tolist(), (ci + c0).tolist()):
            cand[a].append(b)
    for q in range(nq):
        if not ok[q]:
            continue
        c = np.asarray(cand[q], np.int64)
        cd = ((query[q] - cloud[c]) ** 2).sum(1)
        kth = np.partition(cd, m - 1)[m - 1]                                    # the m-th smallest fp64 distance of the whole cloud
        if not ((got[q] <= kth * (1 + KNN_SLACK)).all() and (np.diff(got[q]) >= -KNN_SLACK * kth).all()):
            ok[q] = False
            continue
        pos = {int(i): j for j, i in enumerate(lst[q])}
        for j, i in enumerate(lst[q].tolist()):
            twins = c[(c < i) & (cloud[c] == cloud[i]).all(1)]
            if any(pos.get(int(t), m) > j for t in twins):
                ok[q] = False
                break
    return ok


def pca_normal(cloud, knn):
    """Normal of each row's neighbourhood: eigenvector of the smallest eigenvalue of the centred scatter matrix (numpy.linalg.eigh),
    flipped when fewer than half of the neighbours project positively onto it.  -1 entries of knn are padding.

    Returns dict(normal [n,3] with the vote applied, axis [n,3] before it, gap [n] = (l1 - l0) / l2, flipped [n], blend [n] (see
    BLEND_P1_MIN: the reference's solver does not return the eigenvector there),
    borderline [n] = some |projection| < VOTE_MARGIN * sqrt(l2), or the vote is an even split)."""
    cloud, knn = np.asarray(cloud, np.float64), np.asarray(knn, np.int64)
    valid = knn >= 0
    cnt = valid.sum(1)
    nb = cloud[np.where(valid, knn, 0)] * valid[..., None]
    mean = nb.sum(1) / cnt[:, None]
    x = (nb - mean[:, None, :]) * valid[..., None]
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", x, x))
    axis = v[:, :, 0]
    pr = np.einsum("nki,ni->nk", x, axis)
    npos = ((pr > 0) & valid).sum(1)
    flipped = npos < 0.5 * cnt
    lmax = np.maximum(w[:, 2], 1e-300)
    # an even split cannot orient the axis at all: negating the axis leaves the split even, and neither gets flipped
    borderline = (np.where(valid, np.abs(pr), np.inf) < VOTE_MARGIN * np.sqrt(lmax)[:, None]).any(1) | (2 * npos == cnt)
    cov = np.einsum("nki,nkj->nij", x, x)
    p1 = cov[:, 0, 1] ** 2 + cov[:, 0, 2] ** 2 + cov[:, 1, 2] ** 2
    return dict(normal=np.where(flipped[:, None], -axis, axis), axis=axis, gap=(w[:, 1] - w[:, 0]) / lmax, flipped=flipped,
                borderline=borderline, blend=p1 < BLEND_P1_MIN,
                eps_term=3 * 2.0 ** -23 / np.maximum((w[:, 1] - w[:, 0]) * (w[:, 2] - w[:, 0]), 1e-300))


def check_normals(got, ref):
    """Compare fp32 normals `got` [n,3] with pca_normal's `ref`.  Returns dict(dir_err [n] up to sign, dir_checked [n] (gap > GAP_MIN and
    no blend),
    sign_ok [n], sign_checked [n] (direction checked and vote not borderline))."""
    got = np.asarray(got, np.float64)
    n = ref["normal"]
    dir_err = np.minimum(np.abs(got - n).max(1), np.abs(got + n).max(1))
    dir_checked = (ref["gap"] > GAP_MIN) & ~ref["blend"]
    sign_ok = (got * n).sum(1) > 0
    return dict(dir_err=dir_err, dir_checked=dir_checked, sign_ok=sign_ok, sign_checked=dir_checked & ~ref["borderline"], eps_term=ref["eps_term"])


# =====================================================================================================
# quadricell
# =====================================================================================================
def ellipse_perimeter(b, c):
    """Ramanujan's first approximation in the form the reference uses: pi (s + 3 (b-c)^2 / (10 s + sqrt(b^2 + 14 b c + c^2)))."""
    s = b + c
    return np.pi * (s + 3 * (b - c) ** 2 / (10 * s + np.sqrt(b * b + 14 * b * c + c * c)))


def ellipsoid_surface(a, b, c, p=1.6075):
    """Knud Thomsen's approximation."""
    return 4 * np.pi * (((a * b) ** p + (a * c) ** p + (b * c) ** p) / 3) ** (1 / p)


def _near_integer(q):
    return np.abs(q - np.round(q)) < FLOOR_TIE


def ring_plan(scale_row, target_points):
    """Rings of one ellipsoid (semi axes a, b, c; sliced along a).  Returns (rings, side, bs, cs, z, cells, floor_tie):
    per ring the semi axes of its ellipse, its offset along the slicing axis and its cell count; floor_tie says that some quotient
    that gets floored is within FLOOR_TIE of an integer (the fp32 count may then differ by one)."""
    a, b, c = (float(v) for v in scale_row)
    empty = np.zeros(0)
    if not all(np.isfinite(v) for v in (a, b, c)):
        return 0, np.nan, empty, empty, empty, empty.astype(np.int64), False
    side = np.sqrt(ellipsoid_surface(a, b, c) / target_points)
    qb, qc = ellipse_perimeter(a, b) / (2 * side), ellipse_perimeter(a, c) / (2 * side)
    if not (np.isfinite(qb) and np.isfinite(qc)):
        return 0, side, empty, empty, empty, empty.astype(np.int64), False
    tie = bool(_near_integer(qb) or _near_integer(qc))
    rings = int((np.floor(qb) + np.floor(qc)) * 0.5)
    if rings > MAX_RINGS or rings <= 0:
        return 0, side, empty, empty, empty, empty.astype(np.int64), tie and rings <= MAX_RINGS
    x = (np.arange(rings) + 0.5) * (2 * a / rings)
    f = 1 - (x - a) ** 2 / (a * a)
    bs, cs = b * np.sqrt(f), c * np.sqrt(f)
    q = ellipse_perimeter(bs, cs) / side
    tie = tie or bool(_near_integer(q).any())
    return rings, side, bs, cs, x - a, np.floor(q).astype(np.int64), tie


def quadricell_cells(scale, target_points, table_res=1000, fallback=None, _all_alternatives=False):
    """Cell centres of the quadricell partition of every ellipsoid, in the ellipsoid's own frame (slicing axis stored as z).

    scale [E,3] activated semi axes.  Returns dict(points [C,3], eid [C], ring [C], counts [E], count_tie [E], unchecked [C],
      tie [C]: the cell's angle EQUALS a table entry next to it (within TABLE_EXACT * 2 pi, fp64's own rounding).  The table is sampled
        with the ring's cell step, so this is structural -- rings of 3 or 9 cells, of 4, 8, 16 cells under a 257- or 1025-entry table
        -- and frequent at small targets (a tenth of all cells at 17 target cells).  "<" is then decided by the last bit of whoever
        computed the table, the reference included: both look-ups are the reference's answer.  alt_points [C,3] holds the other one
        for ties and is IDENTICAL to points on every other cell, so that taking the nearer of the two at the full tolerance gives
        a tie two answers and every other cell one: ties are not excluded;
      ambiguous [C]: within TABLE_TIE * 2 pi of an entry without being a tie; compared within step_bound [C] (the largest table step of
        the cell's ring x the ring's larger semi axis: how far an off-by-one look-up moves the cell).  Capped by CAP_AMBIGUOUS*.)

    An ellipsoid with count_tie takes its cells from fallback(scale_row float32 [1,3], target_points, table_res) -> points [n,3]
    (the fp32 CPU oracle): the counts are then the oracle's, and the cells are `unchecked` (ring -1), since fp64 cannot say which
    way fp32 floors there."""
    scale32 = np.asarray(scale, np.float32)
    scale = np.asarray(scale, np.float64)
    pts, eid, rid, amb, stp, tie, alt = [], [], [], [], [], [], []
    counts = np.zeros(scale.shape[0], np.int64)
    count_tie = np.zeros(scale.shape[0], bool)
    j_tab = np.arange(table_res - 1)
    for e in range(scale.shape[0]):
        rings, side, bs, cs, z, cells, count_tie[e] = ring_plan(scale[e], target_points)
        if count_tie[e]:
            p = np.asarray(fallback(scale32[e:e + 1], target_points, table_res), np.float64)
            n = p.shape[0]
            pts.append(p)
            alt.append(p)
            tie.append(np.zeros(n, bool))
            amb.append(np.zeros(n, bool))
            stp.append(np.zeros(n))
            eid.append(np.full(n, e, np.int64))
            rid.append(np.full(n, -1, np.int64))
            counts[e] = n
            continue
        for r in range(rings):
            n = int(cells[r])
            if n < 1:
                continue
            dth = 2 * np.pi / n
            th = j_tab * dth
            inc = np.sqrt(bs[r] * np.sin(th) ** 2 + cs[r] * np.cos(th) ** 2) * dth
            tab = np.concatenate([[0.0], np.cumsum(inc)])
            tab *= 2 * np.pi / tab[-1]
            theta = np.arange(n) * dth
            below = np.searchsorted(tab[1:], theta, side="left")            # entries of tab[1:] that are < theta
            tp = tab[np.maximum(below - 1, 0)]
            pts.append(np.stack([bs[r] * np.cos(tp), cs[r] * np.sin(tp), np.full(n, z[r])], 1))
            # the two entries of tab[1:] the comparison is decided between: the last one below theta and the first one not below
            d_hi = np.abs(tab[1:][np.minimum(below, table_res - 2)] - theta)
            d_lo = np.where(below > 0, np.abs(tab[1:][np.maximum(below - 1, 0)] - theta), np.inf)
            near = np.minimum(d_hi, d_lo)
            amb.append(near < TABLE_TIE * 2 * np.pi)
            tie.append(near < TABLE_EXACT * 2 * np.pi)
            # the other answer: fp32 counts the first entry not below as below, or the last entry below as not below
            other = np.clip(np.where(d_hi <= d_lo, below + 1, below - 1), 0, table_res - 1)
            ta = tab[np.maximum(other - 1, 0)]
            alt.append(np.stack([bs[r] * np.cos(ta), cs[r] * np.sin(ta), np.full(n, z[r])], 1))
            stp.append(np.full(n, np.diff(tab).max() * max(bs[r], cs[r])))
            eid.append(np.full(n, e, np.int64))
            rid.append(np.full(n, r, np.int64))
            counts[e] += n
    cat = lambda l, shape, dt: np.concatenate(l) if l else np.zeros(shape, dt)
    ring = cat(rid, 0, np.int64)
    tie = cat(tie, 0, bool)
    points = cat(pts, (0, 3), np.float64)
    alt_points = cat(alt, (0, 3), np.float64)
    if not _all_alternatives:                  # (the switch serves the test that moves a cell to the neighbouring entry on purpose)
        alt_points = np.where(tie[:, None], alt_points, points)                   # a second answer exists for ties ONLY
    return dict(points=points, eid=cat(eid, 0, np.int64), ring=ring, counts=counts, tie=tie,
                alt_points=alt_points, ambiguous=cat(amb, 0, bool) & ~tie, step_bound=cat(stp, 0, np.float64),
                count_tie=count_tie, unchecked=ring < 0)


def quat_rotation(rot):
    """Rotation matrices [n,3,3] of quaternions (w, x, y, z), normalised (floor 1e-12 on the norm) and normalised again."""
    q = np.asarray(rot, np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def quadricell_rays(points, eid, normals, xyz, rot, reach=None):
    """Rays of the cells that face the normal.  normals, xyz, rot are per emitted ellipsoid (rows eid refers to).  reach [C]: how far
    a cell may lie from `points` (the step_bound of an ambiguous cell, else 0); a cell whose |p_world.x| is within its reach may fall
    on either side of the mask and is returned as `unsure`.

    Returns dict(ori [C,3], dir [C,3] for EVERY cell, keep [C] (normal.x * p_world.x > 0), borderline [C]
    (|normal.x * p_world.x| < HEMI_TIE * |p|; a normal whose x is exactly 0 masks every cell exactly, in any precision, and is
    not borderline))."""
    points, normals, xyz = np.asarray(points, np.float64), np.asarray(normals, np.float64), np.asarray(xyz, np.float64)
    pw = np.einsum("nij,nj->ni", quat_rotation(rot)[eid], points)
    nx = normals[eid, 0]
    proj = nx * pw[:, 0]
    plen = np.linalg.norm(pw, axis=1)
    out = dict(ori=pw + xyz[eid], dir=pw / np.maximum(plen, 1e-12)[:, None], keep=proj > 0,
               borderline=(nx != 0) & (np.abs(proj) < HEMI_TIE * plen))
    if reach is not None:
        out["unsure"] = (nx != 0) & (np.abs(pw[:, 0]) <= reach) & ~out["borderline"]
    return out


def align_rays(got_ori, ref, tol):
    """Which cells a kernel's ray list consists of.  The list must hold every kept non-borderline cell, no dropped non-borderline cell,
    in cell order; a borderline cell belongs to it when the ray at its position has its origin (within tol[cell]).
    Returns the cell index of every ray, or None when the count fits no such choice."""
    bl = ref["borderline"] | ref.get("unsure", False)
    keep = ref["keep"] & ~bl
    got_ori = np.asarray(got_ori, np.float64)
    if not bl.any():
        idx = np.nonzero(keep)[0]
        return idx if idx.shape[0] == got_ori.shape[0] else None
    take = keep.copy()
    before = np.cumsum(keep) - keep            # kept non-borderline cells before each cell
    extra = 0
    for i in np.nonzero(bl)[0].tolist():
        pos = int(before[i]) + extra
        if pos < got_ori.shape[0] and np.abs(got_ori[pos] - ref["ori"][i]).max() <= tol[i]:
            take[i] = True
            extra += 1
    idx = np.nonzero(take)[0]
    return idx if idx.shape[0] == got_ori.shape[0] else None


# =====================================================================================================
# iso-cell
# =====================================================================================================
def isocell_dirs(target, n0=1):
    """Equal-area cells of the unit disc lifted to the hemisphere: n = ceil(sqrt(target / n0)) rings, ring r (1-based) has
    n0 (2r - 1) cells at radius (r - 1/2) / n, cell j at angle (j + 1/2) 2 pi / cells; z = sqrt(1 - x^2 - y^2)."""
    n = int(np.ceil(np.sqrt(target / n0)))
    r = np.arange(1, n + 1)
    cells = n0 * (2 * r - 1)
    ring = np.repeat(r, cells)
    j = np.arange(cells.sum()) - np.repeat(np.cumsum(cells) - cells, cells)
    rad = (ring - 0.5) / n
    th = (j + 0.5) * 2 * np.pi / np.repeat(cells, cells)
    x, y = rad * np.cos(th), rad * np.sin(th)
    return np.stack([x, y, np.sqrt(np.maximum(1 - x * x - y * y, 0))], 1)


def isocell_rotation(normals):
    """Rodrigues matrices [E,3,3] turning +z onto each normalised normal; NaN where the normal is exactly +-z (v = z x n = 0)."""
    b = np.asarray(normals, np.float64)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    v = np.stack([-b[:, 1], b[:, 0], np.zeros(b.shape[0])], 1)
    s2, c = (v * v).sum(1), b[:, 2]
    K = np.zeros((b.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.eye(3)[None] + K + (K @ K) * ((1 - c) / s2)[:, None, None]
    R[s2 == 0] = np.nan
    return R


def isocell_rotate(dirs, normals):
    """[E,K,3]: the distribution rotated onto every normal."""
    return np.einsum("eij,kj->eki", isocell_rotation(normals), np.asarray(dirs, np.float64))


def isocell_rays(dirs, normals, xyz, scale, rot):
    """Iso-cell rays of every ellipsoid: direction d = rotated distribution, origin = centre + d / sqrt(sum ((R^T d)_i / s_i)^2),
    the point of the ellipsoid's surface along d.  scale: activated semi axes.  Returns (ori [E,K,3], dir [E,K,3])."""
    d = isocell_rotate(dirs, normals)
    local = np.einsum("eji,ekj->eki", quat_rotation(rot), d)
    t = 1 / np.sqrt(((local / np.asarray(scale, np.float64)[:, None, :]) ** 2).sum(-1))
    return np.asarray(xyz, np.float64)[:, None, :] + t[..., None] * d, d


# =====================================================================================================
# colour
# =====================================================================================================
_PI = np.pi
SH_C0 = 0.5 / np.sqrt(_PI)
SH_C1 = np.sqrt(3 / (4 * _PI))
SH_C2 = (0.5 * np.sqrt(15 / _PI), 0.25 * np.sqrt(5 / _PI), 0.25 * np.sqrt(15 / _PI))
SH_C3 = (0.25 * np.sqrt(35 / (2 * _PI)), 0.5 * np.sqrt(105 / _PI), 0.25 * np.sqrt(21 / (2 * _PI)), 0.25 * np.sqrt(7 / _PI),
         0.25 * np.sqrt(105 / _PI))


def sh_colour(coef, dirs, degree):
    """Colour of every ray: real spherical harmonics (3D Gaussian splatting's sign convention) up to `degree`, evaluated at the view
    direction -d, plus 0.5, clamped at 0.  coef [R, >= (degree+1)^2, 3], dirs [R,3]."""
    coef, v = np.asarray(coef, np.float64), -np.asarray(dirs, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    basis = [np.full(x.shape, SH_C0)]
    if degree > 0:
        basis += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if degree > 1:
        basis += [SH_C2[0] * x * y, -SH_C2[0] * y * z, SH_C2[1] * (2 * zz - xx - yy), -SH_C2[0] * x * z, SH_C2[2] * (xx - yy)]
    if degree > 2:
        basis += [-SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * x * y * z, -SH_C3[2] * y * (4 * zz - xx - yy),
                  SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), -SH_C3[2] * x * (4 * zz - xx - yy), SH_C3[4] * z * (xx - yy),
                  -SH_C3[0] * x * (xx - 3 * yy)]
    B = np.stack(basis, 1)
    return np.maximum(np.einsum("rk,rkc->rc", B, coef[:, :B.shape[1], :]) + 0.5, 0)


# =====================================================================================================
# the case lists shared by the CPU and the GPU test (inputs only; float32 as the kernels take them)
# =====================================================================================================
NEEDLE = (1.0e4, 1.0e-4, 1.0e-4)       # ~26 000 rings at 17 target cells: more than MAX_RINGS


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def unit(v):
    v = np.asarray(v, np.float64)
    return f32(v / np.linalg.norm(v, axis=-1, keepdims=True))


def mixed_cloud(n, seed):
    """Half Gaussian, half clustered (blobs at the 125 lattice points, some sixty times the Gaussian's central density at 1.5 M points:
    crowded cells between empty ones), 1 % exact duplicates of earlier points.
    Returns (cloud float32 [n,3], indices of the duplicated rows)."""
    rng = np.random.default_rng(seed)
    half = n // 2
    spread = max(1.0, (n / 3000.0) ** (1.0 / 3.0))      # keeps neighbourhoods O(0.1..1) wide at every n: see BLEND_P1_MIN
    blobs = rng.standard_normal((n - half, 3)) * 0.05 + rng.integers(-2, 3, (n - half, 3))
    c = f32(np.concatenate([rng.standard_normal((half, 3)), blobs])[rng.permutation(n)] * spread)
    dup = rng.choice(np.arange(n // 2, n), max(n // 100, 1) if n >= 100 else 0, replace=False)
    c[dup] = c[rng.integers(0, n // 2, dup.shape[0])]
    return c, dup


def knn_probe_rows(cloud, dup, n_rows, seed):
    """Rows whose lists are judged in fp64: the points nearest the low and the high corner of the bounding box, two duplicated
    points (inside the clusters of coincident points), and random rows up to n_rows."""
    rng = np.random.default_rng(seed)
    c = cloud.astype(np.float64)
    rows = [int(np.argmin(((c - c.min(0)) ** 2).sum(1))), int(np.argmin(((c - c.max(0)) ** 2).sum(1)))]
    rows += [int(i) for i in dup[:2]]
    rest = rng.choice(cloud.shape[0], min(n_rows + len(rows), cloud.shape[0]), replace=False)
    rows += [int(i) for i in rest if int(i) not in rows][: max(n_rows - len(rows), 0)]
    return np.asarray(rows[:n_rows] if cloud.shape[0] >= n_rows else sorted(set(rows)), np.int64)


def log_uniform_scales(n, seed):
    rng = np.random.default_rng(seed)
    return f32(np.exp(rng.uniform(np.log(0.2), np.log(2.0), (n, 3))))


def cell_case_scales(target_points, seed=11):
    """8 ellipsoids (3 at the two large targets) with log-uniform semi axes over 0.2..2, plus (0.3, 1, 2)."""
    n = 3 if target_points >= 20000 else 8
    return np.concatenate([log_uniform_scales(n, seed + target_points), f32([[0.3, 1.0, 2.0]])])


def needle_case_scales(e, seed=5):
    """E ellipsoids at 17 target cells: every 7th a needle (no cells), first and last included, one NaN scale."""
    s = log_uniform_scales(e, seed + e)
    needle = (np.arange(e) % 7 == 0)
    needle[-1] = True
    s[needle] = NEEDLE
    if e > 2:
        s[min(3, e - 2), 1] = np.nan
    return s, needle


def scene_arrays(n, seed, n_coef=16):
    """A random scene: centres, quaternions (not normalised), SH coefficients."""
    rng = np.random.default_rng(seed)
    return dict(xyz=f32(rng.standard_normal((n, 3)) * 2), rot=f32(rng.standard_normal((n, 4))),
                f_dc=f32(0.3 * rng.standard_normal((n, 1, 3))), f_rest=f32(0.3 * rng.standard_normal((n, n_coef - 1, 3))))


# =====================================================================================================
# comparisons shared by the CPU and the GPU test: an implementation's numpy outputs against the reference.
# They assert what is exact (counts, ids, order, NaN pattern) and return the float errors and exclusion shares for the
# caller to bound (the CPU test bounds the oracle by ORACLE_*, the host instantiation and the kernels by TOL_*).
# =====================================================================================================
def ambiguous_cap(target_points):
    return CAP_AMBIGUOUS_SMALL if target_points <= 64 else CAP_AMBIGUOUS


def _max(a):
    return float(a.max()) if a.size else 0.0


def compare_cells(scale, target_points, table_res, got_pts, got_eid, fallback, only=None):
    """quadricell_centers' output for activated semi axes scale [E,3] against quadricell_cells.  `only`: rows whose points are
    compared (all by default); ids are checked for every row."""
    scale = np.asarray(scale, np.float32)
    e = scale.shape[0]
    got_pts, got_eid = np.asarray(got_pts, np.float64), np.asarray(got_eid, np.int64)
    assert got_eid.size == 0 or (got_eid.min() >= 0 and got_eid.max() < e)
    counts = np.bincount(got_eid, minlength=e)
    assert (got_eid == np.repeat(np.arange(e), counts)).all(), "ids are not one ascending run per ellipsoid"
    rows = np.arange(e) if only is None else np.asarray(only, np.int64)
    ref = quadricell_cells(scale[rows], target_points, table_res, fallback)
    assert (counts[rows] == ref["counts"]).all(), (counts[rows], ref["counts"])
    offs = np.cumsum(counts) - counts
    take = np.concatenate([np.arange(offs[r], offs[r] + counts[r]) for r in rows]) if rows.size else np.zeros(0, np.int64)
    g = got_pts[take]
    s = scale[rows].astype(np.float64)[ref["eid"]]
    smax = s.max(1)
    err = np.minimum(np.abs(g - ref["points"]).max(1), np.abs(g - ref["alt_points"]).max(1))
    chk = ~ref["unchecked"]
    plain, amb = chk & ~ref["ambiguous"], chk & ref["ambiguous"]
    eq = np.abs((g[:, 0] / s[:, 1]) ** 2 + (g[:, 1] / s[:, 2]) ** 2 + (g[:, 2] / s[:, 0]) ** 2 - 1)
    n = max(g.shape[0], 1)
    return dict(cells=g.shape[0], checked=int(plain.sum()), err=_max(err[plain] / smax[plain]),
                err_ambiguous=_max((err[amb] - ref["step_bound"][amb]) / smax[amb]), equation=_max(eq),
                ambiguous_share=float(amb.sum()) / n, tie_share=float(ref["tie"].sum()) / n,
                fallback_share=float(ref["count_tie"].mean()) if rows.size else 0.0)


def compare_quadricell_rays(scale, normals, xyz, rot, src_of, coef, degree, target_points, table_res, got, fallback):
    """emit_quadricell's output `got` = (ori, dir, rgb or None, src, n_cells) against the reference.  Every array argument is per EMITTED
    ellipsoid (rows gathered through sel by the caller): activated semi axes, normals, centres, quaternions, the Gaussian id each
    row reports as src, SH coefficients [E, n_coef, 3]."""
    ori, dr, rgb, src, n_cells = got
    ori, dr = np.asarray(ori, np.float64), np.asarray(dr, np.float64)
    scale = np.asarray(scale, np.float32)
    cells = quadricell_cells(scale, target_points, table_res, fallback)
    slack = np.where(cells["ambiguous"], cells["step_bound"], 0.0)
    rr = quadricell_rays(cells["points"], cells["eid"], normals, xyz, rot, reach=np.where(cells["tie"], cells["step_bound"], slack))
    ra = quadricell_rays(cells["alt_points"], cells["eid"], normals, xyz, rot)
    eid = cells["eid"]
    assert int(n_cells) == eid.shape[0], (int(n_cells), eid.shape[0])
    mag = (np.nan_to_num(scale.astype(np.float64)).max(1) + np.linalg.norm(np.asarray(xyz, np.float64), axis=1))[eid]
    idx = align_rays(ori, rr, TOL_QC_ORI * mag + np.where(cells["tie"], cells["step_bound"], slack))
    definite = int((rr["keep"] & ~rr["borderline"] & ~rr["unsure"]).sum())
    assert idx is not None, f"{ori.shape[0]} rays, fp64 keeps {definite}, {int(rr['borderline'].sum())} borderline, {int(rr['unsure'].sum())} unsure"
    assert (np.asarray(src, np.int64) == np.asarray(src_of, np.int64)[eid[idx]]).all(), "src / ray order"
    chk = ~cells["unchecked"][idx]
    plen = np.linalg.norm(cells["points"], axis=1)[idx]
    e_ori = (np.minimum(np.abs(ori - rr["ori"][idx]).max(1), np.abs(ori - ra["ori"][idx]).max(1)) - slack[idx]) / mag[idx]
    e_dir = np.minimum(np.abs(dr - rr["dir"][idx]).max(1), np.abs(dr - ra["dir"][idx]).max(1)) - slack[idx] / np.maximum(plen, 1e-300)
    out = dict(cells=eid.shape[0], rays=ori.shape[0], checked=int(chk.sum()), ori=_max(e_ori[chk]), dir=_max(e_dir[chk]),
               unit=_max(np.abs(np.linalg.norm(dr, axis=1) - 1)), borderline_share=float(rr["borderline"].mean()) if eid.size else 0.0,
               ambiguous_share=float(cells["ambiguous"].mean()) if eid.size else 0.0, tie_share=float(cells["tie"].mean()) if eid.size else 0.0,
               unsure_share=float(rr["unsure"].mean()) if eid.size else 0.0, fallback_share=float(cells["count_tie"].mean()))
    if rgb is not None:
        out["rgb"] = _max(np.abs(np.asarray(rgb, np.float64) - sh_colour(np.asarray(coef)[eid[idx]], dr, degree)))
    return out


def compare_isocell_rays(dirs, scale, normals, xyz, rot, src_of, coef, degree, got):
    """emit_isocell's output `got` = (ori, dir, rgb or None, src or None), each [E*K, ...], against isocell_rays / sh_colour.  Arrays per
    emitted ellipsoid as in compare_quadricell_rays.  The NaN pattern of origins and directions (normals exactly +-z) must be identical;
    the colours of those rays are pinned to what the code gives today (see below)."""
    ori, dr, rgb, src = got
    k = np.asarray(dirs).shape[0]
    e = np.asarray(normals).shape[0]
    ori, dr = np.asarray(ori, np.float64).reshape(e, k, 3), np.asarray(dr, np.float64).reshape(e, k, 3)
    r_ori, r_dir = isocell_rays(dirs, normals, xyz, scale, rot)
    assert (np.isnan(dr) == np.isnan(r_dir)).all() and (np.isnan(ori) == np.isnan(r_ori)).all(), "NaN pattern"
    mag = (np.asarray(scale, np.float64).max(1) + np.linalg.norm(np.asarray(xyz, np.float64), axis=1))[:, None]
    fin = ~np.isnan(r_dir).any(-1)
    out = dict(rays=e * k, checked=int(fin.sum()), ori=_max((np.abs(ori - r_ori).max(-1) / mag)[fin]), dir=_max(np.abs(dr - r_dir).max(-1)[fin]))
    if src is not None:
        assert (np.asarray(src, np.int64).reshape(e, k) == np.asarray(src_of, np.int64)[:, None]).all(), "src"
    if rgb is not None:
        want = sh_colour(np.repeat(np.asarray(coef), k, axis=0), dr.reshape(-1, 3), degree)
        rgb = np.asarray(rgb, np.float64)
        # Rays that have a direction are compared with sh_colour.  A ray without one (normal exactly +-z) gets colour NaN from the
        # reference's torch.clamp_min at degrees 1..3, but sh_channel ends in fmaxf(r + 0.5, 0), which returns 0 for a NaN
        # (device_math.h; o_eval_sh_color does the same): a known difference (profiles/emission_edges.md).  Until it is fixed the
        # tests PIN what the code does, so that a change on those rays is not silent: exactly 0 at degrees 1..3, and at degree 0,
        # where no direction enters, the colour sh_colour gives.
        fin = ~np.isnan(dr.reshape(-1, 3)).any(1)
        assert not np.isnan(rgb[fin]).any() and not np.isnan(want[fin]).any(), "NaN colour on a ray that has a direction"
        out["rgb"] = _max(np.abs(rgb - want)[fin])
        if degree > 0:
            assert (rgb[~fin] == 0).all(), "colour of a ray without a direction (pinned: 0)"
        else:
            out["rgb"] = max(out["rgb"], _max(np.abs(rgb - want)[~fin]))
        out["rays_without_direction"] = int((~fin).sum())
    return out


def compare_knn_rows(query, cloud, knn, normals, k, with_normals=True):
    """Neighbour lists and normals of some queries against fp64: every list must pass knn_accept; returns the normals' figures."""
    ok = knn_accept(query, cloud, knn, k)
    assert ok.all(), f"lists rejected in fp64: rows {np.nonzero(~ok)[0][:8].tolist()}"
    if not with_normals:
        return dict(rows=int(ok.shape[0]))
    c = check_normals(normals, pca_normal(cloud, knn))
    d, s = c["dir_checked"], c["sign_checked"]
    return dict(rows=int(ok.shape[0]), dir_checked=int(d.sum()), dir_raw=_max(c["dir_err"][d]), dir=_max((c["dir_err"] - c["eps_term"])[d]),
                small_gap_share=float((~d).mean()),
                sign_checked=int(s.sum()), sign_wrong=int((~c["sign_ok"][s]).sum()), vote_borderline_share=float((d & ~s).sum()) / max(int(d.sum()), 1))


# =====================================================================================================
# the cases (shared, so that the CPU test vets exactly what the GPU test runs)
# =====================================================================================================
GRID_SEED = 40
GRID_CLOUDS = (99_999, 100_000, 262_145, 1_500_000)     # g = 64 | 128 | 128 + second bbox stride | 256 (16 chunks of k_scan_sums)
KNN_KS = (1, 3, 20, 32)
TINY_CLOUDS = (1, 5, 19, 20, 21)
TILE_CLOUDS = (1023, 1024, 1025, 2049)                  # k_normals_knn stages the cloud through LDS 1024 points at a time
TILE_QUERIES = (1, 255, 257)
CELL_TARGETS = (17, 50, 256, 20_000, 40_000)
TABLE_RES = (2, 257, 1000, 1025)
NEEDLE_COUNTS = (1, 1024, 1025, 2049)                   # k_exclusive_scan scans 1024 counts at a time
ISO_TARGETS = ((1, 1), (35, 3), (100, 1), (300, 1))     # K = 1, 48, 100, 324


def tile_queries(nq, seed=GRID_SEED + 4):
    return f32(np.random.default_rng(seed).standard_normal((nq, 3)) * 1.5)


def oracle_cell_counts(oracle, scale, target_points):
    """Cells per ellipsoid by the fp32 CPU oracle, with the product's rule for needles (more than MAX_RINGS rings: none)."""
    scale = f32(scale)
    rings = oracle.total_rings(scale, target_points)
    return np.asarray([0 if rings[i] > MAX_RINGS else oracle.quadricell_centers(scale[i:i + 1], target_points)[1].shape[0]
                       for i in range(scale.shape[0])], np.int64)


def sampled_ellipsoids(e, needle, n=64, seed=3):
    rows = np.random.default_rng(seed).choice(e, min(n, e), replace=False)
    return np.unique(np.concatenate([rows, [0, e - 1]]))


def _sel_with_repeats(n_scene, length, seed):
    rng = np.random.default_rng(seed)
    sel = np.concatenate([rng.permutation(n_scene), rng.integers(0, n_scene, max(length - n_scene, 0))])[:length]
    if length > 2:
        sel[-1] = sel[0]
        sel[length // 2] = sel[0]
    return sel.astype(np.int64)


def _ray(id, target, deg, ncoef, log, sel=None, **kw):
    return dict(id=id, target=target, deg=deg, ncoef=ncoef, log=log, sel=sel, **kw)


RAY_CASES = (
    _ray("P17-deg0-short-log", 17, 0, 1, True),
    _ray("P50-deg1-short-sel", 50, 1, 4, False, sel=13),
    _ray("P256-deg2-short-log-sel", 256, 2, 9, True, sel=9),
    _ray("P256-deg3-full", 256, 3, 16, False),
    _ray("P50-deg1-full-log", 50, 1, 16, True),
    _ray("P50-no-rgb-log-sel", 50, 3, 16, True, sel=12, rgb=False),
    _ray("P50-res257-deg2-full", 50, 2, 16, False, res=257, reseed=1),    # first draw: a floored quotient within FLOOR_TIE of an integer
    _ray("P20000-deg3-full", 20_000, 3, 16, False),
    _ray("P40000-deg2-short-log", 40_000, 2, 9, True),
    _ray("P40000-half-chunks", 40_000, 0, 1, False, half_chunks=True),
    _ray("P17-sel1025-of-64", 17, 3, 16, True, sel=1025, scene=64),
)


def ray_case_arrays(case):
    """Inputs of emit_quadricell for a case, as the entry point takes them (scale as logs when case["log"])."""
    seed = 100 + sum(map(ord, case["id"])) + case.get("reseed", 0)
    if case.get("half_chunks"):                      # identity rotation, normal +x: p_world.x = bs cos(theta') > 0 on half of each ring
        act = f32([[0.3, 1.0, 2.0]])
        a = scene_arrays(1, seed, case["ncoef"])
        a["rot"] = f32([[1, 0, 0, 0]])
        normals = f32([[1, 0, 0]])
    else:
        if "scene" in case:
            act, _ = needle_case_scales(case["scene"], seed)
        else:
            act = cell_case_scales(case["target"], seed)
        a = scene_arrays(act.shape[0], seed, case["ncoef"])
    n = act.shape[0]
    a["sel"] = None if case["sel"] is None else _sel_with_repeats(n, case["sel"], seed)
    e = n if a["sel"] is None else a["sel"].shape[0]
    if not case.get("half_chunks"):
        normals = unit(np.random.default_rng(seed + 1).standard_normal((e, 3)))
        normals[1 % e] = (0, 1, 0)                   # x = 0: every cell of this ellipsoid is masked
    a["normals"] = normals
    a["scale"] = f32(np.log(act.astype(np.float64))) if case["log"] else act
    return a


def _activated(case, a):
    return f32(np.exp(a["scale"].astype(np.float64))) if case["log"] else a["scale"]


def ray_case_reference_args(case, a):
    """The arguments of compare_quadricell_rays in front of `got`."""
    sel = np.arange(a["xyz"].shape[0]) if a["sel"] is None else a["sel"]
    coef = np.concatenate([a["f_dc"], a["f_rest"]], 1)
    return (_activated(case, a)[sel], a["normals"], a["xyz"][sel], a["rot"][sel], sel, coef[sel], case["deg"], case["target"],
            case.get("res", 1000))


def iso_normals(e, seed):
    """Generic directions, then (from 15 ellipsoids on) +-z exactly -- unit or not -- and polar angles 1e-3, 1e-2, 1e-1 from +z and -z."""
    rng = np.random.default_rng(seed)
    n = f32(rng.standard_normal((e, 3)))
    if e >= 15:
        special = [(0, 0, 1), (0, 0, -1), (0, 0, 2.5), (0, 0, -3)]
        for i, t in enumerate((1e-3, 1e-2, 1e-1)):
            phi = 0.7 + 2.1 * i
            special += [(np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t)), (np.sin(t) * np.sin(phi), np.sin(t) * np.cos(phi), -np.cos(t))]
        n[2:2 + len(special)] = f32(special)
    return n


def _iso_cases():
    out = []
    i = 0
    for e in (1, 15, 16, 17, 33):
        for tgt, n0 in ISO_TARGETS:
            k = n0 * int(np.ceil(np.sqrt(tgt / n0))) ** 2
            deg = i % 4
            short = (i // 4) % 2 == 0
            out.append(dict(id=f"E{e}-K{k}-deg{deg}{'s' if short else 'f'}", E=e, K=k, target=tgt, n0=n0, deg=deg,
                            ncoef=(deg + 1) ** 2 if short else 16, sel=i % 2 == 1, log=(i // 2) % 2 == 0, rgb=i % 5 != 4, src=i % 7 != 3))
            i += 1
    return tuple(out)


ISO_CASES = _iso_cases()


def iso_case_arrays(case):
    seed = 500 + 41 * case["E"] + case["K"]
    e = case["E"]
    n = e + 7 if case["sel"] else e                   # a source scene larger than what is emitted
    a = scene_arrays(n, seed, case["ncoef"])
    act = log_uniform_scales(n, seed)
    a["sel"] = _sel_with_repeats(n, e, seed) if case["sel"] else None
    a["normals"] = iso_normals(e, seed + 1)
    a["scale"] = f32(np.log(act.astype(np.float64))) if case["log"] else act
    a["dirs"] = f32(isocell_dirs(case["target"], case["n0"]))
    return a


def iso_case_reference_args(case, a):
    """The arguments of compare_isocell_rays in front of `got`."""
    sel = np.arange(a["xyz"].shape[0]) if a["sel"] is None else a["sel"]
    coef = np.concatenate([a["f_dc"], a["f_rest"]], 1)
    return a["dirs"], _activated(case, a)[sel], a["normals"], a["xyz"][sel], a["rot"][sel], sel, coef[sel], case["deg"]
