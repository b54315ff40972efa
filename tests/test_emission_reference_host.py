"""CPU tests that make tests/emission_reference.py (fp64) trustworthy before a GPU sees it, and that run the case lists of
tests/test_gpu_emission_edges.py with CPU code in the kernels' place.

  (a) the reference against the reference-generated goldens g1-g4;
  (b) the fp32 CPU oracle against the reference on every case list: this MEASURES the ORACLE_* constants of the reference module
      (each test prints its figure; the assertion is that the constant, the figure rounded up to one significant digit, still holds);
  (c) the host instantiation of device_math.h (libsixdgs_hostcheck.so) against the reference on the same case lists within the
      TOL_* the GPU test uses, and inside every exclusion cap.  A case whose inputs break a cap is replaced here (another seed), never
      loosened on the GPU.

Case sizes are the GPU test's, except that the neighbour searches run the oracle's exhaustive search on the probe rows only.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import emission_reference as R


@pytest.fixture(scope="module")
def hc():
    b = importlib.import_module("6dgs_amd.build")
    lib = C.CDLL(b.build_hostcheck())
    lib.hc_quadricell_centers.restype = C.c_longlong
    lib.hc_emit_rays.restype = C.c_longlong
    lib.hc_isocell_dirs.restype = C.c_longlong
    return lib


def P(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


f32 = R.f32


class Oracle:
    """The fp32 CPU oracle behind the interface of 6dgs_amd.ops that the comparisons need (numpy in, numpy out)."""
    name = "oracle"

    def __init__(self, oracle, hc=None):
        self.o = oracle

    def fallback(self, scale_row, target, res):
        return self.o.quadricell_centers(scale_row, target, res)[0]

    def _emitting(self, scale, target):
        """The product's rule for needles (k_quadricell): more than MAX_RINGS rings -> no cells.  The CPU code would walk them all."""
        scale = f32(scale).copy()
        scale[self.o.total_rings(scale, target) > R.MAX_RINGS] = np.nan
        return scale

    def quadricell_centers(self, scale, target, res=1000):
        return self.o.quadricell_centers(self._emitting(scale, target), target, res)

    def rays(self, pts, eid, normals, xyz, rot):
        return self.o.mask_and_compute_rays(pts, eid, normals, xyz, self.o.build_rotation(rot))

    def sh(self, coef, dirs, deg):          # coef [R, n_coef, 3]
        return self.o.eval_sh_color(np.ascontiguousarray(f32(coef).transpose(0, 2, 1)), dirs, deg)

    def emit_quadricell(self, xyz, scale, rot, coef, deg, sel, normals, target, res=1000, scale_is_log=True, want_rgb=True):
        sel = np.arange(xyz.shape[0]) if sel is None else np.asarray(sel, np.int64)
        act = f32(np.exp(f32(scale))) if scale_is_log else f32(scale)
        pts, eid = self.quadricell_centers(act[sel], target, res)
        ori, dr, mid = self.rays(pts, eid, normals, xyz[sel], rot[sel])
        rgb = self.sh(coef[sel][mid], dr, deg) if want_rgb else None
        return ori, dr, rgb, sel[mid], pts.shape[0]

    def isocell_distribution(self, target, n0=1):
        return self.o.isocell_distribution(target, n0)

    def rotate_isocell(self, dirs, normals):
        return self.o.rotate_isocell(dirs, normals)

    def emit_isocell(self, xyz, scale, rot, coef, deg, sel, normals, dirs, scale_is_log=True, want_rgb=True, want_src=True):
        """The origin formula lives in k_emit_isocell alone; its stand-in is the same formula in float32 numpy."""
        sel = np.arange(xyz.shape[0]) if sel is None else np.asarray(sel, np.int64)
        act = (f32(np.exp(f32(scale))) if scale_is_log else f32(scale))[sel]
        d = f32(self.rotate_isocell(dirs, normals))                                     # [E,K,3]
        loc = np.einsum("eji,ekj->eki", f32(self.o.build_rotation(rot[sel])), d).astype(np.float32)
        u = loc / act[:, None, :]
        with np.errstate(invalid="ignore"):
            t = (np.float32(1) / np.sqrt((u * u).sum(-1, dtype=np.float32))).astype(np.float32)
        ori = (xyz[sel][:, None, :] + t[..., None] * d).astype(np.float32).reshape(-1, 3)
        d = d.reshape(-1, 3)
        k = dirs.shape[0]
        rgb = self.sh(np.repeat(coef[sel], k, axis=0), d, deg) if want_rgb else None
        return ori, d, rgb, (np.repeat(sel, k) if want_src else None)

    def normals_knn(self, query, cloud, k):
        return self.o.compute_normals(query, cloud, k, return_knn=True)


class Host(Oracle):
    """The host instantiation of device_math.h in the kernels' place (the search itself is the oracle's: it is not per-thread math)."""
    name = "hostcheck"

    def __init__(self, oracle, hc):
        self.o, self.hc = oracle, hc

    def quadricell_centers(self, scale, target, res=1000):
        sc = self._emitting(scale, target)
        n = self.hc.hc_quadricell_centers(P(sc), C.c_longlong(sc.shape[0]), target, res, None, None)
        pts, eid = np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
        self.hc.hc_quadricell_centers(P(sc), C.c_longlong(sc.shape[0]), target, res, P(pts), P(eid, C.c_longlong))
        return pts, eid

    def rays(self, pts, eid, normals, xyz, rot):
        n = pts.shape[0]
        ori, dr, mid = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
        r = self.hc.hc_emit_rays(P(f32(pts)), P(np.ascontiguousarray(eid, np.int64), C.c_longlong), C.c_longlong(n), P(f32(normals)),
                                 P(f32(xyz)), P(f32(rot)), P(ori), P(dr), P(mid, C.c_longlong))
        return ori[:r].copy(), dr[:r].copy(), mid[:r].copy()

    def sh(self, coef, dirs, deg):
        coef = np.ascontiguousarray(f32(coef).transpose(0, 2, 1))
        out = np.zeros((dirs.shape[0], 3), np.float32)
        self.hc.hc_sh_color(P(coef), coef.shape[2], P(f32(dirs)), C.c_longlong(dirs.shape[0]), deg, P(out))
        return out

    def isocell_distribution(self, target, n0=1):
        n = self.hc.hc_isocell_dirs(target, n0, None)
        d = np.zeros((n, 3), np.float32)
        self.hc.hc_isocell_dirs(target, n0, P(d))
        return d

    def rotate_isocell(self, dirs, normals):
        out = np.zeros((normals.shape[0], dirs.shape[0], 3), np.float32)
        self.hc.hc_rotate_isocell(P(f32(dirs)), C.c_longlong(dirs.shape[0]), P(f32(normals)), C.c_longlong(normals.shape[0]), P(out))
        return out

    def normals_knn(self, query, cloud, k):
        _, knn = self.o.compute_normals(query, cloud, k, return_knn=True)
        if cloud.shape[0] < k:                      # hc_normals_from_knn takes full lists only
            return _, knn
        n = np.zeros((query.shape[0], 3), np.float32)
        self.hc.hc_normals_from_knn(P(f32(cloud)), P(np.ascontiguousarray(knn), C.c_longlong), C.c_longlong(query.shape[0]), k, P(n))
        return n, knn


@pytest.fixture(scope="module", params=[Oracle, Host], ids=["oracle", "hostcheck"])
def impl(request, oracle, hc):
    return request.param(oracle, hc)


def bound(impl, oracle_dev, tol):
    """The oracle is held to the measured deviation, the stand-in of the kernels to the tolerance the GPU test uses."""
    return oracle_dev if impl.name == "oracle" else tol


def normals_within(impl, st):
    """Direction error beyond the row's eps_term (the reference solver's regulariser, see the reference module)."""
    return st["dir"] <= bound(impl, R.ORACLE_NORMAL, R.TOL_NORMAL)


def report(tag, impl, figures):
    print(f"[emission] {tag} {impl.name}: " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


# =====================================================================================================
# (a) the reference against the goldens
# =====================================================================================================
@pytest.mark.parametrize("Pt", [50, 64, 256])
def test_reference_agrees_with_golden_quadricell(golden, oracle, Pt):
    """g1: cell counts and ids identical to the reference implementation's, cells within ORACLE_CELLS outside the ambiguous ones, the ray
    set identical, origins and directions within ORACLE_QC_*."""
    g = golden("g1_quadricell")
    fb = Oracle(oracle).fallback
    st = R.compare_cells(g["scale"], Pt, 1000, g[f"P{Pt}_points"], g[f"P{Pt}_eid"], fb)
    print(st)
    assert st["err"] <= R.ORACLE_CELLS and st["err_ambiguous"] <= R.ORACLE_CELLS and st["equation"] <= R.TOL_ELLIPSOID_EQ
    # the golden's ellipsoids are what they are (5.2 % of their cells are ambiguous at 50 target cells): the exclusion caps are for
    # the case lists below, whose inputs can be replaced; here the compared share must just stay the bulk
    assert st["checked"] >= 0.9 * st["cells"] and st["fallback_share"] <= R.CAP_COUNT_FALLBACK
    E = g["scale"].shape[0]
    got = (g[f"P{Pt}_ori"], g[f"P{Pt}_dir"], None, g[f"P{Pt}_mid"], g[f"P{Pt}_points"].shape[0])
    st = R.compare_quadricell_rays(g["scale"], g["normals"], g["xyz"], g["rot"], np.arange(E), None, 0, Pt, 1000, got, fb)
    print(st)
    assert st["ori"] <= R.ORACLE_QC_ORI and st["dir"] <= R.ORACLE_QC_DIR and st["borderline_share"] + st["unsure_share"] <= R.CAP_BORDERLINE


def test_reference_agrees_with_golden_normals(golden):
    """g2: the reference implementation's own neighbour lists pass knn_accept (its distances come from a matrix product, so as in
    test_a4_normals_knn a hundredth of the rows may differ in the last places), and pca_normal reproduces its normals."""
    g = golden("g2_normals")
    pts, knn = g["pts"], np.ascontiguousarray(g["knn"], np.int64)
    ok = R.knn_accept(pts, pts, knn, 20)
    assert ok.mean() > 0.99
    c = R.check_normals(g["normals"], R.pca_normal(pts, knn))
    d, s = c["dir_checked"], c["sign_checked"]
    print("g2 normals: dir", c["dir_err"][d].max(), "small gap share", (~d).mean(), "sign checked", s.sum(), "wrong", (~c["sign_ok"][s]).sum())
    assert (c["dir_err"] - c["eps_term"])[d].max() <= R.ORACLE_NORMAL and (~d).mean() <= R.CAP_SMALL_GAP and c["sign_ok"][s].all() and s.sum() >= R.MIN_CHECKED


@pytest.mark.parametrize("tgt,n0", [(35, 3), (64, 1), (256, 1)])
def test_reference_agrees_with_golden_isocell(golden, tgt, n0):
    g = golden("g3_isocell")
    ref = g[f"dirs_{tgt}_{n0}"]
    d = R.isocell_dirs(tgt, n0)
    assert d.shape == ref.shape and np.abs(d - ref).max() <= R.ORACLE_ISO_DIRS
    if n0 == 1:
        rot, want = R.isocell_rotate(ref, g["normals"]), g[f"rot_{tgt}"]
        assert (np.isnan(rot) == np.isnan(want)).all() and np.nanmax(np.abs(rot - want)) <= R.ORACLE_ISO_ROT


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_reference_agrees_with_golden_sh(golden, deg):
    g = golden("g4_sh")
    assert np.abs(R.sh_colour(g["sh"].transpose(0, 2, 1), g["dir"], deg) - g[f"rgb_deg{deg}"]).max() <= R.ORACLE_RGB


# =====================================================================================================
# (b) + (c) the case lists of the GPU test, oracle and host instantiation in the kernels' place
# =====================================================================================================
@pytest.mark.parametrize("n", R.GRID_CLOUDS)
def test_knn_rows_of_the_grid_clouds(impl, n):
    """The clouds of the GPU test's grid cases: lists and normals of the 64 probe rows."""
    cloud, dup = R.mixed_cloud(n, R.GRID_SEED)
    rows = R.knn_probe_rows(cloud, dup, 64, 1)
    nrm, knn = impl.normals_knn(cloud[rows], cloud, 20)
    st = R.compare_knn_rows(cloud[rows], cloud, knn, nrm, 20)
    report(f"grid cloud {n}", impl, st)
    assert normals_within(impl, st) and st["sign_wrong"] == 0
    assert st["small_gap_share"] <= R.CAP_SMALL_GAP and st["dir_checked"] >= R.MIN_CHECKED


@pytest.mark.parametrize("k", R.KNN_KS)
def test_knn_every_k(impl, k):
    cloud, _ = R.mixed_cloud(3000, R.GRID_SEED + 1)
    nrm, knn = impl.normals_knn(cloud, cloud, k)
    st = R.compare_knn_rows(cloud, cloud, knn, nrm, k, with_normals=k >= 20)
    report(f"k={k}", impl, st)
    if k >= 20:
        assert normals_within(impl, st) and st["sign_wrong"] == 0
        assert st["small_gap_share"] <= R.CAP_SMALL_GAP and st["dir_checked"] >= R.MIN_CHECKED


@pytest.mark.parametrize("e", R.TINY_CLOUDS)
def test_knn_tiny_clouds(oracle, e):
    """Fewer points than k: all points in distance order, then -1."""
    cloud, _ = R.mixed_cloud(e, R.GRID_SEED + 2)
    _, knn = oracle.compute_normals(cloud, cloud, 20, return_knn=True)
    assert R.knn_accept(cloud, cloud, knn, 20).all()
    assert (knn[:, min(e, 20):] == -1).all()
    if e <= 20:
        assert (np.sort(knn[:, :e], 1) == np.arange(e)[None, :]).all()


@pytest.mark.parametrize("e", R.TILE_CLOUDS)
def test_knn_tile_edge_clouds(impl, e):
    cloud, _ = R.mixed_cloud(e, R.GRID_SEED + 3)
    q = R.tile_queries(257)
    nrm, knn = impl.normals_knn(q, cloud, 20)
    st = R.compare_knn_rows(q, cloud, knn, nrm, 20)
    report(f"tile cloud {e}", impl, st)
    assert normals_within(impl, st) and st["sign_wrong"] == 0 and st["small_gap_share"] <= R.CAP_SMALL_GAP
    assert st["dir_checked"] >= R.MIN_CHECKED


def test_knn_accept_rejects_wrong_lists(oracle):
    """The judge itself: a swapped pair, a farther point, a repeated index, reversed duplicates and wrong padding are all rejected."""
    cloud, dup = R.mixed_cloud(3000, R.GRID_SEED + 1)
    rows = R.knn_probe_rows(cloud, dup, 64, 1)
    _, knn = oracle.compute_normals(cloud[rows], cloud, 20, return_knn=True)
    assert R.knn_accept(cloud[rows], cloud, knn, 20).all()
    d = ((cloud[rows, None, :].astype(np.float64) - cloud[knn]) ** 2).sum(-1)
    bad = knn.copy()
    far = np.argsort(((cloud[rows[:1]].astype(np.float64) - cloud) ** 2).sum(1))[25]
    bad[0, 19] = far                                                       # not among the 20 nearest
    bad[1, 5] = bad[1, 4]                                                  # repeated index
    j = int(np.argmax(np.diff(d[2]) > 1e-3 * d[2, 19]))
    bad[2, [j, j + 1]] = bad[2, [j + 1, j]]                                # not ascending
    bad[3, 19] = -1                                                        # padding where a neighbour belongs
    assert not R.knn_accept(cloud[rows], cloud, bad, 20)[:4].any() and R.knn_accept(cloud[rows], cloud, bad, 20)[4:].all()
    # coincident points must come lowest index first
    twin = np.repeat(cloud[:50], 2, axis=0)
    _, knn = oracle.compute_normals(twin, twin, 4, return_knn=True)
    assert R.knn_accept(twin, twin, knn, 4).all()
    swapped = knn.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]                                 # the point itself and its twin, at distance 0
    assert not R.knn_accept(twin, twin, swapped, 4).any()


@pytest.mark.parametrize("target", R.CELL_TARGETS)
def test_quadricell_cells(impl, target):
    """The chunk edges of k_quadricell's cell loop: 20 000 target cells give a ring of 364 cells (two chunks of 256), 40 000 one of 515."""
    scale = R.cell_case_scales(target)
    pts, eid = impl.quadricell_centers(scale, target)
    st = R.compare_cells(scale, target, 1000, pts, eid, impl.fallback)
    report(f"cells P={target}", impl, st)
    tol = bound(impl, R.ORACLE_CELLS, R.TOL_CELLS)
    assert st["err"] <= tol and st["err_ambiguous"] <= tol and st["equation"] <= R.TOL_ELLIPSOID_EQ
    assert st["ambiguous_share"] <= R.ambiguous_cap(target) and st["fallback_share"] <= R.CAP_COUNT_FALLBACK
    assert st["checked"] >= R.MIN_CHECKED or target < 32
    if target >= 20000:
        widest = np.bincount(R.quadricell_cells(scale[-1:], target)["ring"]).max()
        assert widest > (256 if target == 20000 else 512)


def test_a_cell_one_table_entry_off_is_rejected(oracle):
    """The comparison itself: a single cell that is no tie, moved to the neighbouring table entry, breaks the cell tolerance by orders of
    magnitude, in the cells and in the rays; a tie moved to its other look-up is accepted (both are the reference's answer)."""
    impl = Oracle(oracle)
    scale = R.cell_case_scales(256)
    ref = R.quadricell_cells(scale, 256)
    pts, eid = impl.quadricell_centers(scale, 256)
    assert (ref["alt_points"][~ref["tie"]] == ref["points"][~ref["tie"]]).all() and ref["tie"].any()
    good = R.compare_cells(scale, 256, 1000, pts, eid, impl.fallback)
    assert good["err"] <= R.ORACLE_CELLS
    # the other look-up of every cell, computed as for ties: one table entry away
    full = R.quadricell_cells(scale, 256, _all_alternatives=True)["alt_points"]
    moved = np.abs(full - ref["points"]).max(1) > 100 * R.TOL_CELLS * scale[ref["eid"]].max(1)
    assert moved.mean() > 0.9                                     # (cell 0 of a ring looks up entry 0 either way)
    plain = np.nonzero(~ref["tie"] & ~ref["ambiguous"] & moved)[0]
    for i in plain[[0, len(plain) // 2, -1]]:
        bad = pts.copy()
        bad[i] = full[i]
        assert R.compare_cells(scale, 256, 1000, bad, eid, impl.fallback)["err"] > 100 * R.TOL_CELLS
    swapped = pts.copy()
    swapped[ref["tie"]] = full[ref["tie"]]
    assert R.compare_cells(scale, 256, 1000, swapped, eid, impl.fallback)["err"] <= R.ORACLE_CELLS
    # rays: the same move on a cell that is kept, well away from the mask
    case = next(c for c in R.RAY_CASES if c["id"] == "P256-deg3-full")
    a = R.ray_case_arrays(case)
    coef = np.concatenate([a["f_dc"], a["f_rest"]], 1)
    got = impl.emit_quadricell(a["xyz"], a["scale"], a["rot"], coef, 3, None, a["normals"], 256, 1000, False, True)
    args = R.ray_case_reference_args(case, a)
    assert R.compare_quadricell_rays(*args, got, impl.fallback)["ori"] <= R.ORACLE_QC_ORI
    cells = R.quadricell_cells(args[0], 256)
    full = R.quadricell_cells(args[0], 256, _all_alternatives=True)["alt_points"]
    rr = R.quadricell_rays(cells["points"], cells["eid"], args[1], args[2], args[3])
    ra = R.quadricell_rays(full, cells["eid"], args[1], args[2], args[3])
    kept = np.nonzero(rr["keep"])[0]
    cand = [r for r, i in enumerate(kept) if not cells["tie"][i] and not cells["ambiguous"][i] and ra["keep"][i]
            and abs(rr["ori"][i][0] - args[2][cells["eid"][i]][0]) > 10 * cells["step_bound"][i]]
    r = cand[len(cand) // 2]
    ori = got[0].copy()
    ori[r] = ra["ori"][kept[r]]
    st = R.compare_quadricell_rays(*args, (ori,) + tuple(got[1:]), impl.fallback)
    assert st["ori"] > 100 * R.TOL_QC_ORI


@pytest.mark.parametrize("res", R.TABLE_RES)
def test_quadricell_table_resolutions(impl, res):
    scale = R.cell_case_scales(50)
    pts, eid = impl.quadricell_centers(scale, 50, res)
    st = R.compare_cells(scale, 50, res, pts, eid, impl.fallback)
    report(f"cells res={res}", impl, st)
    tol = bound(impl, R.ORACLE_CELLS, R.TOL_CELLS)
    assert st["err"] <= tol and st["err_ambiguous"] <= tol and st["equation"] <= R.TOL_ELLIPSOID_EQ
    assert st["ambiguous_share"] <= R.ambiguous_cap(50) and st["fallback_share"] <= R.CAP_COUNT_FALLBACK


@pytest.mark.parametrize("e", R.NEEDLE_COUNTS)
def test_quadricell_needles_and_offsets(impl, oracle, e):
    """k_exclusive_scan's chunk edges: E = 1024 / 1025 / 2049 ellipsoids, every 7th (first and last included) without cells."""
    scale, needle = R.needle_case_scales(e)
    pts, eid = impl.quadricell_centers(scale, 17)
    counts = R.oracle_cell_counts(oracle, scale, 17)
    assert (counts[needle] == 0).all() and (np.bincount(eid, minlength=e) == counts).all()
    assert (eid == np.repeat(np.arange(e), counts)).all()
    only = R.sampled_ellipsoids(e, needle)
    st = R.compare_cells(scale, 17, 1000, pts, eid, impl.fallback, only=only)
    report(f"needles E={e}", impl, st)
    tol = bound(impl, R.ORACLE_CELLS, R.TOL_CELLS)
    assert st["err"] <= tol and st["err_ambiguous"] <= tol and st["equation"] <= R.TOL_ELLIPSOID_EQ
    assert st["ambiguous_share"] <= R.ambiguous_cap(17) and st["fallback_share"] <= R.CAP_COUNT_FALLBACK


@pytest.mark.parametrize("case", R.RAY_CASES, ids=lambda c: c["id"])
def test_quadricell_rays(impl, case):
    a = R.ray_case_arrays(case)
    coef = np.concatenate([a["f_dc"], a["f_rest"]], 1)
    got = impl.emit_quadricell(a["xyz"], a["scale"], a["rot"], coef, case["deg"], a["sel"], a["normals"], case["target"],
                               case.get("res", 1000), case["log"], case.get("rgb", True))
    st = R.compare_quadricell_rays(*R.ray_case_reference_args(case, a), got, impl.fallback)
    report(case["id"], impl, st)
    assert st["ori"] <= bound(impl, R.ORACLE_QC_ORI, R.TOL_QC_ORI) and st["dir"] <= bound(impl, R.ORACLE_QC_DIR, R.TOL_QC_DIR)
    assert st.get("rgb", 0.0) <= bound(impl, R.ORACLE_RGB, R.TOL_RGB)
    assert st["borderline_share"] + st["unsure_share"] <= R.CAP_BORDERLINE and st["ambiguous_share"] <= R.ambiguous_cap(case["target"])
    assert st["fallback_share"] <= R.CAP_COUNT_FALLBACK and st["checked"] >= R.MIN_CHECKED
    if "half_chunks" in case:          # the ellipsoid whose normal keeps about half of every 256-cell chunk
        assert 0.4 < st["rays"] / st["cells"] < 0.6


@pytest.mark.parametrize("tgt,n0", R.ISO_TARGETS)
def test_isocell_distribution_and_rotation(impl, tgt, n0):
    d = impl.isocell_distribution(tgt, n0)
    ref = R.isocell_dirs(tgt, n0)
    assert d.shape == ref.shape
    e_dirs = float(np.abs(d - ref).max())
    nrm = R.iso_normals(40, 3)
    rot, want = impl.rotate_isocell(d, nrm), R.isocell_rotate(d, nrm)
    assert (np.isnan(rot) == np.isnan(want)).all() and np.isnan(want).any() and not np.isnan(want).all()
    e_rot = float(np.nanmax(np.abs(rot - want)))
    report(f"isocell {tgt}/{n0}", impl, dict(dirs=e_dirs, rotated=e_rot))
    assert e_dirs <= bound(impl, R.ORACLE_ISO_DIRS, R.TOL_ISO_DIRS) and e_rot <= bound(impl, R.ORACLE_ISO_ROT, R.TOL_ISO_ROT)


@pytest.mark.parametrize("case", R.ISO_CASES, ids=lambda c: c["id"])
def test_isocell_rays(impl, case):
    a = R.iso_case_arrays(case)
    coef = np.concatenate([a["f_dc"], a["f_rest"]], 1)
    got = impl.emit_isocell(a["xyz"], a["scale"], a["rot"], coef, case["deg"], a["sel"], a["normals"], a["dirs"], case["log"],
                            case.get("rgb", True), case.get("src", True))
    st = R.compare_isocell_rays(*R.iso_case_reference_args(case, a), got)
    report(case["id"], impl, st)
    assert st["ori"] <= bound(impl, R.ORACLE_ISO_ORI, R.TOL_ISO_ORI) and st["dir"] <= bound(impl, R.ORACLE_ISO_ROT, R.TOL_ISO_ROT)
    assert st.get("rgb", 0.0) <= bound(impl, R.ORACLE_RGB, R.TOL_RGB)
    assert st["checked"] >= min(R.MIN_CHECKED, case["E"] * case["K"] // 2)
