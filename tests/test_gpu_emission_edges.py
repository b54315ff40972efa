"""GPU tests of scene emission (6dgs_amd/csrc/geometry.hip) against tests/emission_reference.py (fp64, written from the mathematics)
at the shapes where its kernels change path.  Run with `-m gpu` on an MI355X; everything runs in this process.

Every case list lives in emission_reference.py and is vetted on the CPU by tests/test_emission_reference_host.py (fp32 oracle and
host instantiation of device_math.h in the kernels' place, inside every exclusion cap).  Integer results are exact; float results are
held to the TOL_* of the reference module (existing kernel-vs-oracle tolerance + measured oracle-vs-fp64 deviation).

Branch -> case (the docstrings say it again where the case is):
  grid_plan g = 64 / 128 / 256 ............. clouds of 99 999 / 100 000 and 262 145 / 1 500 000 points
  k_scan_sums' chunk loop (nb > 1024) ...... 100 000 points (nb = 2048: 2 chunks), 1 500 000 points (nb = 16 384: 16 chunks)
  k_grid_bbox' second grid stride .......... 262 145 points (one point beyond 1024 blocks x 256 threads)
  k of 1..32, cnt < k with -1 padding ...... test_knn_every_k, test_knn_tiny_clouds
  k_normals_knn's LDS tile edge ............ clouds of 1023 / 1024 / 1025 / 2049 points x 1 / 255 / 257 queries
  k_exclusive_scan's second / third chunk .. 1024 / 1025 / 2049 ellipsoids (cells), sel of length 1025 (rays)
  k_quadricell's second / third cell chunk . 20 000 / 40 000 target cells (rings of 364 / 515 cells), n_kept carried across chunks
  an ellipsoid that emits nothing in a run . needles (rings > 4096), a NaN scale, a normal with x = 0 (all cells masked)
  sel with repeats, table_res != 1000, sh_degree < 3 with a short f_rest ... RAY_CASES, TABLE_RES
  k_emit_isocell's short tail (n3) ......... K = 100, 324 and every E x K that is no multiple of 256
  K > 256, sel, scale_is_log=False, want_rgb / want_src off, degrees 0..2, the zero fill kk < n_coef ... ISO_CASES
"""
import importlib

import numpy as np
import pytest

import emission_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


def G(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def N(t):
    return None if t is None else t.detach().cpu().numpy()


def report(tag, figures):
    print(f"[emission] {tag} gpu: " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def same_bits(a, b):
    return torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.fixture(scope="module")
def fallback(oracle):
    return lambda scale_row, target, res: oracle.quadricell_centers(scale_row, target, res)[0]


# =====================================================================================================
# kNN normals
# =====================================================================================================
def assert_normal_figures(st, min_rows=R.MIN_CHECKED):
    # st["dir"] is the largest error beyond the row's eps_term (the reference solver's regulariser: see the reference module)
    assert st["dir"] <= R.TOL_NORMAL and st["sign_wrong"] == 0
    assert st["small_gap_share"] <= R.CAP_SMALL_GAP and st["dir_checked"] >= min_rows


@pytest.mark.parametrize("n", R.GRID_CLOUDS)
def test_grid_knn_at_every_grid_size(ops, n):
    """grid_plan's three grids through the cloud size: 99 999 points take g = 64, 100 000 and 262 145 take g = 128 (k_scan_sums walks 2
    chunks of 1024 block sums; at 262 145 points k_grid_bbox' grid-stride loop comes round a second time), 1 500 000 take g = 256 (16
    chunks).  The whole result equals the exhaustive search bit for bit up to 262 145 points; at 1 500 000 a fixed 2048 rows of the
    by-cell result do, and the same rows plus 512 queries outside the box through the path that is not by cell.  64 rows (both box
    corners and two coincident points among them) are judged in fp64."""
    cloud, dup = R.mixed_cloud(n, R.GRID_SEED)
    c = G(cloud)
    ng, kg = ops.normals_knn(c, c, 20, return_knn=True, method="grid")                  # query is cloud: by cell
    rng = np.random.default_rng(7)
    sub = torch.from_numpy(np.sort(rng.choice(n, 2048, replace=False))).cuda()
    if n <= 262_145:
        nb, kb = ops.normals_knn(c, c, 20, return_knn=True, method="brute")
        assert torch.equal(kb, kg) and same_bits(nb, ng)
    else:
        nb, kb = ops.normals_knn(c[sub].contiguous(), c, 20, return_knn=True, method="brute")
        assert torch.equal(kb, kg[sub]) and same_bits(nb, ng[sub])
    lo, hi = cloud.min(0), cloud.max(0)
    # queries just outside the box (2 % of its extent beyond a face): farther ones only walk more empty shells of the grid, one dependent
    # load per grid row, which at g = 256 takes seconds per query
    out = rng.uniform(-0.02, 1.02, (512, 3))
    out[np.arange(512), rng.integers(0, 3, 512)] = rng.choice([-0.02, 1.02], 512)        # at least one coordinate beyond the box
    q = torch.cat([c[sub], G(R.f32(lo + out * (hi - lo)))]).contiguous()
    nb, kb = ops.normals_knn(q, c, 20, return_knn=True, method="brute")
    nq, kq = ops.normals_knn(q, c, 20, return_knn=True, method="grid")                  # not by cell
    assert torch.equal(kb, kq) and same_bits(nb, nq)
    rows = R.knn_probe_rows(cloud, dup, 64, 1)
    rt = torch.from_numpy(rows).cuda()
    st = R.compare_knn_rows(cloud[rows], cloud, N(kg[rt]), N(ng[rt]), 20)
    report(f"grid cloud {n}", st)
    assert_normal_figures(st)


@pytest.mark.parametrize("k", R.KNN_KS)
def test_knn_every_k(ops, k):
    """k = 1, 3, 20, 32 (the kernels take 1..32; every other test uses 20) on 3000 points, both searches: lists judged in fp64 for
    every k, normals for k >= 20."""
    cloud, _ = R.mixed_cloud(3000, R.GRID_SEED + 1)
    c = G(cloud)
    nb, kb = ops.normals_knn(c, c, k, return_knn=True, method="brute")
    ng, kg = ops.normals_knn(c, c, k, return_knn=True, method="grid")
    assert torch.equal(kb, kg) and same_bits(nb, ng)
    st = R.compare_knn_rows(cloud, cloud, N(kb), N(nb), k, with_normals=k >= 20)
    report(f"k={k}", st)
    if k >= 20:
        assert_normal_figures(st)


def test_knn_k_beyond_32_is_refused(ops):
    c = G(R.mixed_cloud(100, 1)[0])
    for method in ("brute", "grid"):
        with pytest.raises(RuntimeError):
            ops.normals_knn(c, c, 33, return_knn=True, method=method)


@pytest.mark.parametrize("e", R.TINY_CLOUDS)
def test_knn_tiny_clouds(ops, e):
    """Fewer cloud points than k (the cnt < k path): the first min(k, E) entries are every point in fp64 distance order, the rest -1,
    and the grid search equals the exhaustive one."""
    cloud, _ = R.mixed_cloud(e, R.GRID_SEED + 2)
    c = G(cloud)
    nb, kb = ops.normals_knn(c, c, 20, return_knn=True, method="brute")
    ng, kg = ops.normals_knn(c, c, 20, return_knn=True, method="grid")
    assert torch.equal(kb, kg) and same_bits(nb, ng)
    knn = N(kb)
    assert R.knn_accept(cloud, cloud, knn, 20).all()
    m = min(e, 20)
    assert (knn[:, m:] == -1).all()
    if e <= 20:
        assert (np.sort(knn[:, :m], 1) == np.arange(e)[None, :]).all()


@pytest.mark.parametrize("nq", R.TILE_QUERIES)
@pytest.mark.parametrize("e", R.TILE_CLOUDS)
def test_knn_tile_edges(ops, e, nq):
    """k_normals_knn stages the cloud through LDS 1024 points at a time, 256 queries per block: clouds of 1023 / 1024 / 1025 / 2049 points
    (a tile short by one, full, one point into the next, one point into the third) and 1 / 255 / 257 queries."""
    cloud, _ = R.mixed_cloud(e, R.GRID_SEED + 3)
    q = R.tile_queries(257)[:nq]
    nb, kb = ops.normals_knn(G(q), G(cloud), 20, return_knn=True, method="brute")
    ng, kg = ops.normals_knn(G(q), G(cloud), 20, return_knn=True, method="grid")
    assert torch.equal(kb, kg) and same_bits(nb, ng)
    st = R.compare_knn_rows(q, cloud, N(kb), N(nb), 20)
    report(f"tile cloud {e} x {nq}", st)
    assert_normal_figures(st, min_rows=0 if nq == 1 else R.MIN_CHECKED)


# =====================================================================================================
# quadricell: cells
# =====================================================================================================
def assert_cell_figures(st, target):
    assert st["err"] <= R.TOL_CELLS and st["err_ambiguous"] <= R.TOL_CELLS and st["equation"] <= R.TOL_ELLIPSOID_EQ
    assert st["ambiguous_share"] <= R.ambiguous_cap(target) and st["fallback_share"] <= R.CAP_COUNT_FALLBACK


@pytest.mark.parametrize("target", R.CELL_TARGETS)
def test_quadricell_cells(ops, fallback, target):
    """17 .. 256 target cells keep every ring inside one 256-cell chunk of k_quadricell; 20 000 need a second chunk (widest ring 364
    cells), 40 000 a third (515).  Counts and ids exact, cells against fp64, every cell on its ellipsoid."""
    scale = R.cell_case_scales(target)
    pts, eid = ops.quadricell_centers(G(scale), target)
    st = R.compare_cells(scale, target, 1000, N(pts), N(eid), fallback)
    report(f"cells P={target}", st)
    assert_cell_figures(st, target)
    assert st["checked"] >= R.MIN_CHECKED


@pytest.mark.parametrize("res", R.TABLE_RES)
def test_quadricell_table_resolutions(ops, fallback, res):
    """table_res at its limits (2 and 1025 = kMaxTable + 1), at 257 and at the default."""
    scale = R.cell_case_scales(50)
    pts, eid = ops.quadricell_centers(G(scale), 50, res)
    st = R.compare_cells(scale, 50, res, N(pts), N(eid), fallback)
    report(f"cells res={res}", st)
    assert_cell_figures(st, 50)


@pytest.mark.parametrize("res", [1, 1026])
def test_quadricell_table_resolution_out_of_range_is_refused(ops, res):
    with pytest.raises(RuntimeError):
        ops.quadricell_centers(G(R.cell_case_scales(50)), 50, res)


@pytest.mark.parametrize("e", R.NEEDLE_COUNTS)
def test_quadricell_needles_and_offsets(ops, oracle, fallback, e):
    """k_exclusive_scan scans 1024 counts per chunk: 1 / 1024 / 1025 / 2049 ellipsoids.  Every 7th ellipsoid, the first and the last
    among them, is a needle (rings > 4096: no cells) and one has a NaN scale, so empty ellipsoids sit inside runs of emitting ones.
    Offsets and ids against the cumulative sum of the oracle's counts; the cells of 64 sampled ellipsoids against fp64."""
    scale, needle = R.needle_case_scales(e)
    pts, eid = ops.quadricell_centers(G(scale), 17)
    counts = R.oracle_cell_counts(oracle, scale, 17)
    eid = N(eid)
    assert (counts[needle] == 0).all() and eid.shape[0] == counts.sum()
    assert (eid == np.repeat(np.arange(e), counts)).all()            # = searchsorted of the cumulative sum: offsets and ids
    st = R.compare_cells(scale, 17, 1000, N(pts), eid, fallback, only=R.sampled_ellipsoids(e, needle))
    report(f"needles E={e}", st)
    assert_cell_figures(st, 17)


# =====================================================================================================
# quadricell: rays
# =====================================================================================================
@pytest.mark.parametrize("case", R.RAY_CASES, ids=lambda c: c["id"])
def test_quadricell_rays(ops, fallback, case):
    """emit_quadricell on the cell sets above: n_cells, the ray count (fp64's outside the borderline cells), src and order, origins,
    directions, and the colour against sh_colour on the emitted directions.  Across the cases: sel as a permutation with repeats and
    one of length 1025 into 64 ellipsoids (k_exclusive_scan's second chunk on ray counts), both scale_is_log, want_rgb off (with a
    degree the absent coefficients could not serve), degrees 0..3 with f_rest of exactly (d+1)^2 - 1 coefficients ([E, 0, 3] at degree
    0) and of 15, table_res 257, one ellipsoid whose normal has x = 0 (all cells masked) in every set, and at 40 000 target cells an
    ellipsoid whose normal keeps about half of every 256-cell chunk (n_kept carried from chunk to chunk)."""
    a = R.ray_case_arrays(case)
    got = ops.emit_quadricell(G(a["xyz"]), G(a["scale"]), G(a["rot"]), G(a["f_dc"]), G(a["f_rest"]), case["deg"], G(a["sel"]), G(a["normals"]),
                              case["target"], case.get("res", 1000), scale_is_log=case["log"], want_rgb=case.get("rgb", True))
    assert (got[2] is None) == (not case.get("rgb", True))
    st = R.compare_quadricell_rays(*R.ray_case_reference_args(case, a), tuple(N(t) for t in got[:4]) + (got[4],), fallback)
    report(case["id"], st)
    assert st["ori"] <= R.TOL_QC_ORI and st["dir"] <= R.TOL_QC_DIR and st.get("rgb", 0.0) <= R.TOL_RGB
    assert st["borderline_share"] + st["unsure_share"] <= R.CAP_BORDERLINE and st["ambiguous_share"] <= R.ambiguous_cap(case["target"])
    assert st["fallback_share"] <= R.CAP_COUNT_FALLBACK and st["checked"] >= R.MIN_CHECKED
    if "half_chunks" in case:
        assert 0.4 < st["rays"] / st["cells"] < 0.6


# =====================================================================================================
# iso-cell
# =====================================================================================================
@pytest.mark.parametrize("tgt,n0", R.ISO_TARGETS)
def test_isocell_distribution_and_rotation(ops, tgt, n0):
    """Targets 1, 35 (n0 = 3), 100, 300; normals in general position, exactly +-z (unit or not: the NaN pattern must be identical) and
    at polar angles 1e-3, 1e-2, 1e-1 from +z and -z."""
    d = ops.isocell_distribution(tgt, n0)
    ref = R.isocell_dirs(tgt, n0)
    assert tuple(d.shape) == ref.shape
    e_dirs = float(np.abs(N(d) - ref).max())
    nrm = R.iso_normals(40, 3)
    rot, want = N(ops.rotate_isocell(d, G(nrm))), R.isocell_rotate(N(d), nrm)
    assert (np.isnan(rot) == np.isnan(want)).all() and np.isnan(want).any()
    e_rot = float(np.nanmax(np.abs(rot - want)))
    report(f"isocell {tgt}/{n0}", dict(dirs=e_dirs, rotated=e_rot))
    assert e_dirs <= R.TOL_ISO_DIRS and e_rot <= R.TOL_ISO_ROT


GUARD = 64


def emit_isocell_guarded(ops, a, case):
    """ops.emit_isocell's call into the library with output buffers of our own: every one is followed by GUARD sentinel elements, which
    must come back untouched.  Returns (ori, dir, rgb, src) as ops.emit_isocell does."""
    lib = importlib.import_module("6dgs_amd._lib").load()
    t = {k: G(v) for k, v in a.items()}
    e = a["normals"].shape[0]
    k = a["dirs"].shape[0]
    want_rgb, want_src = case.get("rgb", True), case.get("src", True)
    buf = {name: torch.full((e * k * 3 + GUARD,), 12345.0, device="cuda") for name in ("ori", "dir", "rgb")}
    src = torch.full((e * k + GUARD,), -7, dtype=torch.int64, device="cuda")
    p = ops._p
    ops.check(lib.sixdgs_emit_isocell(p(t["xyz"]), p(t["scale"]), int(case["log"]), p(t["rot"]), p(t["f_dc"] if want_rgb else None),
                                      p(t["f_rest"] if want_rgb else None), case["deg"] if want_rgb else 0, a["f_rest"].shape[1] + 1 if want_rgb else 1,
                                      p(t["sel"]), e, p(t["normals"]), p(t["dirs"]), k, p(buf["ori"]), p(buf["dir"]),
                                      p(buf["rgb"] if want_rgb else None), p(src if want_src else None), ops._stream()), "emit_isocell")
    torch.cuda.synchronize()
    for name, b in buf.items():
        assert (b[e * k * 3:] == 12345.0).all(), f"guard band after {name}"
    assert (src[e * k:] == -7).all(), "guard band after src"
    assert want_rgb or (buf["rgb"] == 12345.0).all()
    assert want_src or (src == -7).all()
    return (buf["ori"][:e * k * 3].reshape(-1, 3), buf["dir"][:e * k * 3].reshape(-1, 3),
            buf["rgb"][:e * k * 3].reshape(-1, 3) if want_rgb else None, src[:e * k] if want_src else None)


@pytest.mark.parametrize("case", R.ISO_CASES, ids=lambda c: c["id"])
def test_isocell_rays(ops, case):
    """emit_isocell for E in 1, 15, 16, 17, 33 (16 ellipsoids per block: one short block, one full, one ellipsoid into the next, a third
    block) x K in 1, 48, 100, 324 (256 rays staged at a time: K = 100 and 324 leave short tails stored through n3, K = 324 spreads one
    ellipsoid over two chunks).  Across the cases: sel with repeats into a larger scene, both scale_is_log, want_rgb and want_src off,
    degrees 0..3 with f_rest of (d+1)^2 - 1 coefficients (the zero fill kk < n_coef) and of 15, normals exactly +-z.  Every output
    element against fp64; a guard band after each output buffer must stay untouched."""
    a = R.iso_case_arrays(case)
    got = emit_isocell_guarded(ops, a, case)
    via = ops.emit_isocell(G(a["xyz"]), G(a["scale"]), G(a["rot"]), G(a["f_dc"]), G(a["f_rest"]), case["deg"], G(a["sel"]), G(a["normals"]),
                           G(a["dirs"]), scale_is_log=case["log"], want_rgb=case.get("rgb", True), want_src=case.get("src", True))
    for x, y in zip(got, via):
        assert (x is None) == (y is None) and (x is None or (same_bits(x, y) if x.is_floating_point() else torch.equal(x, y)))
    st = R.compare_isocell_rays(*R.iso_case_reference_args(case, a), tuple(N(t) for t in got))
    report(case["id"], st)
    assert st["ori"] <= R.TOL_ISO_ORI and st["dir"] <= R.TOL_ISO_ROT and st.get("rgb", 0.0) <= R.TOL_RGB
    assert st["checked"] >= min(R.MIN_CHECKED, case["E"] * case["K"] // 2)
