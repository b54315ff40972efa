"""Starting a scene from a point cloud, without a GPU: the three restatements of sixdgs_knn_mean_dist2 against each other
(tests/knn_reference.py); csrc/knn_rules.h -- the pair and box rules the kernels of knn.hip run -- through its host instantiation
(libsixdgs_hostcheck.so): Morton cells, the box distance as a lower bound IN fp32, and the whole boxed search bit for bit against the
brute force on every cloud of the table; what the two entry points answer and refuse without a device; the point-cloud readers against
the reference's (golden g16) and a PLY round trip; GaussianScene.from_points against the reference's numbers and an fp64 restatement."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as K  # noqa: E402

torch = pytest.importorskip("torch")

F = np.float32
BADARG, WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())
    lib.hc_knn_boxed.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_points")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def boxed(hc, p, box=None):
    p = np.ascontiguousarray(p, F)
    out, visited = np.full(p.shape[0], np.nan, F), np.zeros(p.shape[0], np.int32)
    assert hc.hc_knn_boxed(C.c_longlong(p.shape[0]), _ptr(p), int(box or hc.hc_knn_box()), _ptr(out), _ptr(visited)) == 0
    return out, visited


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("uniform1025", "clustered", "offset", "anisotropic", "line"))
def test_brute_np_is_within_its_derived_bound_of_fp64(name):
    p, got = K.case(name)
    want = K.brute_f64(p)
    ratio = float((np.abs(got.astype(np.float64) - want) / np.maximum(K.REL_MEAN * want, 1e-300)).max())
    print(f"{name}: max |fp32 - fp64| / (9 u mean) = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", ("uniform257", "clustered", "duplicated", "lattice"))
def test_brute_torch_on_cpu_is_bit_equal_to_brute_np(name):
    p, want = K.case(name)
    got = K.brute_torch(torch.from_numpy(np.array(p)), chunk=200)
    assert got.dtype == F and np.array_equal(bits(got), bits(want))


def test_lattice_and_duplicates_have_their_exact_results():
    assert np.all(K.case("lattice")[1] == F(1.0))
    assert np.all(K.case("duplicated")[1] == F(0.0)) and np.all(K.case("identical600")[1] == F(0.0))


# ---- knn_rules.h ----------------------------------------------------------------------------------------------------------------
def test_morton_cells_clamp_and_are_zero_on_a_flat_axis(hc):
    rng = np.random.default_rng(0)
    lo, hi = np.array([-1.0, 2.0, 5.0], F), np.array([3.0, 2.0, 5.5], F)              # y is flat
    p = (rng.random((4000, 3)) * 8 - 3).astype(F)                                       # many points outside the box
    p[:8] = [[-1, 2, 5], [3, 2, 5.5], [1e30, 2, -1e30], [-1e30, 2, 1e30], [np.nan, 2, 5.25], [3, 7, 5.5], [np.inf, 2, -np.inf], [1, 2, 5.25]]
    code, cells = np.zeros(4000, np.uint32), np.zeros((4000, 3), np.uint32)
    hc.hc_knn_morton(C.c_longlong(4000), _ptr(p), _ptr(lo), _ptr(hi), _ptr(code), _ptr(cells))
    assert cells.max() == 1023 and np.all(cells[:, 1] == 0)
    assert tuple(cells[0]) == (0, 0, 0) and tuple(cells[1]) == (1023, 0, 1023) and tuple(cells[2]) == (1023, 0, 0)
    assert tuple(cells[3]) == (0, 0, 1023) and cells[4, 0] == 0 and tuple(cells[6]) == (1023, 0, 0)
    inside = np.all((p >= lo) & (p <= hi), axis=1)
    t = (p[inside][:, [0, 2]] - lo[[0, 2]]) / (hi[[0, 2]] - lo[[0, 2]]) * F(1023.0)
    assert t.dtype == F and np.array_equal(cells[inside][:, [0, 2]], np.minimum(t.astype(np.uint32), 1023))

    def spread(v):
        return sum(((v >> b) & 1) << (3 * b) for b in range(10))
    c64 = cells.astype(np.uint64)
    assert np.array_equal(code.astype(np.uint64), (spread(c64[:, 0]) << 2) | (spread(c64[:, 1]) << 1) | spread(c64[:, 2]))
    assert code.max() < 2 ** 30


def test_box_distance_is_a_lower_bound_of_d2_in_fp32(hc):
    """box_d2(q, box) <= d2(q, p) for every p of the box, compared as fp32 numbers: random boxes at several magnitudes and offsets,
    queries anywhere, and queries exactly on a face, an edge or a corner; p includes the box's own corners."""
    rng = np.random.default_rng(1)
    m = 60000
    scale = F(10.0) ** rng.integers(-3, 5, (m, 1)).astype(F)
    centre = (rng.normal(0, 1, (m, 3)) * rng.choice([0.0, 1.0, 4096.0], (m, 1))).astype(F)
    a, b = (centre + scale * rng.normal(0, 1, (m, 3))).astype(F), (centre + scale * rng.normal(0, 1, (m, 3))).astype(F)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    hi[::7, 1] = lo[::7, 1]                                                               # flat boxes
    p = (lo + (hi - lo) * rng.random((m, 3)).astype(F)).astype(F)
    p = np.clip(p, lo, hi)
    corner = rng.random((m, 3)) < 0.5
    p[::3] = np.where(corner[::3], lo[::3], hi[::3])                                       # the box's own corners
    q = (centre + F(3.0) * scale * rng.normal(0, 1, (m, 3))).astype(F)
    on = rng.integers(0, 3, (m, 3))                                                        # per axis: free, on lo, on hi
    q[::2] = np.where(on[::2] == 1, lo[::2], np.where(on[::2] == 2, hi[::2], q[::2]))      # faces, edges, corners
    lo, hi, p, q = (np.ascontiguousarray(v, F) for v in (lo, hi, p, q))
    box, pair = np.zeros(m, F), np.zeros(m, F)
    hc.hc_knn_box_d2(C.c_longlong(m), _ptr(q), _ptr(lo), _ptr(hi), _ptr(box))
    hc.hc_knn_pair_d2(C.c_longlong(m), _ptr(q), _ptr(p), _ptr(pair))
    d = p - q
    assert np.array_equal(bits(pair), bits((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    assert np.all(box <= pair), int((box > pair).sum())
    inside = np.all((q >= lo) & (q <= hi), axis=1)
    assert inside.sum() > 100 and np.all(box[inside] == 0)
    # a box of queries against a box: below the box distance of every query inside it
    qa, qb = np.minimum(q, p), np.maximum(q, p)
    lo2, hi2 = np.roll(lo, 1, axis=0), np.roll(hi, 1, axis=0)
    bb, b1, b2 = np.zeros(m, F), np.zeros(m, F), np.zeros(m, F)
    hc.hc_knn_box_box_d2(C.c_longlong(m), _ptr(qa), _ptr(qb), _ptr(lo2), _ptr(hi2), _ptr(bb))
    hc.hc_knn_box_d2(C.c_longlong(m), _ptr(q), _ptr(lo2), _ptr(hi2), _ptr(b1))
    hc.hc_knn_box_d2(C.c_longlong(m), _ptr(p), _ptr(lo2), _ptr(hi2), _ptr(b2))
    assert np.all(bb <= b1) and np.all(bb <= b2)


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_boxed_search_on_the_host_is_bit_equal_to_brute_force(hc, name):
    p, want = K.case(name)
    got, visited = boxed(hc, p)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    print(f"{name}: n {p.shape[0]}, boxes walked per query: mean {visited.mean():.2f}, max {visited.max()}")
    if name.startswith("identical"):
        assert visited.max() <= 2            # >= prunes every other box once three zeros are held (two only for a short last box)


@pytest.mark.parametrize("box", (1, 3, 7, 64))
def test_boxed_search_with_other_box_sizes(hc, box):
    for name in ("uniform513", "clustered", "duplicated"):
        p, want = K.case(name)
        assert np.array_equal(bits(boxed(hc, p, box)[0]), bits(want)), (name, box)


def test_boxed_search_refuses_fewer_than_four_points(hc):
    p, out = np.zeros((3, 3), F), np.zeros(3, F)
    assert hc.hc_knn_boxed(C.c_longlong(3), _ptr(p), 256, _ptr(out), None) == -1


# ---- the entry points without a device -----------------------------------------------------------------------------------------
def test_entry_points_answer_argument_errors_without_a_gpu():
    lib = importlib.import_module("6dgs_amd._lib").load()
    ws_bytes = lib.sixdgs_knn_workspace_bytes
    assert [ws_bytes(n) for n in (-1, 0, 1, 2, 3, 2 ** 31, 2 ** 40)] == [0] * 7
    assert 0 < ws_bytes(4) <= ws_bytes(257) < ws_bytes(500000) < 2 ** 26
    call = lib.sixdgs_knn_mean_dist2
    xyz, out, ws = 0x10000, 0x90000000, 0x40000000                      # never dereferenced: every case is refused on the host
    need = ws_bytes(1000)
    assert call(0, None, None, None, 0, None) == 0
    for n in (1, 2, 3, -5, 2 ** 31):
        assert call(n, xyz, out, ws, 2 ** 40, None) == BADARG
    assert call(1000, None, out, ws, need, None) == BADARG and call(1000, xyz, None, ws, need, None) == BADARG
    assert call(1000, xyz + 2, out, ws, need, None) == BADARG and call(1000, xyz, out + 1, ws, need, None) == BADARG
    assert call(1000, xyz, xyz, ws, need, None) == BADARG and call(1000, xyz, xyz + 11996, ws, need, None) == BADARG
    assert call(1000, xyz + 3996, xyz, ws, need, None) == BADARG
    assert call(1000, xyz, out, ws, need - 1, None) == WORKSPACE and call(1000, xyz, out, ws, 0, None) == WORKSPACE
    assert call(1000, xyz, out, None, need, None) == BADARG and call(1000, xyz, out, ws + 128, need, None) == BADARG


def test_wrapper_validates_before_the_library():
    ops = importlib.import_module("6dgs_amd.ops")
    for bad in (torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(3, 5).t(), torch.zeros(15)):
        with pytest.raises(ValueError):
            ops.knn_mean_dist2(bad)
    with pytest.raises(ValueError):
        ops.knn_mean_dist2(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.knn_mean_dist2(torch.zeros(5, 3))                               # no CPU fallback on the product path


# ---- readers ----------------------------------------------------------------------------------------------------------------
def test_points3d_readers_match_the_reference(tmp_path, g16):
    D = importlib.import_module("6dgs_amd.datasets")
    (tmp_path / "points3D.bin").write_bytes(g16["points3d_bin"].tobytes())
    (tmp_path / "points3D.txt").write_bytes(g16["points3d_txt"].tobytes())
    for got, kind in ((D.read_points3D_binary(str(tmp_path / "points3D.bin")), "bin"), (D.read_points3D_text(str(tmp_path / "points3D.txt")), "txt")):
        for a, k in zip(got, ("xyz", "rgb", "err")):
            want = g16[f"{kind}_{k}"]
            assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want), (kind, k)
    assert g16["bin_xyz"].shape == (50, 3)


def test_ply_round_trip_and_fallback_order(tmp_path, g16):
    D = importlib.import_module("6dgs_amd.datasets")
    sparse = tmp_path / "sparse" / "0"
    sparse.mkdir(parents=True)
    xyz, rgb = g16["bin_xyz"], g16["bin_rgb"]
    (sparse / "points3D.txt").write_bytes(g16["points3d_txt"].tobytes())
    pcd = D.read_point_cloud(str(tmp_path))                                  # .txt only
    assert isinstance(pcd, D.BasicPointCloud) and np.array_equal(pcd.points, xyz) and np.array_equal(pcd.colors, rgb / 255.0)
    assert pcd.normals.shape == (50, 3) and not pcd.normals.any()
    (sparse / "points3D.bin").write_bytes(g16["points3d_bin"].tobytes()[:-3] )
    assert np.array_equal(D.read_point_cloud(str(tmp_path)).points, xyz)     # a broken .bin falls back to .txt, as the reference does
    (sparse / "points3D.bin").write_bytes(g16["points3d_bin"].tobytes())
    (sparse / "points3D.txt").write_text("# empty\n")
    assert np.array_equal(D.read_point_cloud(str(tmp_path)).points, xyz)     # .bin before .txt
    D.store_ply(str(sparse / "points3D.ply"), xyz[:20] + 1.0, rgb[:20])
    pcd = D.read_point_cloud(str(tmp_path))                                  # .ply first
    assert pcd.points.shape == (20, 3) and pcd.points.dtype == F and np.array_equal(pcd.points, (xyz[:20] + 1.0).astype(F))
    assert np.array_equal(pcd.colors, rgb[:20] / 255.0) and 0.0 <= pcd.colors.min() and pcd.colors.max() <= 1.0
    assert pcd.normals.shape == (20, 3) and not pcd.normals.any()
    head = (sparse / "points3D.ply").read_bytes().split(b"end_header\n")[0].decode()
    assert head.split("\n")[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 20"]
    assert [ln.split()[1:] for ln in head.split("\n")[3:12]] == [["float", k] for k in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", k] for k in ("red", "green", "blue")]
    # ascii and big-endian files of the same content, property order changed
    v = np.zeros(20, dtype=[("red", "u1"), ("green", "u1"), ("blue", "u1"), ("x", ">f8"), ("y", ">f8"), ("z", ">f8")])
    for a, k in enumerate(("x", "y", "z")):
        v[k] = pcd.points[:, a]
    for a, k in enumerate(("red", "green", "blue")):
        v[k] = rgb[:20, a]
    hdr = "ply\nformat {} 1.0\ncomment other order\nelement vertex 20\n" + "".join(f"property uchar {k}\n" for k in ("red", "green", "blue")) \
        + "".join(f"property double {k}\n" for k in ("x", "y", "z")) + "element face 0\nproperty list uchar int vertex_indices\nend_header\n"
    (tmp_path / "be.ply").write_bytes(hdr.format("binary_big_endian").encode() + v.tobytes())
    (tmp_path / "as.ply").write_text(hdr.format("ascii") + "".join(" ".join(repr(x.item()) for x in row) + "\n" for row in v))
    for name in ("be.ply", "as.ply"):
        other = D.fetch_ply(str(tmp_path / name))
        assert np.array_equal(other.points, pcd.points) and np.array_equal(other.colors, pcd.colors) and not other.normals.any()
    (tmp_path / "bad.ply").write_bytes(b"plx\n")
    with pytest.raises(RuntimeError):
        D.fetch_ply(str(tmp_path / "bad.ply"))


# ---- GaussianScene.from_points ----------------------------------------------------------------------------------------------
def test_from_points_matches_the_reference_numbers(g16):
    pkg = importlib.import_module("6dgs_amd")
    rgb = g16["rgb"]
    n = rgb.shape[0]
    rng = np.random.default_rng(3)
    points = rng.normal(0, 2, (n, 3)).astype(F)
    d2 = (F(10.0) ** rng.uniform(-9, 4, n)).astype(F)                       # both sides of the 1e-7 floor
    d2[:3] = [0.0, 1e-7, 1.0]
    scene = pkg.GaussianScene.from_points(points, rgb, mean_dist2=d2, device="cpu")
    got, want = K.check_from_points(scene, points, rgb, d2)
    assert np.array_equal(bits(got["f_dc"][:, 0, :]), bits(g16["sh"]))                  # the reference's RGB2SH, to the bit
    assert np.array_equal(bits(got["opacity"][:7]), bits(g16["logit_init"])) and np.all(got["opacity"] == got["opacity"][0])
    assert got["scale"][0, 0] == got["scale"][1, 0] and got["scale"][2, 0] == 0          # the floor; log(sqrt(1)) is exact
    # against fp64: the subtraction, the constant rounded to fp32 and the division, one rounding each
    assert np.abs(got["f_dc"].astype(np.float64) - want["f_dc"]).max() <= 3 * K.U * np.abs(want["f_dc"]).max()
    for k, p in enumerate(g16["prob"]):
        s = pkg.GaussianScene.from_points(points[:4], rgb[:4], 1, opacity=float(p), mean_dist2=d2[:4], device="cpu")
        assert abs(float(s._opacity[0, 0]) - float(g16["logit"][k])) <= 4 * K.U * max(1.0, abs(float(g16["logit"][k])))
        assert s._features_rest.shape == (4, 3, 3) and s.max_sh_degree == 1
    # a caller's own arrays are not aliased, integer colours and float64 points are accepted
    s = pkg.GaussianScene.from_points(points.astype(np.float64), rgb, 0, mean_dist2=torch.from_numpy(d2), device="cpu")
    assert s._features_rest.shape == (n, 0, 3) and np.array_equal(s._xyz.numpy(), points)


def test_create_from_pcd_keeps_the_reference_name_and_lr_scale(g16):
    pkg = importlib.import_module("6dgs_amd")
    D = importlib.import_module("6dgs_amd.datasets")
    pcd = D.BasicPointCloud(points=g16["bin_xyz"], colors=g16["bin_rgb"] / 255.0, normals=np.zeros((50, 3)))
    with pytest.raises(RuntimeError, match="GPU"):                           # the search itself has no CPU path
        pkg.GaussianScene(2).create_from_pcd(pcd, 3.5, device="cpu")
    assert hasattr(pkg.GaussianModel, "create_from_pcd")


def test_from_points_refuses_bad_input():
    pkg = importlib.import_module("6dgs_amd")
    p, c, d = np.zeros((5, 3), F), np.zeros((5, 3), F), np.ones(5, F)
    fp = pkg.GaussianScene.from_points
    for bad in (dict(points=p[:3], colors=c[:3], mean_dist2=d[:3]), dict(points=p, colors=c[:4], mean_dist2=d), dict(points=p[:, :2], colors=c[:, :2], mean_dist2=d),
                dict(points=p, colors=c, mean_dist2=d[:4]), dict(points=p, colors=c, mean_dist2=d, sh_degree=4),
                dict(points=p, colors=c, mean_dist2=d, opacity=1.0), dict(points=p, colors=c, mean_dist2=d, min_dist2=0.0)):
        with pytest.raises(ValueError):
            fp(device="cpu", **bad)
    for v in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[2, 1] = v
        with pytest.raises(ValueError, match="finite"):
            fp(q, c, mean_dist2=d, device="cpu")
