"""The consensus pose solver (sixdgs_solve_pose_consensus, added under ABI 10) without a GPU: the entry points in the header, the
binding and the library; argument errors answered without touching the GPU; the refusals of ops.solve_pose_consensus and of the
host layers above it; and the fp64 restatement of the estimator (tests/pose_consensus_reference.py) on planted scenes -- which pins
the estimator independently of the kernel: camera on the radius-4 sphere, origins uniform in [-1, 1]^3, 0.003 of direction noise on the
inliers, outliers aimed at random points of that sphere; seeds 0-11, k in {100, 256}, inlier fractions 0.5 / 0.3 / 0.2, tau = 0.05,
uniform prior: centre within 0.06 of the planted camera at every seed."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_consensus_reference as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_solve_pose_consensus", "sixdgs_solve_pose_consensus_workspace_bytes")


def test_entry_points_in_header_binding_and_library_abi_still_10():
    ge = importlib.import_module("__graft_entry__")
    lib = importlib.import_module("6dgs_amd._lib")
    text = open(os.path.join(ROOT, "include", "sixdgs.h")).read()
    assert "added under ABI 10, additive" in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert ge.header_abi_version() == 10 == lib.ABI_VERSION
    assert len(lib.SIGNATURES["sixdgs_solve_pose_consensus"][1]) == 24
    assert "pose_consensus.hip" in importlib.import_module("6dgs_amd.build").SOURCES
    if not os.path.exists(lib.LIB_PATH):
        return
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(so, name), f"{name} is not exported by the library"
    L = lib.load()
    assert L.sixdgs_abi_version() == 10
    ws = L.sixdgs_solve_pose_consensus_workspace_bytes
    # one (support, pair) per block of 256 hypotheses and image: 8 bytes each
    assert ws(8, 256) >= 8 * 128 * 8 and ws(8, 1024) >= 8 * 128 * 8 and ws(8, 100) >= 8 * 20 * 8 and ws(1, 2) >= 8
    assert ws(16, 256) >= ws(8, 256) and ws(0, 100) == 0
    assert ws(8, 1) == 0 and ws(8, 1025) == 0 and ws(-1, 100) == 0

    def call(k=100, batch=1, tau=0.05, prior=0, ws_bytes=1 << 20):
        n = None
        return L.sixdgs_solve_pose_consensus(n, n, 10, n, n, k, n, n, batch, tau, prior, n, n, n, n, n, n, n, n, n, n, n, ws_bytes, n)

    # argument errors are answered without touching the GPU (every pointer is NULL here)
    assert call(k=1) == -1 and call(k=1025) == -1 and call(k=0) == -1
    assert call(tau=0.0) == -1 and call(tau=-1.0) == -1 and call(tau=float("nan")) == -1 and call(tau=1e-30) == -1
    assert call(prior=2) == -1 and call(prior=-1) == -1
    assert call(ws_bytes=0) == -1 and call(k=256, batch=8, ws_bytes=ws(8, 256) - 1) == -1      # a short workspace
    assert call(batch=-1) == -1
    assert call() == -1                               # NULL operands
    assert call(batch=0, ws_bytes=0) == 0             # no images: nothing to do


def _operands(b=2, k=10, r=50):
    g = torch.Generator().manual_seed(0)
    ori, dr = torch.rand(r, 3, generator=g), torch.nn.functional.normalize(torch.randn(r, 3, generator=g), dim=1)
    idx = torch.randint(0, r, (b, k), generator=g)
    return ori, dr, idx, torch.rand(b, k, generator=g), torch.tensor([[0.0, 1.0, 0.0]] * b)


def test_solve_pose_consensus_validates_before_it_marshals():
    ops = importlib.import_module("6dgs_amd.ops")
    ori, dr, idx, val, up = _operands()
    f = ops.solve_pose_consensus
    with pytest.raises(TypeError):
        f(ori, dr, idx, val, up)                                        # inlier_scale is required
    with pytest.raises(RuntimeError):
        f(ori, dr, idx, val, up, inlier_scale=0.05)                     # CPU tensors: no CPU fallback
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f(ori, dr, idx, val, up, inlier_scale=tau)
    with pytest.raises(ValueError):
        f(ori, dr, idx, val, up, inlier_scale=0.05, prior="softmax")
    bad = [
        dict(rays_ori=ori[:, :2]), dict(rays_dir=dr[:10]), dict(rays_ori=ori.reshape(-1)),        # rays not [R,3] twice
        dict(val=val[:, :5]), dict(idx=idx[0]), dict(val=val[:1]),                                  # idx / val not the same [B,k]
        dict(up=up[:1]), dict(up=up[:, :2]), dict(up=up.reshape(-1)),                              # up not [B,3]
        dict(gt_c2w=torch.eye(4)), dict(gt_c2w=torch.eye(4)[None]), dict(gt_c2w=torch.zeros(2, 3, 4)),
        dict(idx=idx[:, :1], val=val[:, :1]),                                                      # k < 2
        dict(idx=torch.zeros(1, 1025, dtype=torch.int64), val=torch.zeros(1, 1025), up=up[:1]),    # k > 1024
    ]
    for kw in bad:
        args = dict(rays_ori=ori, rays_dir=dr, idx=idx, val=val, up=up, gt_c2w=None)
        args.update(kw)
        with pytest.raises(ValueError):
            f(args["rays_ori"], args["rays_dir"], args["idx"], args["val"], args["up"], args["gt_c2w"], inlier_scale=0.05)
    for kw in (dict(idx=idx.float()), dict(val=val.long()), dict(up=up.long()), dict(rays_ori=ori.long()), dict(gt_c2w=torch.zeros(2, 4, 4).long()),
               dict(idx=idx.tolist())):
        args = dict(rays_ori=ori, rays_dir=dr, idx=idx, val=val, up=up, gt_c2w=None)
        args.update(kw)
        with pytest.raises(TypeError):
            f(args["rays_ori"], args["rays_dir"], args["idx"], args["val"], args["up"], args["gt_c2w"], inlier_scale=0.05)


def test_solve_pose_names_its_limit():
    """ops.solve_pose depended on k <= 256 silently (the library answered 'bad argument'); now it says so and points at the consensus solver."""
    ops = importlib.import_module("6dgs_amd.ops")
    ori, dr, _, _, up = _operands(b=1)
    with pytest.raises(ValueError, match="solve_pose_consensus"):
        ops.solve_pose(ori, dr, torch.zeros(1, 257, dtype=torch.int64), torch.zeros(1, 257), up)
    with pytest.raises(RuntimeError):                                   # a valid k still reaches the GPU check
        ops.solve_pose(ori, dr, torch.zeros(1, 256, dtype=torch.int64), torch.zeros(1, 256), up)
    assert ops.SOLVE_POSE_MAX_K == 256 and ops.CONSENSUS_MAX_K == 1024 and "consensus" in ops.solve_pose.__doc__


def test_host_layers_carry_the_solver_choice():
    T = importlib.import_module("6dgs_amd.test")
    for fn in (T.estimate_poses, T._solve_batch, T.test_pose_estimation, T.PoseStream.__init__):
        ps = inspect.signature(fn).parameters
        for name, default in (("pose_solver", "ls"), ("inlier_scale", None), ("pose_prior", "uniform")):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default == default, (fn, name)
    ps = inspect.signature(T.resolve_poses).parameters
    assert all(ps[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("pose_solver", "inlier_scale", "pose_prior"))
    for bad in (dict(pose_solver="ransac"), dict(pose_prior="softmax")):
        with pytest.raises(ValueError):
            T.estimate_poses(None, None, None, None, None, **bad)
        with pytest.raises(ValueError):
            T.PoseStream(None, None, None, None, **bad)
        with pytest.raises(ValueError):
            T.test_pose_estimation([], None, torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.tensor([0.0, 1.0, 0.0]), verbose=False, **bad)


def test_default_inlier_scale_is_cached_per_ray_tensor():
    T = importlib.import_module("6dgs_amd.test")
    mod = torch.nn.Identity()
    rays = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 12.0], [1.0, 1.0, 1.0]])
    assert T.default_inlier_scale(mod, rays) == pytest.approx(0.13)
    held = mod.__dict__["_inlier_scale_cache"]
    assert T.default_inlier_scale(mod, rays) == held[2] and mod.__dict__["_inlier_scale_cache"] is held       # not recomputed
    rays.mul_(2.0)                                                      # an in-place change is seen (version counter)
    assert T.default_inlier_scale(mod, rays) == pytest.approx(0.26)
    assert T.default_inlier_scale(mod, rays.clone() * 0.5) == pytest.approx(0.13)


def test_evaluation_sweep_flags():
    m = importlib.import_module("6dgs_amd.pretrain_eval_attention")
    base = ["--exp_path", "x", "--out_path", "y"]
    a, _ = m.parse_args(base)
    assert (a.pose_solver, a.inlier_scale, a.rays_to_output) == ("ls", None, 100)
    a, _ = m.parse_args(base + ["--pose_solver", "consensus", "--inlier_scale", "0.02", "--rays_to_output", "5000"])
    assert (a.pose_solver, a.inlier_scale, a.rays_to_output) == ("consensus", 0.02, 1024)
    for bad in (["--pose_solver", "ls", "--rays_to_output", "300"], ["--pose_solver", "consensus", "--inlier_scale", "0"], ["--rays_to_output", "0"]):
        with pytest.raises(SystemExit):
            m.parse_args(base + bad)


def test_hypothesis_sets():
    i, j = PR.hypothesis_pairs(100)
    assert len(i) == 4950 and (i < j).all()
    i, j = PR.hypothesis_pairs(256)
    assert len(i) == 32640
    i, j = PR.hypothesis_pairs(1024)
    assert len(i) == 32768 and (((j - i) % 1024) <= 32).all() and (((j - i) % 1024) >= 1).all()
    assert i[0] == 0 and j[0] == 1 and np.array_equal(np.lexsort((j, i)), np.arange(len(i)))
    assert (i[i == 1023] == 1023).sum() == 32 and set(j[i == 1023].tolist()) == set(range(32))     # the wrap
    i, j = PR.hypothesis_pairs(300)
    assert len(i) == 300 * 109 and len(set(zip(np.minimum(i, j).tolist(), np.maximum(i, j).tolist()))) == len(i)      # no pair twice


@pytest.mark.parametrize("k", PR.KS)
@pytest.mark.parametrize("fraction", PR.INLIER_FRACTIONS)
def test_reference_recovers_the_planted_camera(k, fraction):
    worst, ls_best, gaps = 0.0, float("inf"), []
    for seed in PR.SEEDS:
        cam, o, d, inlier = PR.planted_scene(seed, k, fraction)
        out = PR.consensus(o, d, np.arange(k), np.ones(k), PR.TAU)
        err = float(np.linalg.norm(out["centre"] - cam))
        ls = float(np.linalg.norm(PR.least_squares_centre(o, d)[0] - cam))
        print(f"k={k} inliers={fraction} seed={seed}: centre error {err:.4f} (least squares {ls:.3f}), support {out['support']:.3f}, "
              f"n_inliers {out['n_inliers']} of {int(inlier.sum())} planted, gap {out['gap']:.2e}")
        worst, ls_best = max(worst, err), min(ls_best, ls)
        gaps.append(out["gap"])
        assert out["status"] == 0 and out["winner"][0] < out["winner"][1]
        assert abs(out["w_final"].sum() - 1) < 1e-12 and 0 <= out["support"] <= 1
        assert err <= PR.CENTRE_BOUND, (seed, err)
        assert ls > 1.0, (seed, ls)                  # what the plain least-squares centre does with the same rays
    print(f"k={k} inliers={fraction}: worst centre error {worst:.4f}, best least-squares error {ls_best:.3f}, smallest gap {min(gaps):.2e}")


def test_reference_edge_cases():
    cam, o, d, _ = PR.planted_scene(3, 40, 0.5)
    full = PR.consensus(o, d, np.arange(40), np.ones(40), PR.TAU)
    # padding entries neither vote nor form hypotheses: the same answer as the short list
    idx = np.concatenate([np.arange(30), [-1] * 6, [40, 10 ** 6, -5, 99]])
    a = PR.consensus(o, d, idx, np.ones(40), PR.TAU)
    b = PR.consensus(o, d, np.arange(30), np.ones(30), PR.TAU)
    assert a["n"] == 30 and np.allclose(a["centre"], b["centre"], atol=1e-12) and a["winner"] == b["winner"] and (a["w_final"][30:] == 0).all()
    assert np.isnan(a["r_final"][30:]).all()
    # all-parallel rays: no hypothesis, least-squares fall-back, which is singular too
    par = PR.consensus(o, np.tile(d[:1], (40, 1)), np.arange(40), np.ones(40), PR.TAU)
    assert par["status"] == 12 and par["winner"] == (-1, -1) and np.isnan(par["centre"]).all() and par["n_inliers"] == 0
    # k = 2: the one pair, or none
    two = PR.consensus(o[inl2(cam, o, d)], d[inl2(cam, o, d)], np.arange(2), np.ones(2), PR.TAU)
    assert two["winner"] == (0, 1) and two["status"] == 0 and np.linalg.norm(two["centre"] - cam) < 0.5
    away = PR.consensus(o[:2], -d[:2], np.arange(2), np.ones(2), PR.TAU)              # the closest approach lies behind both rays
    assert away["status"] & 8 and away["winner"] == (-1, -1)
    # the score prior follows val; zero and negative scores do not vote
    val = np.where(np.arange(40) % 2 == 0, 1.0, 0.0)
    val[1] = -3.0
    sc = PR.consensus(o, d, np.arange(40), val, PR.TAU, prior="score")
    assert (sc["w_final"][1::2] == 0).all() and abs(sc["w_final"].sum() - 1) < 1e-12
    assert np.linalg.norm(full["centre"] - cam) < 0.06


def inl2(cam, o, d):
    """Two rays of the scene that do see the camera."""
    v = cam[None] - o
    t = (v * d).sum(1)
    r = np.linalg.norm(v - t[:, None] * d, axis=1)
    return np.argsort(r)[:2]
