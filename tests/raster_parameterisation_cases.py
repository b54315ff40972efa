"""The two scenes of tests/test_gpu_raster_parameterisation.py that are not a seeded case of raster_backward_reference.PARAM_CASES, with
what the restatements alone say about them: a 66 000-Gaussian scene in which only 300 Gaussians are seen, and two one-tile scenes in
which every pixel stops early inside a list that takes several staging rounds.  No GPU is needed here:
tests/test_raster_parameterisation_host.py asserts the same without one."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402

N, SCENE_SEED, VIEWS, CAM_SEED, WIDTH, HEIGHT = RB.PARAM_BASE
GAUSSIAN_KEYS = RB.NAMES[:-1]
C0 = 0.28209479177387814

# ---- more than 65 536 Gaussians through the backward -------------------------------------------------------------------------------------
BIG_N = 66_000
BIG_SLOTS = np.concatenate([np.arange(0, 100), np.arange(65_500, 65_600), np.arange(65_900, 66_000)])       # blocks 0, 255, 256 and 257


def big_scene(syn):
    """66 000 Gaussians: the 300 of make_scene(300, 2) at BIG_SLOTS (in their order), every other one a filler both views cull -- centred
    50 units along minus the sum of the two viewing directions (w2c row 2), unit-normal spread, so behind both near planes."""
    small = syn.make_scene(N, SCENE_SEED)
    rows = RR.camera_rows(syn.make_cameras(VIEWS, CAM_SEED, width=WIDTH, height=HEIGHT))
    scene = syn.make_scene(BIG_N, 17)
    scene["xyz"] = (scene["xyz"].astype(np.float64) - 50.0 * (rows[0, 8:11] + rows[1, 8:11]).astype(np.float64)).astype(np.float32)
    for k in GAUSSIAN_KEYS:
        scene[k][BIG_SLOTS] = small[k]
    return scene, rows


_big = {}


def big_case(syn):
    if not _big:
        scene, rows = big_scene(syn)
        _big["c"] = RB.measure(RR.measure(scene, rows, WIDTH, HEIGHT), WIDTH, HEIGHT)
    return _big["c"]


def check_big_case(syn):
    """From the restatement alone: the fillers have radius 0 and are decidable in both precisions; the image, the instances and the
    gradients are those of the 300-Gaussian scene.  -> (the case, the mask of the fillers)."""
    c, small = big_case(syn), RB.case(syn, *RB.PARAM_BASE, 3)
    filler = np.ones(BIG_N, bool)
    filler[BIG_SLOTS] = False
    for r in (c["rr"]["r64"], c["rr"]["r32"]):
        assert not r["radii"][:, filler].any() and r["decidable"][:, filler].all()
    for p in ("r64", "r32"):
        assert np.array_equal(c["rr"][p]["image"], small["rr"][p]["image"])
        assert c["rr"][p]["instances"] == small["rr"][p]["instances"] > 0
    assert np.array_equal(c["rr"]["undecidable"], small["rr"]["undecidable"]) and np.array_equal(c["g"], small["g"])
    for k in GAUSSIAN_KEYS:
        assert np.array_equal(c["g64"][k][BIG_SLOTS], small["g64"][k]) and not c["g64"][k][filler].any() and not c["g32"][k][filler].any(), k
    return c, filler


# ---- an early stop inside a tile whose list takes several rounds --------------------------------------------------------------------------
ROW16 = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 10.0, 10.0, 8.0, 8.0]], np.float32)       # identity pose, f = 10, 16 x 16: one tile
# The stoppers are the "saturation" row of test_gpu_raster.test_edges_of_the_definition (o = 0.98 at z = 2.0, 2.1, 2.2) with sigma 20 for
# its 5: at f = 10 that is a sigma of 100 pixels at z = 2.0 and of 91 at z = 2.2, so alpha >= 0.98 exp(-(7.5^2 + 7.5^2) / (2 x 91^2)) =
# 0.973 on EVERY pixel of the tile and T' <= 0.027^3 = 2e-5 < 1e-4 at the third (sigma 5 would leave the tile's corners, alpha 0.87,
# blending on).
STOPPERS = dict(xyz=[[0, 0, 2.0], [0, 0, 2.1], [0, 0, 2.2]], sigma=[20.0] * 3, o=[0.98] * 3, colour=[(1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)])


def hand_scene(xyz, sigma, o, colour):
    """Isotropic Gaussians with given opacities (values in (0, 1)) and flat colours (SH degree 0), as the GPU tests' _hand makes them."""
    n = len(xyz)
    sigma = np.broadcast_to(np.asarray(sigma, np.float64).reshape(n, 1), (n, 3))
    o = np.asarray(o, np.float64).reshape(n, 1)
    return {"xyz": np.asarray(xyz, np.float32).reshape(n, 3), "log_scale": np.log(sigma).astype(np.float32),
            "rot": np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (n, 1)), "opacity": np.log(o / (1 - o)).astype(np.float32),
            "f_dc": ((np.asarray(colour, np.float64).reshape(n, 1, 3) - 0.5) / C0).astype(np.float32), "f_rest": np.zeros((n, 0, 3), np.float32),
            "sh_degree": 0}


def _scatter(rng, count, z_lo, z_hi, sigma, o):
    """count small Gaussians whose centres fall inside the 16 x 16 image, depths in [z_lo, z_hi]."""
    z = rng.uniform(z_lo, z_hi, count)
    uv = rng.uniform(0.5, 15.5, (count, 2))
    xyz = np.stack([(uv[:, 0] - 8.0) * z / 10.0, (uv[:, 1] - 8.0) * z / 10.0, z], axis=1)
    return dict(xyz=xyz.tolist(), sigma=(sigma * rng.uniform(0.8, 1.2, count)).tolist(), o=[o] * count, colour=rng.uniform(0.1, 0.9, (count, 3)).tolist())


def early_stop_scene(which):
    """A: the three stoppers in front of 600 small Gaussians (603 instances in the one tile: three staging rounds, every pixel stops at
    list position 2).  B: 600 faint small ones in front (o = 0.05), the stoppers at positions 600 .. 602 -- inside the third round --
    and 300 more behind, a fourth round no pixel reaches.  -> (scene, index of the first Gaussian no pixel adds)."""
    rng = np.random.default_rng(31 if which == "A" else 33)       # (B: seed 32 leaves one undecidable pixel, and one of 256 is past the cap)
    parts = [STOPPERS, _scatter(rng, 600, 2.5, 3.5, 0.3, 0.5)] if which == "A" else \
        [_scatter(rng, 600, 1.0, 1.8, 0.1, 0.05), STOPPERS, _scatter(rng, 300, 2.5, 3.5, 0.3, 0.5)]
    scene = hand_scene(*[sum((list(p[k]) for p in parts), []) for k in ("xyz", "sigma", "o", "colour")])
    return scene, (2 if which == "A" else 602)


_early = {}


def early_stop_case(which):
    """The scene's restatements and, from them alone, what the scene is for: every Gaussian is an instance of the one tile; before the
    stoppers T stays above 0.05 on every pixel (nothing saturates early); every pixel stops at the third stopper at the latest, clear of
    the 1e-4 threshold.  -> (the case, the Gaussians in blending order, the position of the first one no pixel adds)."""
    if which not in _early:
        scene, first_unused = early_stop_scene(which)
        c = RB.measure(RR.measure(scene, ROW16, 16, 16), 16, 16)
        n = scene["xyz"].shape[0]
        assert c["rr"]["r64"]["instances"] == c["rr"]["r64"]["instances_lo"] == c["rr"]["r64"]["instances_hi"] == n and n > 2 * RR.ROUND
        P = RR.project(scene, ROW16[0], 16, 16, np.float64)
        ys, xs = (a.reshape(-1) for a in np.meshgrid(np.arange(16), np.arange(16), indexing="ij"))
        order = np.lexsort((np.arange(n), P["z"]))
        assert np.array_equal(order, np.arange(n)[np.argsort(scene["xyz"][:, 2], kind="stable")]) and order[first_unused] == first_unused
        power, alpha = RR._alpha(P, order[:first_unused + 1], xs, ys, np.float64)
        T = np.cumprod(1.0 - np.where((power <= 0) & (alpha >= 1.0 / 255.0), alpha, 0.0), axis=0)
        assert first_unused == 2 or T[first_unused - 3].min() > 0.05, T[first_unused - 3].min()
        assert T[-1].max() < 0.5e-4, T[-1].max()
        for k in GAUSSIAN_KEYS:         # behind the stop: exact zeros in both precisions
            assert not c["g64"][k][order[first_unused:]].any() and not c["g32"][k][order[first_unused:]].any(), k
            assert k in ("rot", "f_rest") or np.abs(c["g64"][k][order[:first_unused]]).max() > 0, k
        _early[which] = (c, order, first_unused)
    return _early[which]
