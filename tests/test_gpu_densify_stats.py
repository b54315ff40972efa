"""sixdgs_densify_stats on the GPU: the raw (du, dv) per (view, Gaussian) against fp64 autograd of the torch restatement with u, v
retained as leaves (tests/densify_reference.py) under a bound taken from the restatement's own fp32 rounding; the three statistics
restated in numpy from the kernel's own grad2d and radii, bit for bit; accumulation over calls; views alone and in a batch; a Gaussian
seen in no view; an overflowed capacity; guard values behind every output.  Everything runs inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import densify_reference as D  # noqa: E402
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")
CASE = (2000, 0, 3, 21, 64, 64)
SIZE = 64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    importlib.import_module("6dgs_amd")
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def case(syn):
    return RB.case(syn, *CASE)


def subset(case, n, views):
    """The first n Gaussians and views of the case; with n > 1 the middle one is made invisible everywhere (a NaN position is culled)."""
    scene = {k: np.array(case["scene"][k][:n]) for k in KEYS}
    if n > 1:
        scene["xyz"][n // 2] = np.nan
    return scene, np.array(case["rows"][:views]), np.array(case["g"][:views])


def bits(t):
    return t.contiguous().view(torch.int32)


def run(ops, scene, rows, g, stats=None, status=None):
    """Forward, backward in a kept workspace and one sixdgs_densify_stats -> (grad2d, radii, stats, (state, bwd workspace))."""
    args = [torch.from_numpy(np.array(scene[k])).cuda() for k in KEYS] + [3]
    cams = torch.from_numpy(np.array(rows)).cuda()
    n, views = args[0].shape[0], cams.shape[0]
    _, radii, state = ops.raster_views(*args, cams, SIZE, SIZE, want_float=True, want_u8=False, want_radii=True, want_state=True,
                                       background=RR.BACKGROUND)
    bwd_ws = torch.empty(ops.raster_views_backward_workspace_bytes(n, views, SIZE, SIZE, state[1]), dtype=torch.uint8, device="cuda")
    d_xyz = ops.raster_views_backward(*args, cams, SIZE, SIZE, torch.from_numpy(np.array(g)).cuda(), state, background=RR.BACKGROUND,
                                      want=("xyz",), workspace=bwd_ws)[0]
    stats = ops.densify_stats_state(n, "cuda") if stats is None else stats
    before = state[0].clone(), bwd_ws.clone()
    grad2d = ops.densify_stats(state, bwd_ws, radii, stats, SIZE, SIZE, want_grad2d=True, status=status)
    assert torch.equal(state[0], before[0]) and torch.equal(bwd_ws, before[1]), "a workspace was written"
    return grad2d, radii, stats, (state, bwd_ws), d_xyz


def to_np(stats):
    return {k: v.cpu().numpy() for k, v in stats.items()}


def same_stats(got, want):
    return all(np.array_equal(got[k].cpu().numpy().view(np.int32), np.ascontiguousarray(want[k]).view(np.int32)) for k in want)


def test_grad2d_against_fp64_autograd(ops, case):
    """The bound is the project's bounds() rule: max(FACTOR * the fp32 restatement's error, FLOOR * scale), on the (view, Gaussian)
    pairs whose rectangle both precisions decide alike."""
    g64 = D.grad2d(case["scene"], case["rows"], SIZE, SIZE, np.float64, case["g"])
    g32 = D.grad2d(case["scene"], case["rows"], SIZE, SIZE, np.float32, case["g"])
    grad2d, radii, stats, _, _ = run(ops, case["scene"], case["rows"], case["g"])
    got = grad2d.cpu().numpy().astype(np.float64)
    dec = np.asarray(case["rr"]["decidable"])
    visible = radii.cpu().numpy() > 0
    assert got.shape == (3, 2000, 2) and dec.mean() > 0.99 and visible[dec].sum() > 1000
    assert np.array_equal(visible[dec], (np.asarray(case["rr"]["r64"]["radii"]) > 0)[dec])
    assert not got[~visible].any(), "grad2d is not exactly zero where the rectangle is empty"
    scale = float(np.abs(g64[dec]).max())
    y = float(np.abs(g32[dec].astype(np.float64) - g64[dec]).max())
    limit = max(RB.FACTOR * y, RB.FLOOR * scale)
    err = float(np.abs(got[dec] - g64[dec]).max())
    print(f"grad2d: max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
    assert limit <= RB.CEILING * scale, "the case is unfit"
    assert np.isfinite(got).all() and err <= limit
    assert same_stats(stats, D.stats_update(to_np(ops.densify_stats_state(2000, "cpu")), grad2d.cpu().numpy(), radii.cpu().numpy(), SIZE, SIZE))


@pytest.mark.parametrize("n", (1, 257, 2000))
@pytest.mark.parametrize("views", (1, 3))
def test_statistics_are_the_restatement_of_the_kernels_own_grad2d(ops, case, n, views):
    scene, rows, g = subset(case, n, views)
    grad2d, radii, stats, _, d_xyz = run(ops, scene, rows, g)
    g2, r = grad2d.cpu().numpy(), radii.cpu().numpy()
    assert g2.shape == (views, n, 2) and r.shape == (views, n) and (n == 1 or (r > 0).sum() > n // 4)
    once = D.stats_update(to_np(ops.densify_stats_state(n, "cpu")), g2, r, SIZE, SIZE)
    assert same_stats(stats, once)
    assert np.array_equal(once["denom"], (r > 0).sum(axis=0)) and np.array_equal(once["max_radii"], r.max(axis=0))
    if n > 1:
        assert (g2[r > 0] != 0).any() and bool(torch.isfinite(d_xyz[torch.arange(n) != n // 2]).all())
    # a Gaussian seen in no view keeps denom == 0 and a zero sum
    unseen = (r > 0).sum(axis=0) == 0
    assert n == 1 or unseen[n // 2]
    assert not stats["denom"].cpu().numpy()[unseen].any() and not stats["grad_accum"].cpu().numpy()[unseen].any() and not g2[:, unseen].any()
    # a second, accumulating call: the hand sum; the same bytes twice
    grad2d_b, _, stats, _, _ = run(ops, scene, rows, g, stats=stats)
    assert torch.equal(bits(grad2d), bits(grad2d_b)) and same_stats(stats, D.stats_update(once, g2, r, SIZE, SIZE))
    # a view's contribution is the same bits alone or in the batch
    if views > 1:
        alone = ops.densify_stats_state(n, "cuda")
        for v in range(views):
            g_v, r_v, alone, _, _ = run(ops, scene, rows[v:v + 1], g[v:v + 1], stats=alone)
            assert torch.equal(bits(g_v[0]), bits(grad2d[v])) and torch.equal(r_v[0], radii[v]), v
        assert same_stats(alone, once)
    # with bit 1 of the status set nothing changes
    frozen = {k: v.clone() for k, v in stats.items()}
    run(ops, scene, rows, g, stats=stats, status=torch.tensor([2], dtype=torch.int32, device="cuda"))
    assert all(torch.equal(stats[k], frozen[k]) for k in stats)
    run(ops, scene, rows, g, stats=stats, status=torch.tensor([1], dtype=torch.int32, device="cuda"))
    assert not torch.equal(stats["denom"], frozen["denom"]) or n == 1 and not (r > 0).any()


def test_overflow_changes_nothing_and_guards_survive_through_the_c_call(ops, case):
    lib = importlib.import_module("6dgs_amd._lib").load()
    n, views = 257, 3
    scene, rows, g = subset(case, n, views)
    grad2d, radii, stats, (state, bwd_ws), _ = run(ops, scene, rows, g)
    guard = 64
    fill = {torch.float32: 7.5, torch.int32: 77}
    outs = {k: torch.full((n + 2 * guard,), fill[dt], dtype=dt, device="cuda") for k, dt in ops.DENSIFY_STATS}
    for k in outs:
        outs[k][guard:guard + n] = 0
    g2 = torch.full((views * n * 2 + 2 * guard,), 7.5, device="cuda")
    p = lambda t, off=0: t.data_ptr() + 4 * off      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    st = lib.sixdgs_densify_stats(n, views, SIZE, SIZE, state[1], p(state[0]), state[0].numel(), p(bwd_ws), bwd_ws.numel(), p(radii),
                                  p(outs["grad_accum"], guard), p(outs["denom"], guard), p(outs["max_radii"], guard), p(g2, guard), None, stream)
    torch.cuda.synchronize()
    assert st == 0
    for k, t in outs.items():
        assert bool((t[:guard] == fill[t.dtype]).all()) and bool((t[-guard:] == fill[t.dtype]).all()), f"the guard values of {k} were written"
        assert torch.equal(t[guard:-guard], stats[k]), k
    assert bool((g2[:guard] == 7.5).all()) and bool((g2[-guard:] == 7.5).all()) and torch.equal(bits(g2[guard:-guard]), bits(grad2d.reshape(-1)))
    # a forward whose capacity is one instance short: the backward writes nothing, and neither does the statistics kernel
    args = [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in KEYS]
    cams, gt, bg = torch.from_numpy(rows).cuda(), torch.from_numpy(g).cuda(), torch.tensor(RR.BACKGROUND, device="cuda")
    needed = ops.raster_views(*args, 3, cams, SIZE, SIZE, want_u8=False, want_instances=True, background=RR.BACKGROUND)
    cap = needed - 1
    assert cap >= 1
    fwd = torch.zeros(ops.raster_views_workspace_bytes(n, views, SIZE, SIZE, cap), dtype=torch.uint8, device="cuda")
    bwd = torch.zeros(ops.raster_views_backward_workspace_bytes(n, views, SIZE, SIZE, cap), dtype=torch.uint8, device="cuda")
    image, count = torch.zeros(views, SIZE, SIZE, 4, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    rad, d_xyz = torch.zeros(views, n, dtype=torch.int32, device="cuda"), torch.zeros(n, 3, device="cuda")
    q = lambda t: t.data_ptr()      # noqa: E731
    scene_args = (q(args[0]), q(args[1]), 1, q(args[2]), q(args[3]), 1, q(args[4]), q(args[5]), 3, 16, n, q(cams), views, SIZE, SIZE, 1.0, q(bg))
    assert lib.sixdgs_raster_views(*scene_args, q(image), None, 3, q(rad), cap, q(count), q(fwd), fwd.numel(), stream, None) == 0
    assert lib.sixdgs_raster_views_backward(*scene_args, q(gt), cap, q(fwd), fwd.numel(), q(d_xyz), None, None, None, None, None, None, q(bwd),
                                            bwd.numel(), stream, None) == 0
    kept = {k: t.clone() for k, t in outs.items()}
    kept_g2 = g2.clone()
    st = lib.sixdgs_densify_stats(n, views, SIZE, SIZE, cap, q(fwd), fwd.numel(), q(bwd), bwd.numel(), q(rad), p(outs["grad_accum"], guard),
                                  p(outs["denom"], guard), p(outs["max_radii"], guard), p(g2, guard), None, stream)
    torch.cuda.synchronize()
    assert st == 0 and int(count) == needed
    assert all(torch.equal(outs[k], kept[k]) for k in outs) and torch.equal(bits(g2), bits(kept_g2)), "an overflowed capacity changed something"
