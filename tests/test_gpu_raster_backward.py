"""sixdgs_raster_views_backward on the GPU against fp64 autograd of the torch restatement (tests/raster_backward_reference.py): all
seven gradient arrays under a bound taken from the restatement's own fp32 rounding, the edges of the definition on hand-made scenes,
determinism and batching bit for bit, guard bytes through the raw C call, and the torch.autograd.Function.  Everything runs inside
this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C0 = 0.28209479177387814
KEYS = ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


def _dev(scene):
    return [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in KEYS] + [int(scene["sh_degree"])]


def _run(ops, scene, rows, width, height, g, background=RR.BACKGROUND, max_instances=None, **kw):
    """Forward (float image, state) and backward -> (image, dict of the gradients asked for, the instance count)."""
    args, cams = _dev(scene), torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    image, count, state = ops.raster_views(*args, cams, width, height, want_float=True, want_u8=False, want_instances=True, want_state=True,
                                           background=background, max_instances=max_instances)
    grads = ops.raster_views_backward(*args, cams, width, height, torch.from_numpy(np.array(g, np.float32)).cuda(), state,
                                      background=background, **kw)
    return image, {k: v for k, v in zip(RB.NAMES, grads) if v is not None}, count


def _compare(got, g64, bounds, what, skip=()):
    """Every array within its bound of fp64; prints measured / bound -> the largest ratio."""
    worst = 0.0
    for k in RB.NAMES:
        if k in skip:
            continue
        scale, y, limit = bounds[k]
        a, ref = got[k].cpu().numpy().astype(np.float64).reshape(g64[k].shape), g64[k]
        if not ref.size:
            assert a.size == 0
            continue
        err = float(np.abs(a - ref).max())
        if scale == 0.0:
            assert not a.any(), f"{what} {k}: nonzero where fp64 is zero"
            continue
        assert limit <= RB.CEILING * scale, f"{what} {k}: the case is unfit (bound {limit / scale:.2e} of the scale)"
        print(f"{what} {k}: max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
        assert np.isfinite(a).all() and err <= limit, f"{what} {k}: {err:.3e} > {limit:.3e} at {np.argwhere(np.abs(a - ref) > limit)[:3]}"
        worst = max(worst, err / limit)
    return worst


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", RB.CASES)
def test_gradients_against_fp64_autograd(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """Measured on MI355X, max |gpu - fp64| / bound per case and array: see profiles/raster_backward.md."""
    c = RB.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    assert c["rr"]["undecidable"].mean() <= RR.MAX_UNDECIDABLE_SHARE
    image, got, _ = _run(ops, c["scene"], c["rows"], width, height, c["g"])
    for k, name in zip(RB.NAMES, ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest", "cams")):
        assert got[k].dtype == torch.float32 and got[k].shape == (c["rows"].shape if k == "cams" else c["scene"][k].shape), name
    _compare(got, c["g64"], c["bounds"], f"n={n} {width}x{height} deg={sh_degree}")


ROW = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 20.0, 20.0, 16.0, 16.0]], np.float32)       # identity pose, f = 20, 32 x 32


def _hand(xyz, sigma, o, colour):
    """A scene of isotropic-or-not Gaussians with given opacities (values in (0, 1)) and flat colours (SH degree 0)."""
    n = len(xyz)
    sigma = np.asarray(sigma, np.float64)
    sigma = np.broadcast_to(sigma.reshape(n, 1) if sigma.ndim == 1 else sigma, (n, 3))
    o = np.asarray(o, np.float64).reshape(n, 1)
    return {"xyz": np.asarray(xyz, np.float32).reshape(n, 3), "log_scale": np.log(sigma).astype(np.float32),
            "rot": np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (n, 1)), "opacity": np.log(o / (1 - o)).astype(np.float32),
            "f_dc": ((np.asarray(colour, np.float64).reshape(n, 1, 3) - 0.5) / C0).astype(np.float32), "f_rest": np.zeros((n, 0, 3), np.float32),
            "sh_degree": 0}


def _hand_check(ops, scene, what, background=(0.25, 0.5, 1.0), only=None):
    """The hand-made scene at 32 x 32 against fp64 under the bound rule of the cases; only: the pixels (a pair of slices) that carry a
    loss weight -> (gpu gradients as numpy, fp64 gradients).  Where every Gaussian is isotropic its covariance does not depend on its
    rotation: d rot is zero by symmetry, fp64 and fp32 autograd leave rounding noise there that no relative bound can be taken from,
    and the kernel's is held against 1e-6 of the scale of d log_scale, which the same terms feed."""
    r64 = RR.reference_view(scene, ROW[0], 32, 32, np.float64, background=background)
    r32 = RR.reference_view(scene, ROW[0], 32, 32, np.float32, background=background)
    und = (r64["undecidable"] | r32["undecidable"])[None]
    g = RB.loss_weights((1, 32, 32, 4), und)
    if only is not None:
        keep = np.zeros((1, 32, 32), bool)
        keep[0][only] = True
        g[~keep] = 0
    g64 = RB.gradients(scene, ROW, 32, 32, np.float64, g, background=background)
    g32 = RB.gradients(scene, ROW, 32, 32, np.float32, g, background=background)
    assert np.abs(g64["image"][0] - r64["image"]).max() <= 1e-12
    _, got, _ = _run(ops, scene, ROW, 32, 32, g, background=background)
    isotropic = bool((scene["log_scale"] == scene["log_scale"][:, :1]).all())
    _compare(got, g64, RB.bounds(g64, g32), what, skip=("rot",) if isotropic else ())
    got = {k: v.cpu().numpy() for k, v in got.items()}
    if isotropic:
        assert np.abs(got["rot"]).max() <= 1e-6 * np.abs(g64["log_scale"]).max(), what
    return got, g64


def test_edges_of_the_definition(ops):
    red, green, blue, grey = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)
    mid = (slice(12, 20), slice(12, 20))
    # the saturation row (three near-opaque Gaussians and one behind): on the middle pixels the blend stops at the third, so the third
    # and the fourth get exact zeros from them, and the first two match fp64
    four = _hand([[0, 0, 2.0], [0, 0, 2.1], [0, 0, 2.2], [0, 0, 2.3]], 5.0, [0.98] * 4, [red, blue, green, green])
    got, g64 = _hand_check(ops, four, "saturation", only=mid)
    for k in KEYS[:-1]:
        assert not got[k][2:].any(), k
    assert np.abs(got["xyz"][:2]).max() > 0 and np.abs(got["opacity"][:2]).max() > 0
    # behind the near plane, an empty rectangle: exact zeros beside a visible Gaussian; o < 1/255: zeros everywhere
    got, g64 = _hand_check(ops, _hand([[0, 0, 0.1], [-12.0, 0, 2.0], [0, 0, 2.0]], [0.05, 0.05, 0.2], [0.9] * 3, [red, blue, grey]), "culled")
    for k in KEYS[:-1]:
        assert not got[k][:2].any(), k
    assert np.abs(got["xyz"][2]).max() > 0 and np.abs(got["cams"]).max() > 0
    got, _ = _hand_check(ops, _hand([[0, 0, 2.0]], 0.2, [0.0035], [red]), "faint")
    assert not any(v.any() for v in got.values())
    # an opaque Gaussian: o exp(power) = 0.9999 exp(-0.25 / 100.3) > 0.99 on the four centre pixels, which therefore give nothing to
    # its opacity, conic and centre, but still to its colour
    centre = (slice(15, 17), slice(15, 17))
    got, g64 = _hand_check(ops, _hand([[0, 0, 2.0]], 1.0, [0.9999], [grey]), "0.99 clamp", only=centre)
    assert not got["opacity"].any() and not got["log_scale"].any() and not got["rot"].any() and not got["xyz"].any()
    assert not got["cams"].any()
    assert np.abs(got["f_dc"]).max() > 0.1
    got, g64 = _hand_check(ops, _hand([[0, 0, 2.0]], 1.0, [0.9999], [grey]), "0.99 clamp, every pixel")
    assert np.abs(got["opacity"]).max() > 0
    # far off-axis: p.x / p.z = 1.6 against 1.3 tanx = 1.04, the clamp acts
    got, g64 = _hand_check(ops, _hand([[3.2, 0.4, 2.0]], [[0.3, 0.3, 1.0]], [0.9], [grey]), "1.3 tan clamp")
    assert np.abs(got["cams"][0, 12]).max() > 0
    # n == 0: zero d_cams
    empty = {k: v[:0] for k, v in _hand([[0, 0, 2.0]], 0.2, [0.5], [red]).items() if isinstance(v, np.ndarray)}
    empty["sh_degree"] = 0
    g = RB.loss_weights((2, 24, 40, 4), np.zeros((2, 24, 40), bool))
    _, got, count = _run(ops, empty, np.repeat(ROW, 2, 0), 40, 24, g)
    assert count == 0 and got["cams"].shape == (2, 16) and not bool(got["cams"].any()) and got["xyz"].shape == (0, 3)


def test_determinism_batching_capacity_and_subsets(ops, syn):
    scene = syn.make_scene(3000, 9)
    rows = RR.camera_rows(syn.make_cameras(2, 10, width=96, height=64))
    g = np.random.default_rng(2).standard_normal((2, 64, 96, 4)).astype(np.float32)
    img_a, a, count = _run(ops, scene, rows, 96, 64, g)
    img_b, b, _ = _run(ops, scene, rows, 96, 64, g)
    assert count > 3000 and torch.equal(img_a, img_b)
    for k in RB.NAMES:
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()) and bool(a[k].any()), k
    # views do not mix: d_cams row by row, and each Gaussian array = the single views' added in view order in fp32
    single = [_run(ops, scene, rows[v:v + 1], 96, 64, g[v:v + 1])[1] for v in range(2)]
    for v in range(2):
        assert torch.equal(a["cams"][v], single[v]["cams"][0]), v
    for k in RB.NAMES[:-1]:
        assert torch.equal(a[k], single[0][k] + single[1][k]), k
    # the exact capacity and a retried one give the bytes of the roomy one
    for cap in (count, 1):
        _, c, c_count = _run(ops, scene, rows, 96, 64, g, max_instances=cap)
        assert c_count == count and all(torch.equal(a[k], c[k]) for k in RB.NAMES), cap
    # a subset of the outputs: the same bytes for those
    for want in (("cams",), ("xyz", "f_rest"), ("opacity", "rot", "scale")):
        _, s, _ = _run(ops, scene, rows, 96, 64, g, want=want)
        names = {"scale": "log_scale"}
        assert set(s) == {names.get(w, w) for w in want} and all(torch.equal(a[k], s[k]) for k in s), want


def test_guard_bytes_through_the_c_call(ops, syn):
    lib = importlib.import_module("6dgs_amd._lib").load()
    n, views, width, height = 3000, 2, 96, 64
    scene = syn.make_scene(n, 9)
    rows = RR.camera_rows(syn.make_cameras(views, 10, width=width, height=height))
    g = np.random.default_rng(2).standard_normal((views, height, width, 4)).astype(np.float32)
    args, cams, gt = _dev(scene), torch.from_numpy(rows).cuda(), torch.from_numpy(g).cuda()
    _, want, _ = _run(ops, scene, rows, width, height, g, background=(1.0, 1.0, 1.0))
    (fwd_ws, cap) = ops.raster_views(*args, cams, width, height, want_u8=False, want_state=True)
    before = fwd_ws.clone()
    need = ops.raster_views_backward_workspace_bytes(n, views, width, height, cap)
    assert need >= 36 * cap
    guard = 256
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = [3 * n, 3 * n, 4 * n, n, 3 * n, 45 * n, 16 * views]
    outs = [torch.full((4 * s + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes]
    bg = torch.ones(3, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    st = lib.sixdgs_raster_views_backward(p(args[0]), p(args[1]), 1, p(args[2]), p(args[3]), 1, p(args[4]), p(args[5]), 3, 16, n, p(cams), views,
                                          width, height, 1.0, p(bg), p(gt), cap, p(fwd_ws), fwd_ws.numel(), *[p(o, guard) for o in outs],
                                          p(ws, guard), need, torch.cuda.current_stream().cuda_stream, None)
    torch.cuda.synchronize()
    assert st == 0
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[-guard:] == 0xA5).all()), "the workspace's guard bytes were written"
    for o, k in zip(outs, RB.NAMES):
        assert bool((o[:guard] == 0x5A).all()) and bool((o[-guard:] == 0x5A).all()), f"the guard bytes of d {k} were written"
        assert torch.equal(o[guard:-guard].view(torch.float32), want[k].reshape(-1)), k
    assert torch.equal(fwd_ws, before), "the forward's workspace was written"


def test_autograd_function(pkg, ops, syn):
    autograd = importlib.import_module("6dgs_amd.autograd")
    assert pkg.raster_views is autograd.raster_views
    scene = syn.make_scene(3000, 9)
    rows = RR.camera_rows(syn.make_cameras(2, 10, width=96, height=64))
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 64, 96, 4)).astype(np.float32)).cuda()
    plain, raw, _ = _run(ops, scene, rows, 96, 64, g.cpu().numpy(), background=(0.0, 0.5, 1.0))
    args, cams = _dev(scene), torch.from_numpy(rows).cuda()
    for needs in ((True,) * 7, (True, False, False, True, False, False, True), (False,) * 6 + (True,)):
        leaves = [t.clone().requires_grad_(r) for t, r in zip(args[:6] + [cams], needs)]
        image = autograd.raster_views(*leaves[:6], 3, leaves[6], 96, 64, background=(0.0, 0.5, 1.0))
        assert image.requires_grad and torch.equal(image.detach(), plain)
        image.backward(g, retain_graph=True)
        first = [None if t.grad is None else t.grad.clone() for t in leaves]
        for t, r, k in zip(leaves, needs, RB.NAMES):
            assert (t.grad is not None) == r, k
            if r:
                assert torch.equal(t.grad, raw[k]), k
                t.grad = None
        image.backward(g)           # a second time through the retained graph
        for t, f, k in zip(leaves, first, RB.NAMES):
            assert (f is None and t.grad is None) or torch.equal(t.grad, f), k
    frozen = autograd.raster_views(*args[:6], 3, cams, 96, 64, background=(0.0, 0.5, 1.0))
    assert not frozen.requires_grad and torch.equal(frozen, plain)
