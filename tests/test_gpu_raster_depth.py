"""sixdgs_raster_depth and sixdgs_scene_depth on the GPU: alpha against the forward's own bytes, the median against the numpy restatement
of the definition (tests/depth_reference.py), the depth channel and the lifted points against fp64 within a bound taken from the
restatement's own fp32 rounding, two identities that need no reference (the contribution pass's weights; reprojection of the points),
the contract (determinism, batching, chunking, capacity, guard bytes, NULL outputs, n == 0, argument errors) and the consumers end to
end.  Everything runs inside this process."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as DR  # noqa: E402
import raster_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MAPS = ("expected", "median", "median_index", "alpha")
CASE_ARGS = "n,scene_seed,views,cam_seed,width,height,sh_degree"


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("6dgs_amd._lib").load()


def _dev(scene):
    return [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + \
        [int(scene["sh_degree"])]


_runs = {}


def _run(ops, syn, case):
    """One forward of the case's rows and the depth pass on its state, with both kinds of points, once per session -> (the reference
    pair, {maps, points_median, points_expected as numpy}, the float image, the state)."""
    if case not in _runs:
        c = DR.case(syn, *case)
        n, _, views, _, width, height, _ = case
        cams = torch.from_numpy(np.ascontiguousarray(c["rows"])).cuda()
        image, state = ops.raster_views(*_dev(c["scene"]), cams, width, height, want_float=True, want_u8=False, want_state=True)
        got = ops.raster_depth(state, n, views, width, height, cams=cams, points="median")
        other = ops.raster_depth(state, n, views, width, height, cams=cams, want=("alpha",), points="expected")
        assert torch.equal(other["alpha"], got["alpha"])
        assert got["expected"].dtype == torch.float32 and got["median_index"].dtype == torch.int32 and got["points"].shape == (views, height, width, 3)
        g = {k: got[k].cpu().numpy() for k in MAPS}
        g["points_median"], g["points_expected"] = got["points"].cpu().numpy(), other["points"].cpu().numpy()
        _runs[case] = (c, g, image, state)
    return _runs[case]


@pytest.mark.parametrize(CASE_ARGS, DR.CASES)
def test_alpha_is_the_forwards_alpha_byte_for_byte(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """No reference involved: the walk is the blend's, so 1 - T is the same bits as channel 3 of the image the state came from."""
    _, g, image, _ = _run(ops, syn, (n, scene_seed, views, cam_seed, width, height, sh_degree))
    fwd = image[..., 3].cpu().numpy()
    assert np.array_equal(g["alpha"].view(np.uint32), fwd.view(np.uint32)), np.argwhere(g["alpha"] != fwd)[:4].tolist()
    assert 0.0 < float(fwd.max()) <= 1.0


@pytest.mark.parametrize(CASE_ARGS, DR.CASES)
def test_the_median_is_the_restatements(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    c, g, _, _ = _run(ops, syn, (n, scene_seed, views, cam_seed, width, height, sh_degree))
    und = c["undecidable"]
    print(f"n={n} {width}x{height}x{views} deg={sh_degree}: {und.sum()} of {und.size} pixels undecidable ({und.mean():.2e})")
    assert und.mean() <= RR.MAX_UNDECIDABLE_SHARE
    idx = g["median_index"].astype(np.int64)
    bad = (idx != c["r64"]["median_index"]) & ~und
    assert not bad.any(), f"median_index differs at {np.argwhere(bad)[:4].tolist()}"
    v, y, x = np.nonzero((idx >= 0) & ~und)
    assert v.size > 0 and np.array_equal(g["median"][v, y, x].view(np.uint32), c["r32"]["z"][v, idx[v, y, x]].view(np.uint32))
    none = (idx < 0)
    assert (g["median"][none] == 0).all() and not g["points_median"][none].any() and (idx >= -1).all() and (idx < n).all()


@pytest.mark.parametrize(CASE_ARGS, DR.CASES)
def test_expected_and_points_against_fp64(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    """|gpu - fp64| / max(1, |fp64|) outside the undecidable pixels, under depth_reference.tolerance: 4 x the fp32 restatement's own
    deviation of that quantity in this case, floored at 1e-6 and capped at raster_reference.ERROR_CEILING."""
    c, g, _, _ = _run(ops, syn, (n, scene_seed, views, cam_seed, width, height, sh_degree))
    keep = ~c["undecidable"]
    for k in DR.MEASURED:
        dev, tol = DR.deviation(g[k], c["r64"][k], keep), DR.tolerance(c, k)
        print(f"n={n} {width}x{height}x{views} deg={sh_degree} {k}: max |gpu - fp64| / max(1, |fp64|) {dev:.3e} (fp32 restatement "
              f"{c['deviations'][k]:.3e}, bound {tol:.3e}, ratio {dev / tol:.3f})")
        assert tol <= RR.ERROR_CEILING and dev <= tol, k
    assert not g["points_expected"][g["alpha"] == 0].any() and g["points_expected"][g["alpha"] > 0].any()


def test_the_depth_channel_sums_to_the_contributions_times_depth(ops, syn):
    """Per view, sum over pixels of `expected` against sum over Gaussians of z_vi view_weight[v, i] from ops.raster_contrib on the same
    state, within 2^-23 z_max (sum of view_pixels + H W) 2.  Both sides sum z alpha T over the same (pixel, Gaussian) pairs.  Per pair
    the depth pass forms fl(fl(z alpha) T), two roundings, and the contribution pass fl(alpha T), one, multiplied by z here in fp64: three
    relative roundings of 2^-24 on a term of at most z_max, 1.5 x 2^-23 z_max; the pixel's running sum D <= z_max is rounded once per
    pair, 0.5 x 2^-23 z_max: together the factor 2 on the number of pairs, which is the sum of view_pixels.  The H W term is the same
    factor on the contribution side's own summation (its tree over a tile's pixels and its chain over tiles), whose partial sums add
    up to the view's sum of alpha <= H W -- as test_conservation_against_the_image_alpha allows one 2^-23 per pixel for it."""
    for case in DR.CASES:
        c, g, _, state = _run(ops, syn, case)
        n, _, views, _, width, height, _ = case
        con = ops.raster_contrib(state, n, views, width, height, want_views=True)
        weight, pixels = con["view_weight"].cpu().numpy().astype(np.float64), con["view_pixels"].cpu().numpy().astype(np.int64)
        z = c["r32"]["z"].astype(np.float64)
        for v in range(views):
            seen = pixels[v] > 0
            lhs, rhs = g["expected"][v].astype(np.float64).sum(), (z[v][seen] * weight[v][seen]).sum()
            limit = 2.0 ** -23 * z[v][seen].max() * (int(pixels[v].sum()) + height * width) * 2
            print(f"n={n} {width}x{height} view {v}: sum expected {lhs:.6f}, sum z w {rhs:.6f}, |diff| {abs(lhs - rhs):.3e} (bound {limit:.3e}, "
                  f"ratio {abs(lhs - rhs) / limit:.3f})")
            assert abs(lhs - rhs) <= limit and lhs > 0, (case, v)


def test_points_project_back_to_their_pixel(ops, syn):
    """A valid point, projected with its view's row in fp64, is the pixel's centre within 1e-3 px at depth d within 1e-5 relative."""
    for case in DR.CASES:
        c, g, _, _ = _run(ops, syn, case)
        _, _, views, _, width, height, _ = case
        ys, xs = np.mgrid[0:height, 0:width]
        mean = np.divide(g["expected"].astype(np.float64), g["alpha"].astype(np.float64), out=np.zeros(g["alpha"].shape), where=g["alpha"] > 0)
        for kind, d, valid in (("median", g["median"].astype(np.float64), g["median_index"] >= 0), ("expected", mean, g["alpha"] > 0)):
            worst_px = worst_d = 0.0
            for v in range(views):
                m = c["rows"][v].astype(np.float64)
                W, t = m[:12].reshape(3, 4)[:, :3], m[:12].reshape(3, 4)[:, 3]
                p = g["points_" + kind][v].astype(np.float64) @ W.T + t
                on = valid[v]
                assert on.any()
                px = np.hypot(m[12] * p[..., 0][on] / p[..., 2][on] + m[14] - (xs[on] + 0.5), m[13] * p[..., 1][on] / p[..., 2][on] + m[15] - (ys[on] + 0.5))
                worst_px, worst_d = max(worst_px, float(px.max())), max(worst_d, float((np.abs(p[..., 2][on] - d[v][on]) / d[v][on]).max()))
            print(f"n={case[0]} {width}x{height} {kind}: reprojection off by at most {worst_px:.2e} px, depth by {worst_d:.2e} relative")
            assert worst_px <= 1e-3 and worst_d <= 1e-5, (case, kind)


def _equal(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _guarded(nbytes, fill, guard=256):
    return torch.full((nbytes + 2 * guard,), fill, dtype=torch.uint8, device="cuda")


def _intact(t, fill, guard=256):
    return bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all())


ALL = MAPS + ("points",)
DTYPES = dict(expected=torch.float32, median=torch.float32, median_index=torch.int32, alpha=torch.float32, points=torch.float32)


def test_determinism_batching_chunking_and_capacity(ops, lib, syn):
    c, _, _, state = _run(ops, syn, DR.BIG)
    n, _, views, _, width, height, _ = DR.BIG
    args = _dev(c["scene"])
    cams = torch.from_numpy(np.ascontiguousarray(c["rows"])).cuda()
    for kind in DR.KINDS:
        before = state[0].clone()
        a = ops.raster_depth(state, n, views, width, height, cams=cams, points=kind)
        b = ops.raster_depth(state, n, views, width, height, cams=cams, points=kind)
        assert _equal(a, b, ALL) and torch.equal(state[0], before), "not the same bytes, or fwd_ws was written"
        # each view alone is its rows of the batch
        for v in range(views):
            _, st = ops.raster_views(*args, cams[v:v + 1], width, height, want_u8=True, want_state=True)
            one = ops.raster_depth(st, n, 1, width, height, cams=cams[v:v + 1], points=kind)
            assert all(torch.equal(one[k][0], a[k][v]) for k in ALL), (kind, v)
        # sixdgs_scene_depth at chunk 1, 2 and 5 equals them, its image is the forward's; a capacity of 1 is retried with the needed one
        image = ops.raster_views(*args, cams, width, height, background=RR.BACKGROUND)
        needed = {}
        for chunk in (1, 2, views):
            s = ops.scene_depth_raw(*args, cams, width, height, points=kind, want_image=True, chunk=chunk, background=RR.BACKGROUND)
            assert _equal(s, a, ALL) and torch.equal(s["image"], image) and int(s["status"]) == 0, (kind, chunk)
            needed[chunk] = s["instances_needed"]
        s = ops.scene_depth_raw(*args, cams, width, height, points=kind, chunk=2, max_instances=1)
        assert _equal(s, a, ALL) and s["max_instances"] == needed[2] and int(s["status"]) == 0 and "image" not in s
        s = ops.scene_depth_raw(*args, cams, width, height, points=kind, chunk=2, max_instances=1, retry=False)
        assert int(s["status"]) == 2 and s["instances_needed"] == needed[2] and not any(bool(s[k].any()) for k in ("expected", "median", "alpha", "points"))
        assert bool((s["median_index"] == -1).all())
    counts = [ops.raster_views(*args, cams[v:v + 1], width, height, want_u8=False, want_instances=True) for v in range(views)]
    assert needed[1] == max(counts) and needed[views] == sum(counts) and needed[2] == max(counts[0] + counts[1], counts[2] + counts[3], counts[4])
    # capacity 1 through the C call: bit 1, the needed count, every output as it was, no guard byte written
    px = views * height * width
    sizes = {"expected": 4 * px, "median": 4 * px, "median_index": 4 * px, "alpha": 4 * px, "points": 12 * px, "image": 4 * px}
    outs = {k: _guarded(b_, 0x5A) for k, b_ in sizes.items()}
    flags = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    bg = torch.tensor(RR.BACKGROUND, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda cap, w: lib.sixdgs_scene_depth(p(args[0]), p(args[1]), 1, p(args[2]), p(args[3]), 1, p(args[4]), p(args[5]), 3, 16, n, p(cams),  # noqa: E731
                                                 views, width, height, 1.0, p(bg), views, cap, *[p(outs[k], 256) for k in ALL], 1, p(outs["image"], 256),
                                                 4, p(flags, 4), p(cnt, 8), p(w, 256), w.numel() - 512, stream)
    ws = _guarded(ops.scene_depth_workspace_bytes(n, views, width, height, 1), 0xA5)
    assert call(1, ws) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [-7, 2, -7] and cnt.tolist() == [-7, needed[views], -7]
    assert _intact(ws, 0xA5) and all(bool((t == 0x5A).all()) for t in outs.values()), "an output changed though the chunk did not fit"
    # ... and with room: the same call fills the outputs and still leaves every guard byte alone
    ws2 = _guarded(ops.scene_depth_workspace_bytes(n, views, width, height, needed[views]), 0xA5)
    assert call(needed[views], ws2) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [-7, 0, -7] and cnt.tolist() == [-7, needed[views], -7] and _intact(ws2, 0xA5)
    rgba = ops.raster_views(*args, cams, width, height, channels=4, background=RR.BACKGROUND)
    want = dict(a, image=rgba)          # (a: the last kind's, "expected" = points_kind 1)
    for k, t in outs.items():
        assert _intact(t, 0x5A), k
        assert torch.equal(t[256:-256].view(want[k].dtype).view(want[k].shape), want[k]), k


def test_null_outputs_the_empty_scene_and_argument_errors(ops, lib, syn):
    c, _, _, state = _run(ops, syn, DR.BIG)
    n, _, views, _, width, height, _ = DR.BIG
    cams = torch.from_numpy(np.ascontiguousarray(c["rows"])).cuda()
    full = ops.raster_depth(state, n, views, width, height, cams=cams, points="median")
    fwd, cap = state
    ws = torch.empty(ops.raster_depth_workspace_bytes(n, views, width, height, cap), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda outs, f=fwd.data_ptr(), fb=fwd.numel(), cm=cams.data_ptr(), kind=0, w=ws.data_ptr(), wb=ws.numel(), nn=n, vv=views: \
        lib.sixdgs_raster_depth(nn, vv, width, height, cap, f, fb, cm, *outs, kind, w, wb, stream, None)      # noqa: E731
    # NULL in any combination: what is asked for is what the full call gave
    for mask in itertools.product((False, True), repeat=len(ALL)):
        outs = {k: torch.full_like(full[k], 7) for k, m in zip(ALL, mask) if m}
        assert call([outs[k].data_ptr() if k in outs else None for k in ALL]) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(outs[k], full[k]) for k in outs), mask
    part = ops.raster_depth(state, n, views, width, height, want=("median_index",))
    assert set(part) == {"median_index"} and torch.equal(part["median_index"], full["median_index"])
    # no Gaussians: the values of a pixel with an empty list, over whatever the outputs held; guard bytes survive
    px = views * height * width
    held = {k: _guarded((12 if k == "points" else 4) * px, 0x5A) for k in ALL}
    assert call([held[k].data_ptr() + 256 for k in ALL], nn=0) == 0
    torch.cuda.synchronize()
    for k, t in held.items():
        body = t[256:-256].view(DTYPES[k])
        assert _intact(t, 0x5A) and bool((body == (-1 if k == "median_index" else 0)).all()), k
    # argument errors return without a launch: the outputs keep their pattern
    out = torch.full((views, height, width), 7.0, device="cuda")
    o = [out.data_ptr()] + [None] * 4
    pts = [None] * 4 + [out.data_ptr()]
    assert call(o, nn=-1) == -1 and call(o, vv=65536) == -1 and call(o, f=None) == -1 and call(o, fb=fwd.numel() // 2) == -2 and call(o, kind=2) == -1
    assert call(o, wb=ws.numel() - 1) == -2 and call(o, w=None) == -1 and call(o, w=ws.data_ptr() + 4) == -1 and call([out.data_ptr() + 2] + [None] * 4) == -1
    assert call(pts, cm=None) == -1 and call(o, cm=cams.data_ptr() + 2) == -1 and call(o, vv=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for bad in (dict(want=("depth",)), dict(points="median"), dict(points="mean", cams=cams), dict(points="median", cams=cams[:2])):
        with pytest.raises(ValueError):
            ops.raster_depth(state, n, views, width, height, **bad)
    with pytest.raises(ValueError):
        ops.raster_depth((fwd, 0), n, views, width, height)
    with pytest.raises(ValueError):
        ops.scene_depth_raw(*_dev(c["scene"]), cams, width, height, chunk=0)


def test_render_depth_and_surface_points_end_to_end(pkg, ops, syn):
    render = importlib.import_module("6dgs_amd.render")
    n, seed, views, cam_seed, width, height, _ = DR.BIG
    c = DR.case(syn, *DR.BIG)
    cameras = syn.make_cameras(views, cam_seed, width=width, height=height)
    assert np.array_equal(render.camera_rows(cameras), c["rows"])
    gs = pkg.GaussianScene.from_dict(c["scene"], device="cuda")
    cams = torch.from_numpy(np.ascontiguousarray(c["rows"])).cuda()
    raw = ops.scene_depth_raw(*_dev(c["scene"]), cams, width, height, points="expected")
    # kind="expected": expected / alpha where alpha > 0, else 0
    d = pkg.render_depth(gs, cameras, kind="expected", points=True, chunk=2, return_device=True)
    assert set(d) == {"depth", "alpha", "valid", "points"} and d["depth"].shape == (views, height, width)
    seen = raw["alpha"] > 0
    assert torch.equal(d["valid"], seen) and torch.equal(d["alpha"], raw["alpha"]) and torch.equal(d["points"], raw["points"])
    assert torch.equal(d["depth"][seen], (raw["expected"] / raw["alpha"])[seen]) and not bool(d["depth"][~seen].any()) and bool((~seen).any())
    host = pkg.render_depth(gs, cameras, kind="median")
    assert set(host) == {"depth", "alpha", "valid", "index"} and host["index"].dtype == np.int32 and host["valid"].dtype == bool
    med = ops.scene_depth_raw(*_dev(c["scene"]), cams, width, height, points="median")
    assert np.array_equal(host["depth"], med["median"].cpu().numpy()) and np.array_equal(host["index"], med["median_index"].cpu().numpy())
    assert np.array_equal(host["valid"], host["index"] >= 0)
    # cameras of two sizes: one entry per camera, each its own size's
    small = syn.make_cameras(1, 3, width=40, height=24)
    mixed = pkg.render_depth(gs, [cameras[0], small[0], cameras[1]], kind="median")
    assert [m.shape for m in mixed["depth"]] == [(height, width), (24, 40), (height, width)]
    assert np.array_equal(mixed["depth"][0], host["depth"][0]) and np.array_equal(mixed["depth"][2], host["depth"][1])
    # the surface cloud: every stride-th valid pixel with alpha >= min_alpha; the point lies in its Gaussian's tiles at its depth bits
    stride, min_alpha = 2, 0.6
    xyz, rgb, view, pixel = pkg.surface_points(gs, cameras, min_alpha=min_alpha, stride=stride, chunk=2, background=RR.BACKGROUND)
    keep = (med["median_index"] >= 0) & (med["alpha"] >= min_alpha)
    grid = torch.zeros_like(keep)
    grid[:, ::stride, ::stride] = True
    M = int((keep & grid).sum())
    assert xyz.shape == (M, 3) and rgb.shape == (M, 3) and rgb.dtype == torch.uint8 and view.dtype == torch.int32 and pixel.shape == (M, 2) and M > 100
    v, x, y = view.long(), pixel[:, 0].long(), pixel[:, 1].long()
    assert bool((x % stride == 0).all()) and bool((y % stride == 0).all()) and bool((keep & grid)[v, y, x].all())
    assert torch.equal(xyz, med["points"][v, y, x])
    assert torch.equal(rgb, ops.raster_views(*_dev(c["scene"]), cams, width, height, background=RR.BACKGROUND)[v, y, x])
    idx = med["median_index"][v, y, x].cpu().numpy().astype(np.int64)
    vh, xh, yh = v.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy()
    depth_bits = med["median"][v, y, x].cpu().numpy().view(np.uint32)
    assert np.array_equal(depth_bits, c["r32"]["z"][vh, idx].view(np.uint32))
    for k in range(views):
        on = vh == k
        P = RR.project(c["scene"], c["rows"][k], width, height, np.float32)
        rect = P["outer"][idx[on]]          # the rectangle with its undecidable edges taken outwards
        tx, ty = xh[on] // RR.TILE, yh[on] // RR.TILE
        assert ((tx >= rect[:, 0]) & (tx < rect[:, 2]) & (ty >= rect[:, 1]) & (ty < rect[:, 3])).all(), k
        m = c["rows"][k].astype(np.float64)
        pz = xyz[on].cpu().numpy().astype(np.float64) @ m[8:11] + m[11]
        assert np.abs(pz / med["median"][v, y, x].cpu().numpy()[on] - 1).max() <= 1e-5
    # ... and re-seeds a scene of M Gaussians that renders
    cloud = pkg.GaussianScene.from_points(xyz, rgb.float() / 255, sh_degree=0)
    assert len(cloud) == M
    shots = pkg.render_views(cloud, cameras[:2], renderer="raster")
    assert len(shots) == 2 and shots[0].image.shape == (height, width, 3)
