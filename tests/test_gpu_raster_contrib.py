"""sixdgs_raster_contrib and sixdgs_scene_contrib on the GPU: against the numpy restatement of the definition (tests/contrib_reference.py)
-- counts EQUAL on cases without an undecidable decision, weight and peak within a bound taken from the restatement's own fp32 rounding
--, two identities that need no reference (conservation against the image's alpha; the backward's red-only gradient), hand cases, the
contract (determinism, batching, chunking, capacity, guard bytes, NULL outputs, argument errors) and the two consumers end to end:
pruning inert Gaussians leaves the renders byte-equal, and importance sampling emits from no Gaussian of zero importance.  Everything
runs inside this process."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrib_reference as CR  # noqa: E402
import raster_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ACCS = ("weight", "peak", "pixels", "stops", "seen")
BIG = (3000, 9, 5, 10, 96, 64)          # tests/test_gpu_raster.py's batching scene: Gaussians, scene seed, views, camera seed, width, height


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


def _dev(scene, sh_degree=None):
    return [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + \
        [int(scene["sh_degree"]) if sh_degree is None else sh_degree]


def _measure(ops, scene, rows, width, height, out=None, sh_degree=None, **kw):
    """One forward of the rows and the contribution pass on its state -> (contributions with the per-view rows, float image, state)."""
    cams = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    image, state = ops.raster_views(*_dev(scene, sh_degree), cams, width, height, want_float=True, want_u8=False, want_state=True, **kw)
    got = ops.raster_contrib(state, scene["xyz"].shape[0], rows.shape[0], width, height, out, want_views=True)
    return got, image, state


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if torch.is_tensor(v)}


def _big(syn):
    n, seed, views, cam_seed, width, height = BIG
    return syn.make_scene(n, seed), RR.camera_rows(syn.make_cameras(views, cam_seed, width=width, height=height)), width, height


def _identity_inputs(syn):
    """The fit cases and the larger scene: (name, scene, rows, width, height)."""
    for n, seed, views, cam_seed, width, height, deg in CR.CASES:
        c = CR.case(syn, n, seed, views, cam_seed, width, height, deg)
        yield f"n={n} {width}x{height} deg={deg}", c["scene"], c["rows"], width, height
    scene, rows, width, height = _big(syn)
    yield f"n={BIG[0]} {width}x{height}", scene, rows, width, height


@pytest.mark.parametrize("n,scene_seed,views,cam_seed,width,height,sh_degree", CR.CASES)
def test_counts_equal_and_weights_within_the_bound(ops, syn, n, scene_seed, views, cam_seed, width, height, sh_degree):
    c = CR.case(syn, n, scene_seed, views, cam_seed, width, height, sh_degree)
    assert not c["undecidable"].any() and c["decidable"].all(), "not a fit case: a discrete decision lies in its band"
    b = max(4.0 * c["rounding"], 1e-6)
    assert b <= 5e-5, "not a fit case"
    got, _, _ = _measure(ops, c["scene"], c["rows"], width, height)
    assert got["weight"].dtype == torch.float32 and got["peak"].dtype == torch.float32 and got["pixels"].dtype == torch.int64
    assert got["stops"].dtype == torch.int64 and got["seen"].dtype == torch.int32 and got["view_pixels"].dtype == torch.int32
    assert got["view_weight"].shape == (views, n) and got["view_pixels"].shape == (views, n)
    g, r64 = _np(got), c["r64"]
    for k in ("pixels", "stops", "seen", "view_pixels"):
        assert np.array_equal(g[k], r64[k]), f"{k} differs at {np.argwhere(g[k] != r64[k])[:4].tolist()}"
    assert np.array_equal((g["pixels"] == 0) & (g["stops"] == 0), r64["inert"])
    for k in ("weight", "peak", "view_weight"):
        dev = CR.deviation(g[k], r64[k])
        print(f"n={n} {width}x{height} deg={sh_degree} {k}: max |gpu - fp64| / max(1, fp64) {dev:.3e} (bound {b:.3e}, ratio {dev / b:.3f})")
        assert dev <= b, k
    assert r64["pixels"].sum() > 0 and (g["view_weight"][r64["view_pixels"] == 0] == 0).all()


def test_conservation_against_the_image_alpha(ops, syn):
    """Per view the contributions sum to the image's alpha: one rounding per T update and per product, all terms non-negative."""
    for name, scene, rows, width, height in _identity_inputs(syn):
        got, image, _ = _measure(ops, scene, rows, width, height)
        g, alpha = _np(got), image[..., 3].cpu().numpy().astype(np.float64)
        for v in range(rows.shape[0]):
            lhs, rhs = g["view_weight"][v].astype(np.float64).sum(), alpha[v].sum()
            limit = 2.0 ** -23 * (int(g["view_pixels"][v].astype(np.int64).sum()) + height * width)
            print(f"{name} view {v}: sum w {lhs:.6f}, sum alpha {rhs:.6f}, |diff| {abs(lhs - rhs):.3e} (bound {limit:.3e})")
            assert abs(lhs - rhs) <= limit, (name, v)


def test_the_backward_route_gives_the_same_weights(ops, syn):
    """Degree 0 with f_dc in [0, 1] -- the colour clamp cannot act --, one view at a time, grad_image = (1, 0, 0, 0): the backward's
    d f_dc[i, 0, 0] is C0 view_weight[v, i].  It rebuilds T by division, one rounding per list entry: relative (n + 16) 2^-23."""
    for name, scene, rows, width, height in _identity_inputs(syn):
        n = scene["xyz"].shape[0]
        scene = dict(scene, f_dc=np.random.default_rng(1).random((n, 1, 3)).astype(np.float32))
        args = _dev(scene, 0)
        grad = torch.zeros(1, height, width, 4, device="cuda")
        grad[..., 0] = 1.0
        tol, worst = (n + 16) * 2.0 ** -23, 0.0
        for v in range(rows.shape[0]):
            got, _, state = _measure(ops, scene, rows[v:v + 1], width, height, sh_degree=0)
            cams = torch.from_numpy(np.ascontiguousarray(rows[v:v + 1])).cuda()
            d = ops.raster_views_backward(*args, cams, width, height, grad, state, want=("f_dc",))[4]
            d, w = d[:, 0, 0].cpu().numpy().astype(np.float64), CR.C0 * got["view_weight"][0].cpu().numpy().astype(np.float64)
            assert np.array_equal(d == 0, w == 0), (name, v)
            on = w > 0
            rel = np.abs(d[on] - w[on]) / w[on]
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            assert (rel <= tol).all(), (name, v, float(rel.max()), tol)
        print(f"{name}: largest relative difference to the backward route {worst:.3e} (bound {tol:.3e})")


def _hand(ops, scene, row=CR.ROW, width=32, height=32):
    c = CR.pair(scene, row, width, height)
    assert not c["undecidable"].any(), "the reference reports an undecidable pixel: not a hand case"
    got, _, _ = _measure(ops, scene, row, width, height)
    return _np(got), c


def test_hand_cases(ops):
    # one isotropic Gaussian
    g, c = _hand(ops, CR.hand_one())
    r = c["r64"]
    assert g["pixels"][0] == r["pixels"][0] > 100 and g["stops"][0] == 0 and g["seen"][0] == 1
    assert CR.deviation(g["weight"], r["weight"]) <= CR.bound(c["rounding"])       # the fp64 sum of its alphas: T is 1 everywhere
    P = RR.project(CR.hand_one(), CR.ROW[0], 32, 32, np.float64)
    _, centre = RR._alpha(P, np.arange(1), np.array([16]), np.array([16]), np.float64)
    assert abs(g["peak"][0] - centre[0, 0]) <= 1e-6 and abs(r["weight"][0] - r["pixel_sum"].sum()) <= 1e-9
    # saturation: the third stops the middle pixels and is added by none of them; the fourth is not reached there
    g, c = _hand(ops, CR.hand_saturation())
    for k in ("pixels", "stops", "seen"):
        assert np.array_equal(g[k], c["r64"][k]), k
    assert g["stops"][2] >= 64 and g["stops"][[0, 1]].sum() == 0
    m_row = CR.ROW.copy()
    m_row[0, 14:] = 16.0 - 12.0                # the 8 x 8 middle pixels as an image of their own: (x, y) -> (x - 12, y - 12)
    gm, _ = _hand(ops, CR.hand_saturation(), m_row, 8, 8)
    assert gm["pixels"].tolist() == [64, 64, 0, 0] and gm["stops"].tolist() == [0, 0, 64, 0] and gm["weight"][2] == 0 and gm["weight"][3] == 0
    assert gm["peak"][3] == 0 and gm["seen"].tolist() == [1, 1, 0, 0]
    # behind the near plane, an empty rectangle, o < 1/255: all zeros, inert
    g, c = _hand(ops, CR.hand_nothing())
    assert not g["weight"].any() and not g["peak"].any() and not g["pixels"].any() and not g["stops"].any() and not g["seen"].any()
    assert not g["view_weight"].any() and not g["view_pixels"].any() and c["r64"]["inert"].all()
    # centred on the corner: only the pixels inside the image count
    g, c = _hand(ops, CR.hand_corner())
    shifted = CR.ROW.copy()
    shifted[0, 14:] = 32.0
    whole, _ = _hand(ops, CR.hand_corner(), shifted, 64, 64)
    assert g["pixels"][0] == c["r64"]["pixels"][0] and whole["pixels"][0] / 5 < g["pixels"][0] < whole["pixels"][0] / 3
    assert g["weight"][0] < whole["weight"][0] / 3 and g["peak"][0] <= whole["peak"][0]


def test_a_list_longer_than_one_round(ops):
    """700 copies of one wide Gaussian on a 24 x 16 image: three rounds; every pixel adds the first 302 and is stopped by the 303rd."""
    g, c = _hand(ops, CR.hand_long(), CR.ROW_LONG, 24, 16)
    k, r64 = CR.LONG_ADDS, c["r64"]
    assert (g["pixels"][:k] == 384).all() and (g["stops"][:k] == 0).all()          # 256 + 128: the right tile is half outside
    assert g["pixels"][k] == 0 and g["stops"][k] == 384 and g["weight"][k] == 0 and g["peak"][k] == 0
    for key in ACCS:
        assert not g[key][k + 1:].any(), key
    P = RR.project(CR.hand_long(), CR.ROW_LONG[0], 24, 16, np.float64)
    ys, xs = np.mgrid[0:16, 0:24]
    _, a = RR._alpha(P, np.arange(1), xs.reshape(-1), ys.reshape(-1), np.float64)
    want = (a[0][None, :] * (1 - a[0][None, :]) ** np.arange(k)[:, None]).sum(axis=1)
    b = CR.bound(c["rounding"])
    assert b <= RR.ERROR_CEILING and CR.deviation(g["weight"][:k], want) <= b and CR.deviation(g["weight"], r64["weight"]) <= b
    assert (g["seen"][:k] == 1).all()


def _equal(a, b, keys=ACCS):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _guarded(nbytes, fill, guard=256):
    return torch.full((nbytes + 2 * guard,), fill, dtype=torch.uint8, device="cuda")


def _intact(t, fill, guard=256):
    return bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all())


def test_determinism_batching_chunking_and_capacity(ops, lib, syn):
    scene, rows, width, height = _big(syn)
    n, views = BIG[0], BIG[2]
    a, _, state = _measure(ops, scene, rows, width, height)
    before = state[0].clone()
    b = ops.raster_contrib(state, n, views, width, height, want_views=True)
    assert _equal(a, b, ACCS + ("view_weight", "view_pixels")) and torch.equal(state[0], before), "not the same bytes, or fwd_ws was written"
    assert int(a["seen"].max()) <= views and int((a["pixels"] > 0).sum()) > 0 and int(a["stops"].sum()) >= 0
    # 5 views in one call, as 2 + 2 + 1 and one by one: the same bits in all five outputs (and per view)
    for cuts in ((2, 2, 1), (1, 1, 1, 1, 1)):
        acc, v0 = ops.contrib_state(n, "cuda"), 0
        for m in cuts:
            part, _, _ = _measure(ops, scene, rows[v0:v0 + m], width, height, out=acc)
            assert all(part[k] is acc[k] for k in ACCS)
            assert torch.equal(part["view_weight"], a["view_weight"][v0:v0 + m]) and torch.equal(part["view_pixels"], a["view_pixels"][v0:v0 + m])
            v0 += m
        assert _equal(acc, a), cuts
    # sixdgs_scene_contrib at chunk 1, 2 and 5 equals them; a capacity of 1 is retried with the needed one
    args = _dev(scene)
    cams = torch.from_numpy(rows).cuda()
    needed = {}
    for chunk in (1, 2, 5):
        s = ops.scene_contrib_raw(*args, cams, width, height, chunk=chunk, want_views=True)
        assert _equal(s, a, ACCS + ("view_weight", "view_pixels")) and int(s["status"]) == 0, chunk
        needed[chunk] = s["instances_needed"]
    counts = [ops.raster_views(*args, cams[v:v + 1], width, height, want_u8=False, want_instances=True) for v in range(views)]
    assert needed[1] == max(counts) and needed[5] == sum(counts) and needed[2] == max(counts[0] + counts[1], counts[2] + counts[3], counts[4])
    s = ops.scene_contrib_raw(*args, cams, width, height, chunk=2, max_instances=1)
    assert _equal(s, a) and s["max_instances"] == needed[2] and int(s["status"]) == 0
    s = ops.scene_contrib_raw(*args, cams, width, height, chunk=2, max_instances=1, retry=False)
    assert int(s["status"]) == 2 and s["instances_needed"] == needed[2] and not any(bool(s[k].any()) for k in ACCS)
    # capacity 1 through the C call: bit 1, the needed count, accumulators and per-view rows as they were, no guard byte written
    need = ops.scene_contrib_workspace_bytes(n, 5, width, height, 1)
    ws = _guarded(need, 0xA5)
    sizes = {"weight": 4 * n, "peak": 4 * n, "pixels": 8 * n, "stops": 8 * n, "seen": 4 * n, "view_weight": 4 * n * views, "view_pixels": 4 * n * views}
    outs = {k: _guarded(b_, 0x5A) for k, b_ in sizes.items()}
    flags = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda cap, w: lib.sixdgs_scene_contrib(p(args[0]), p(args[1]), 1, p(args[2]), p(args[3]), 1, p(args[4]), p(args[5]), 3, 16, n, p(cams),  # noqa: E731
                                                   views, width, height, 1.0, 5, cap, *[p(outs[k], 256) for k in sizes], p(flags, 4), p(cnt, 8),
                                                   p(w, 256), w.numel() - 512, stream)
    assert call(1, ws) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [-7, 2, -7] and cnt.tolist() == [-7, needed[5], -7]
    assert _intact(ws, 0xA5) and all(bool((t == 0x5A).all()) for t in outs.values()), "an output changed though the chunk did not fit"
    # ... and with room: the same call fills the pattern-free outputs and still leaves every guard byte alone
    for k, t in outs.items():
        t[256:-256] = 0
    ws2 = _guarded(ops.scene_contrib_workspace_bytes(n, 5, width, height, needed[5]), 0xA5)
    assert call(needed[5], ws2) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [-7, 0, -7] and cnt.tolist() == [-7, needed[5], -7] and _intact(ws2, 0xA5)
    for k, t in outs.items():
        assert _intact(t, 0x5A), k
        assert torch.equal(t[256:-256].view(a[k].dtype).view(a[k].shape), a[k]), k


def test_null_outputs_and_argument_errors(ops, lib, syn):
    scene, rows, width, height = _big(syn)
    n, views = BIG[0], BIG[2]
    full, _, state = _measure(ops, scene, rows, width, height)
    fwd, cap = state
    ws = torch.empty(ops.raster_contrib_workspace_bytes(n, views, width, height, cap), dtype=torch.uint8, device="cuda")
    names = ACCS + ("view_weight", "view_pixels")
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda outs, f=fwd.data_ptr(), fb=fwd.numel(), w=ws.data_ptr(), wb=ws.numel(), nn=n, vv=views: lib.sixdgs_raster_contrib(  # noqa: E731
        nn, vv, width, height, cap, f, fb, *outs, w, wb, stream, None)
    # NULL in any combination: what is asked for is what the full call gave
    for mask in itertools.product((False, True), repeat=len(names)):
        outs = {k: torch.zeros_like(full[k]) for k, m in zip(names, mask) if m}
        assert call([outs[k].data_ptr() if k in outs else None for k in names]) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(outs[k], full[k]) for k in outs), mask
    part = ops.raster_contrib(state, n, views, width, height, {"peak": torch.zeros(n, device="cuda")})
    assert set(part) == {"peak"} and torch.equal(part["peak"], full["peak"])
    # argument errors return without a launch: the outputs keep their pattern
    out = torch.full((n,), 7.0, device="cuda")
    o = [out.data_ptr()] + [None] * 6
    assert call(o, nn=-1) == -1 and call(o, vv=65536) == -1 and call(o, f=None) == -1 and call(o, fb=fwd.numel() // 2) == -2
    assert call(o, wb=ws.numel() - 256) == -2 and call(o, w=None) == -1 and call(o, w=ws.data_ptr() + 4) == -1 and call([out.data_ptr() + 2] + [None] * 6) == -1
    assert call(o, vv=0) == 0 and call(o, nn=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for bad in (dict(out={"weights": out}), dict(out={"weight": out.double()}), dict(out={"weight": out[:-1]})):
        with pytest.raises(ValueError):
            ops.raster_contrib(state, n, views, width, height, **bad)
    with pytest.raises(ValueError):
        ops.raster_contrib((fwd, 0), n, views, width, height)
    with pytest.raises(ValueError):
        ops.scene_contrib_raw(*_dev(scene), torch.from_numpy(rows).cuda(), width, height, chunk=0)


def test_pruning_inert_gaussians_leaves_the_renders_byte_equal(pkg, ops, syn):
    contribution = importlib.import_module("6dgs_amd.contribution")
    scene, rows, width, height = _big(syn)
    n = BIG[0]
    gs = pkg.GaussianScene.from_dict(scene, device="cuda")
    w2c = np.tile(np.eye(4, dtype=np.float32), (rows.shape[0], 1, 1))
    w2c[:, :3, :] = rows[:, :12].reshape(-1, 3, 4)
    K = np.tile(np.eye(3, dtype=np.float32), (rows.shape[0], 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15]
    c2w = np.linalg.inv(w2c)
    contrib = pkg.scene_contribution(gs, c2w, K, width, height, chunk=2, per_view=True)
    assert int(contrib["status"]) == 0 and torch.equal(contrib["inert"], (contrib["pixels"] == 0) & (contrib["stops"] == 0))
    assert contrib["view_weight"].shape == (rows.shape[0], n) and contrib["inert"].dtype == torch.bool
    before = [getattr(gs, k).clone() for k in ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")]
    pruned, keep = pkg.prune_by_contribution(gs, contrib, drop_inert=True)
    removed = n - len(pruned)
    print(f"{removed} of {n} Gaussians are inert for the {rows.shape[0]} views ({100.0 * removed / n:.1f} %)")
    assert removed >= 1 and torch.equal(keep, ~contrib["inert"]) and len(pruned) == int(keep.sum())
    assert all(torch.equal(getattr(gs, k), t) for k, t in zip(("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity"), before))
    cams = contribution.camera_rows(c2w, K).cuda()

    def render(s):
        return ops.raster_views(s._xyz, s._scaling, s._rotation, s._opacity, s._features_dc, s._features_rest, int(s.active_sh_degree), cams, width,
                                height, channels=4, background=RR.BACKGROUND, want_float=True)

    full_f, full_u = render(gs)
    sub_f, sub_u = render(pruned)
    assert torch.equal(sub_f, full_f) and torch.equal(sub_u, full_u), "a pruned-inert scene rendered to other bytes"
    assert float(full_f[..., 3].max()) > 0.5
    # the survivors' contributions are what they were
    again = pkg.scene_contribution(pruned, c2w, K, width, height)
    assert all(torch.equal(again[k], contrib[k][keep]) for k in ACCS) and not bool(again["inert"].any())


def test_importance_selects_the_emitting_gaussians(pkg, ops, syn):
    scene, rows, width, height = _big(syn)
    n = BIG[0]
    gs = pkg.GaussianScene.from_dict(scene, device="cuda")
    got, _, _ = _measure(ops, scene, rows, width, height)
    weight = got["weight"]
    valid = ops.mask_degraded(gs._scaling, 50).bool()
    cand = torch.nonzero(valid & (weight > 0))[:, 0]
    assert 0 < cand.numel() < int(valid.sum())
    torch.manual_seed(3)
    for kw in (dict(), dict(max_ellipsoids=200), dict(max_ellipsoids=None), dict(emitter="isocell", rays_per_ellipsoid=16, max_ellipsoids=300)):
        ori, dr, rgb, src = pkg.generate_all_possible_rays(gs, importance=weight, return_src=True, **kw)
        used = torch.unique(src)
        assert ori.shape[0] == src.shape[0] > 0 and bool((weight[used] > 0).all()) and bool(valid[used].all()), kw
        limit = kw.get("max_ellipsoids", 1000)
        assert used.numel() <= (cand.numel() if limit is None else min(limit, cand.numel())), kw
    _, _, _, src = pkg.generate_all_possible_rays(gs, importance=weight, return_src=True, max_ellipsoids=None)
    assert bool(torch.isin(torch.unique(src), cand).all()) and torch.unique(src).numel() > 0.5 * cand.numel()
    # a given perm indexes the candidate list; the draw favours heavy Gaussians
    perm = torch.arange(cand.numel() - 1, -1, -1, device="cuda")
    _, _, _, src = pkg.generate_all_possible_rays(gs, importance=weight, return_src=True, max_ellipsoids=50, perm=perm)
    assert bool(torch.isin(torch.unique(src), cand[-50:]).all())
    torch.manual_seed(4)
    _, _, _, src = pkg.generate_all_possible_rays(gs, importance=weight, return_src=True, max_ellipsoids=100)
    assert float(weight[torch.unique(src)].mean()) > float(weight[cand].mean())
    # importance=None with a fixed perm: the same tensors as without the keyword
    perm = torch.randperm(int(valid.sum()), generator=torch.Generator().manual_seed(5)).cuda()
    a = pkg.generate_all_possible_rays(gs, perm=perm, return_src=True)
    b = pkg.generate_all_possible_rays(gs, perm=perm, return_src=True, importance=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool(torch.isin(torch.unique(a[3]), torch.nonzero(valid)[:, 0][perm[:1000]]).all())
    for bad in (weight[:-1], -weight, weight > 0):
        with pytest.raises(ValueError):
            pkg.generate_all_possible_rays(gs, importance=bad)
