"""Pose refinement below the C ABI, without a GPU: the new entry points in the header, the binding and the library, what they answer
and refuse without a device; csrc/pose_step.h -- the per-view arithmetic the kernels of refine.hip run -- through its host
instantiation (libsixdgs_hostcheck.so) against the fp64 restatement (tests/pose_step_reference.py) under the restatement's own fp32
bound; the chain rule against fp64 autograd of refine.compose; Adam against torch.optim.Adam; the bookkeeping's rules; the target's
alpha modes on values worked by hand; the refusals of the new keyword arguments."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_step_reference as P  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_pose_compose", "sixdgs_pose_step", "sixdgs_refine_poses_workspace_bytes", "sixdgs_refine_poses")
STATE = ("delta", "m", "v", "rows", "best_loss", "best_step", "best_rows")


@pytest.fixture(scope="module")
def hc():
    return C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_compose(hc, start, delta):
    rows = np.zeros_like(start)
    hc.hc_ps_compose(_ptr(start), _ptr(delta), C.c_longlong(len(start)), _ptr(rows))
    return rows


def host_chain(hc, start, delta, d_rows):
    g = np.zeros((len(start), 6), np.float32)
    hc.hc_ps_chain(_ptr(start), _ptr(delta), _ptr(d_rows), C.c_longlong(len(start)), _ptr(g))
    return g


def host_step(hc, state, start, loss, d_rows, step, *, count=None, max_instances=1 << 30, evaluate_only=False, hyper=P.ADAM):
    """sixdgs_pose_step's per-view function on a float32 state dict (in place) -> the history row."""
    views = len(start)
    row = np.full(views, -7.0, np.float32)
    inst = None if count is None else np.array([count], np.int64)
    f = C.c_float
    hc.hc_ps_step(_ptr(start), _ptr(np.ascontiguousarray(loss, np.float32)), _ptr(d_rows), _ptr(inst), C.c_longlong(max_instances), views, step,
                  int(evaluate_only), f(hyper["lr"]), f(hyper["beta1"]), f(hyper["beta2"]), f(hyper["eps"]), *[_ptr(state[k]) for k in STATE],
                  _ptr(row), _ptr(state["status"]), _ptr(state["instances_needed"]))
    return row


def fresh(start):
    s = P.new_state(start, np.float32)
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def within(got, r64, r32, what):
    scale, y, limit = P.bounds({"x": r64}, {"x": r32})["x"]
    err = float(np.abs(np.asarray(got, np.float64) - r64).max())
    assert limit <= P.CEILING * scale, f"{what}: the case is unfit (bound {limit:.3e}, scale {scale:.3e})"
    assert np.isfinite(got).all() and err <= limit, f"{what}: {err:.3e} > {limit:.3e} (scale {scale:.3e}, y {y:.3e})"
    return err / limit


def _refine_call(L, **kw):
    """sixdgs_refine_poses on (never dereferenced) non-NULL addresses; every call made here is refused or has nothing to do."""
    a = dict(scene=256, n=10, sh_degree=0, n_coef=1, start=256, views=1, width=8, height=8, scale_modifier=1.0, background=256, target=256, is_u8=0,
             target_stride=3, lam=0.2, steps=3, lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_instances=100, out=256, delta=None, needed=256,
             ws=None, ws_bytes=0)
    a.update(kw)
    s, o = a["scene"], a["out"]
    return L.sixdgs_refine_poses(s, s, 1, s, s, 1, s, None if a["n_coef"] == 1 else s, a["sh_degree"], a["n_coef"], a["n"], a["start"], a["views"],
                                 a["width"], a["height"], a["scale_modifier"], a["background"], a["target"], a["is_u8"], a["target_stride"],
                                 a["lam"], a["steps"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["max_instances"], o, o, o, o, a["delta"], o,
                                 a["needed"], a["ws"], a["ws_bytes"], None)


def _step_call(L, **kw):
    a = dict(start=256, loss=256, d_rows=256, instances=None, max_instances=100, views=2, step=0, evaluate_only=0, lr=2e-3, beta1=0.9, beta2=0.999,
             eps=1e-8, state=512, rows=768, best_rows=1024, history=256, needed=256)
    a.update(kw)
    s = a["state"]
    return L.sixdgs_pose_step(a["start"], a["loss"], a["d_rows"], a["instances"], a["max_instances"], a["views"], a["step"], a["evaluate_only"],
                              a["lr"], a["beta1"], a["beta2"], a["eps"], s, s, s, a["rows"], s, s, a["best_rows"], a["history"], s, a["needed"], None)


def test_entry_points_in_header_binding_and_library():
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    ops = importlib.import_module("6dgs_amd.ops")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "refine.hip" in build.SOURCES and "pose_step.h" in build.HEADERS
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES] == [5, 23, 5, 37]
    so = C.CDLL(lib.LIB_PATH)                                              # a missing build fails here, it does not pass
    for name in NAMES:
        assert hasattr(so, name), f"{name} is not exported by the library"
    assert all(hasattr(ops, n) for n in ("pose_compose", "pose_step", "pose_state", "refine_poses_raw", "refine_poses_workspace_bytes"))
    L = lib.load()
    ws = L.sixdgs_refine_poses_workspace_bytes
    # answered without a GPU: the three parts' workspaces, two float images and the state
    parts = (L.sixdgs_raster_views_workspace_bytes(2000, 2, 64, 48, 5000) + L.sixdgs_raster_views_backward_workspace_bytes(2000, 2, 64, 48, 5000)
             + L.sixdgs_photometric_loss_workspace_bytes(2, 64, 48, 1))
    assert parts + 2 * 2 * 64 * 48 * 16 + 2 * 204 <= ws(2000, 2, 64, 48, 5000) <= parts + 2 * 2 * 64 * 48 * 16 + 2 * 204 + 13 * 256
    assert ws(2000, 4, 64, 48, 5000) > ws(2000, 2, 64, 48, 5000) > ws(2000, 2, 32, 48, 5000) > ws(1000, 2, 32, 48, 5000) > ws(1000, 2, 32, 48, 4000) > 0
    assert ws(0, 1, 8, 8, 1) > 0 and ws(10, 0, 8, 8, 1) > 0
    for bad in ((-1, 1, 8, 8, 10), (1 << 31, 1, 8, 8, 10), (10, -1, 8, 8, 10), (10, 65536, 8, 8, 10), (10, 1, 0, 8, 10), (10, 1, 8, 0, 10),
                (10, 1, 16385, 8, 10), (10, 1, 8, 16385, 10), (10, 1, 8, 8, 0), (10, 1, 8, 8, 1 << 31), (10, 65535, 16384, 16384, 10)):
        assert ws(*bad) == 0, bad
    assert ops.refine_poses_workspace_bytes(2000, 2, 64, 48, 5000) == ws(2000, 2, 64, 48, 5000)
    # sixdgs_refine_poses: refused without a launch
    for bad in (dict(n=-1), dict(views=-1), dict(views=65536), dict(width=0), dict(height=16385), dict(max_instances=0), dict(max_instances=1 << 31),
                dict(scale_modifier=0.0), dict(scale_modifier=float("inf")), dict(scale_modifier=float("nan")), dict(sh_degree=4), dict(sh_degree=1),
                dict(n_coef=17), dict(is_u8=2), dict(target_stride=2), dict(is_u8=1, target_stride=4), dict(lam=-0.1), dict(lam=1.5),
                dict(lam=float("nan")), dict(steps=0), dict(steps=-2), dict(lr=0.0), dict(lr=float("inf")), dict(lr=float("nan")), dict(beta1=1.0),
                dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1e-8), dict(eps=float("inf")), dict(start=None),
                dict(background=None), dict(target=None), dict(scene=None), dict(out=None), dict(needed=None), dict(start=258), dict(target=257),
                dict(out=130), dict(delta=2), dict(needed=260)):
        assert _refine_call(L, **bad) == -1, bad
    need = ws(10, 1, 8, 8, 100)
    assert _refine_call(L, ws=256, ws_bytes=need - 1) == -2 and _refine_call(L, ws_bytes=0) == -2           # SIXDGS_E_WORKSPACE
    assert _refine_call(L, ws_bytes=need) == -1 and _refine_call(L, ws=128, ws_bytes=need) == -1            # NULL or misaligned ws
    assert _refine_call(L, is_u8=1, target=257, ws_bytes=0) == -2                                           # a byte target needs no alignment
    assert _refine_call(L, views=0) == 0 and _refine_call(L, views=0, start=None, target=None, out=None, needed=None) == 0
    assert _refine_call(L, views=0, steps=0) == -1
    # sixdgs_pose_compose and sixdgs_pose_step
    assert L.sixdgs_pose_compose(None, None, 0, None, None) == 0
    for bad in ((None, 256, 1, 512), (256, None, 1, 512), (256, 512, 1, None), (256, 512, 1, 256), (256, 512, -1, 768), (256, 512, 65536, 768),
                (258, 512, 1, 768), (256, 513, 1, 768), (256, 512, 1, 770)):
        assert L.sixdgs_pose_compose(bad[0], bad[1], bad[2], bad[3], None) == -1, bad
    for bad in (dict(views=-1), dict(views=65536), dict(step=-1), dict(evaluate_only=2), dict(max_instances=0), dict(max_instances=1 << 31), dict(lr=0.0),
                dict(beta1=1.0), dict(beta2=-0.5), dict(eps=float("nan")), dict(start=None), dict(loss=None), dict(d_rows=None), dict(state=None),
                dict(rows=None), dict(best_rows=None), dict(history=None), dict(needed=None), dict(rows=256), dict(best_rows=768), dict(loss=258),
                dict(instances=260), dict(needed=260), dict(state=514)):
        assert _step_call(L, **bad) == -1, bad
    assert _step_call(L, views=0) == 0 and _step_call(L, views=0, start=None, state=None) == 0


@pytest.mark.parametrize("theta", P.THETAS)
def test_every_case_is_fit_and_the_host_instantiation_is_within_its_bound(hc, theta):
    """compose, the chain rule and five steps of Adam at this theta: fit under the ceiling, and csrc/pose_step.h on the host within
    max(8 y, 1e-6 scale) of fp64 -- the chosen evaluation of a, b, c stays inside the rule on both sides of the series threshold."""
    hc.hc_ps_series_below.restype = C.c_float
    assert float(hc.hc_ps_series_below()) == P.SERIES_BELOW
    worst = 0.0
    for seed in range(3):
        start, delta, d_rows = P.random_views(33, theta, 100 * seed + 1)
        x32 = P._theta2(delta[:, 3:])
        if theta in (1.0 - 1e-6, 1.0 + 1e-6):
            assert bool((x32 < 1.0).all()) == (theta < 1.0) and bool((x32 >= 1.0).all()) == (theta > 1.0)      # each side of the threshold is taken
        abc = np.zeros((len(x32), 3), np.float32)
        hc.hc_ps_coeffs(_ptr(np.ascontiguousarray(x32)), C.c_longlong(len(x32)), _ptr(abc))
        for i, name in enumerate("abc"):
            worst = max(worst, within(abc[:, i], P.coeffs(x32.astype(np.float64), np.float64)[i], P.coeffs(x32, np.float32)[i], f"{name} at {theta}"))
        worst = max(worst, within(host_compose(hc, start, delta), P.compose(start, delta, np.float64), P.compose(start, delta, np.float32), f"rows at {theta}"))
        worst = max(worst, within(host_chain(hc, start, delta, d_rows), P.chain(start, delta, d_rows, np.float64), P.chain(start, delta, d_rows, np.float32),
                                  f"chain at {theta}"))
        # steps 1 to 5 of Adam from this delta: the whole step (chain rule, Adam, compose) in all three arithmetics
        rng = np.random.default_rng(seed)
        got, s64, s32 = fresh(start), P.new_state(start, np.float64), P.new_state(start, np.float32)
        for s in (got, s64, s32):
            s["delta"] = delta.astype(s["delta"].dtype)
            s["rows"] = np.ascontiguousarray(P.compose(start, delta, s["rows"].dtype.type))
        for step in range(5):
            g = (d_rows * rng.uniform(0.5, 2.0, (len(start), 1)) * rng.choice([-1.0, 1.0], (len(start), 16))).astype(np.float32)
            loss = rng.random(len(start)).astype(np.float32)
            host_step(hc, got, start, loss, g, step)
            P.step(s64, start, loss, g, step, np.float64)
            P.step(s32, start, loss, g, step, np.float32)
            for k in ("delta", "m", "v", "rows"):
                worst = max(worst, within(got[k], s64[k], s32[k], f"{k} after step {step + 1} at {theta}"))
        assert not got["status"].any()
    print(f"theta {theta}: worst measured / bound {worst:.3f}")


def test_chain_rule_is_the_derivative_of_refine_compose():
    """The fp64 chain rule against fp64 autograd through refine.compose: 1e-9 of the scale for theta >= 1e-4."""
    refine = importlib.import_module("6dgs_amd.refine")
    for theta in (t for t in P.THETAS if t >= 1e-4):
        start, delta, d_rows = P.random_views(17, theta, 5)
        d = torch.from_numpy(delta).double().requires_grad_(True)
        rows = refine.compose(torch.from_numpy(start).double(), d)
        rows.backward(torch.from_numpy(d_rows).double())
        mine = P.chain(start, delta, d_rows, np.float64)
        assert np.abs(rows.detach().numpy() - P.compose(start, delta, np.float64)).max() <= 1e-9 * np.abs(start).max()
        assert np.abs(d.grad.numpy() - mine).max() <= 1e-9 * np.abs(mine).max(), theta


def test_adam_is_torch_optim_adam():
    rng = np.random.default_rng(3)
    grads = rng.standard_normal((5, 4, 6)) * 10.0 ** rng.uniform(-4, 1, (5, 4, 1))
    p = torch.zeros(4, 6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=P.ADAM["lr"])
    delta, m, v = (np.zeros((4, 6)) for _ in range(3))
    for step in range(5):
        p.grad = torch.from_numpy(grads[step])
        opt.step()
        delta, m, v = P.adam(grads[step], delta, m, v, step, np.float64, rounded=False)
        assert np.abs(p.detach().numpy() - delta).max() <= 1e-12, step
    assert np.abs(delta).max() > 5e-3                      # five steps of about lr each


def test_zero_delta_returns_the_start_bit_for_bit(hc):
    for seed in range(4):
        start, _, _ = P.random_views(65, 0.0, seed)
        zero = np.zeros((65, 6), np.float32)
        assert np.array_equal(host_compose(hc, start, zero).view(np.int32), start.view(np.int32))
        assert np.array_equal(P.compose(start, zero, np.float32).view(np.int32), start.view(np.int32))
        assert np.array_equal(fresh(start)["rows"].view(np.int32), start.view(np.int32))


def test_bookkeeping(hc):
    start, _, d_rows = P.random_views(3, 0.0, 9)
    nan = float("nan")
    for run in ("host", "restatement"):
        def step(s, loss, g, i, **kw):
            if run == "host":
                return host_step(hc, s, start, np.asarray(loss, np.float32), g, i, **kw)
            kw = dict(kw, count=kw.get("count") or 0)
            return P.step(s, start, np.asarray(loss, np.float32), g, i, np.float32, **kw).astype(np.float32)
        # the first minimum is kept on ties; step s evaluates iterate s; the evaluate-only step moves nothing
        s = fresh(start)
        rows_at = []
        for i, loss in enumerate(([0.5, 0.4, 0.3], [0.25, 0.4, 0.6], [0.25, 0.1, 0.3], [0.25, 0.1, 0.2])):
            rows_at.append(s["rows"].copy())
            last = i == 3
            before = {k: s[k].copy() for k in ("delta", "m", "v", "rows")}
            row = step(s, loss, None if last else d_rows, i, evaluate_only=last)
            assert np.array_equal(row, np.asarray(loss, np.float32))
            assert not last or all(np.array_equal(before[k], s[k]) for k in before)
            assert last or not np.array_equal(before["rows"], s["rows"])
        assert s["best_step"].tolist() == [1, 2, 3] and s["best_loss"].tolist() == [np.float32(0.25), np.float32(0.1), np.float32(0.2)]
        for v in range(3):
            assert np.array_equal(s["best_rows"][v], rows_at[s["best_step"][v]][v])
        assert not s["status"].any() and s["instances_needed"][0] == 0
        # a NaN loss, or a non-finite gradient entry among the 12, freezes that view alone and sets bit 0
        s = fresh(start)
        step(s, [0.5, 0.5, 0.5], d_rows, 0)
        frozen = {k: s[k].copy() for k in ("delta", "m", "v", "rows")}
        g = d_rows.copy()
        g[2, 7] = np.inf
        g[1, 13] = nan                                        # an intrinsics entry: ignored
        row = step(s, [nan, 0.4, 0.3], g, 1)
        assert np.isnan(row[0]) and row[1:].tolist() == [np.float32(0.4), np.float32(0.3)]
        assert s["status"].tolist() == [1, 0, 1] and s["best_step"].tolist() == [0, 1, 1]
        for k in frozen:
            assert np.array_equal(s[k][[0, 2]], frozen[k][[0, 2]]) and not np.array_equal(s[k][1], frozen[k][1]), k
        step(s, [0.1, 0.35, 0.2], d_rows, 2)                  # frozen views still record and track the best; they do not move
        assert s["best_step"].tolist() == [2, 2, 2] and s["status"].tolist() == [1, 0, 1]
        for k in frozen:
            assert np.array_equal(s[k][[0, 2]], frozen[k][[0, 2]]), k
        # over capacity: bit 1 everywhere, nothing of the step recorded, NaN history from then on, the largest count kept
        s = fresh(start)
        step(s, [0.5, 0.5, 0.5], d_rows, 0, count=90, max_instances=100)
        kept = {k: s[k].copy() for k in STATE}
        row = step(s, [0.1, 0.1, 0.1], d_rows, 1, count=101, max_instances=100)
        assert np.isnan(row).all() and s["status"].tolist() == [2, 2, 2] and s["instances_needed"][0] == 101
        row = step(s, [0.05, 0.05, 0.05], d_rows, 2, count=95, max_instances=100)         # a later step that would fit changes nothing
        assert np.isnan(row).all() and s["status"].tolist() == [2, 2, 2] and s["instances_needed"][0] == 101
        assert all(np.array_equal(kept[k], s[k]) for k in STATE) and s["best_step"].tolist() == [0, 0, 0]
        s = fresh(start)
        row = step(s, [0.5, 0.5, 0.5], d_rows, 0, count=1000, max_instances=64)            # at step 0: best_rows is the start
        assert np.isnan(row).all() and np.array_equal(s["best_rows"], start) and s["best_step"].tolist() == [0, 0, 0]
        assert np.isinf(s["best_loss"]).all() and s["instances_needed"][0] == 1000


def test_alpha_modes_of_the_target():
    refine = importlib.import_module("6dgs_amd.refine")
    img = torch.tensor([[[[255, 0, 51, 255], [255, 0, 51, 0]], [[100, 200, 50, 51], [0, 255, 102, 153]]]], dtype=torch.uint8)      # [1,2,2,4]
    same, ox, oy = refine.prepare_target(img, 1)
    again, _, _ = refine.prepare_target(img, 1, alpha="ignore")
    assert same.dtype == torch.uint8 and torch.equal(same, img[..., :3]) and torch.equal(again, same) and (ox, oy) == (0, 0)
    assert torch.equal(refine.prepare_target(img, 2)[0], refine.prepare_target(img, 2, "ignore")[0])
    white, ox, oy = refine.prepare_target(img, 1, alpha="composite")
    want = torch.tensor([[[[1.0, 0.0, 0.2], [1.0, 1.0, 1.0]],
                          [[100 / 255 * 0.2 + 0.8, 200 / 255 * 0.2 + 0.8, 50 / 255 * 0.2 + 0.8], [0.4, 0.6 + 0.4, 0.4 * 0.6 + 0.4]]]])
    assert white.dtype == torch.float32 and white.shape == (1, 2, 2, 3) and (ox, oy) == (0, 0) and torch.allclose(white, want, atol=1e-6, rtol=0)
    black = refine.prepare_target(img, 1, alpha="composite", background=(0.0, 0.5, 0.0))[0]
    want_b = torch.tensor([[[[1.0, 0.0, 0.2], [0.0, 0.5, 0.0]], [[100 / 255 * 0.2, 200 / 255 * 0.2 + 0.4, 50 / 255 * 0.2], [0.0, 0.6 + 0.2, 0.4 * 0.6]]]])
    assert torch.allclose(black, want_b, atol=1e-6, rtol=0)
    half = refine.prepare_target(img, 2, alpha="composite")[0]
    assert half.shape == (1, 1, 1, 3) and torch.allclose(half[0, 0, 0], want[0].reshape(4, 3).mean(0), atol=1e-6, rtol=0)
    # what test.prepare_image feeds the backbone
    image, _ = importlib.import_module("6dgs_amd.test").prepare_image(img[0].numpy(), "cpu")
    assert torch.allclose(white[0], image, atol=1e-6, rtol=0)
    # no fourth channel: both modes are the bytes
    assert torch.equal(refine.prepare_target(img[..., :3].contiguous(), 1, alpha="composite")[0], img[..., :3])


def test_backend_and_alpha_refuse_other_strings(syn):
    pkg = importlib.import_module("6dgs_amd")
    refine = importlib.import_module("6dgs_amd.refine")
    ops = importlib.import_module("6dgs_amd.ops")
    pea = importlib.import_module("6dgs_amd.pretrain_eval_attention")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    images, c2w, K = [np.zeros((8, 8, 4), np.uint8)] * 2, torch.eye(4)[None].repeat(2, 1, 1), torch.tensor([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    for bad in (dict(backend="hip"), dict(backend=""), dict(backend=None), dict(alpha="blend"), dict(alpha=None), dict(alpha=True)):
        with pytest.raises(ValueError):
            refine.refine_poses(scene, images, c2w, K, **bad)
    for bad in ("blend", "", None):
        with pytest.raises(ValueError):
            refine.prepare_target(torch.zeros(1, 2, 2, 4, dtype=torch.uint8), 1, alpha=bad)
    for backend in refine.BACKENDS:                                       # the good strings get as far as the scene's device
        with pytest.raises(RuntimeError):
            refine.refine_poses(scene, images, c2w, K, backend=backend, alpha="composite")
    assert refine.BACKENDS == ("torch", "fused") and refine.ALPHA_MODES == ("ignore", "composite")
    # the raw wrappers: no CPU fallback, and argument errors before anything is launched
    start = torch.zeros(2, 16)
    with pytest.raises(RuntimeError):
        ops.pose_compose(start, torch.zeros(2, 6))
    for bad in ((start[:, :12], torch.zeros(2, 6)), (start, torch.zeros(3, 6)), (start.double(), torch.zeros(2, 6)), (start, torch.zeros(2, 7))):
        with pytest.raises(ValueError):
            ops.pose_compose(*bad)
    t = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in syn.make_scene(10, 0).items() if k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")}
    args = (t["xyz"], t["log_scale"], t["rot"], t["opacity"], t["f_dc"], t["f_rest"], 0, start, 8, 8)
    target = torch.zeros(2, 8, 8, 3)
    with pytest.raises(RuntimeError):
        ops.refine_poses_raw(*args, target, steps=2)
    for bad in (dict(steps=0), dict(steps=1.5), dict(steps=2, lr=0.0), dict(steps=2, beta1=1.0), dict(steps=2, eps=-1.0), dict(steps=2, lambda_dssim=2.0),
                dict(steps=2, max_instances=0), dict(steps=2, background=(1.0,)), dict(steps=2, scale_modifier=0.0)):
        with pytest.raises(ValueError):
            ops.refine_poses_raw(*args, target, **bad)
    for bad_target in (target[:1], target.double(), torch.zeros(2, 8, 8, 4, dtype=torch.uint8), torch.zeros(2, 8, 9, 3), torch.zeros(2, 8, 8, 4)[..., :3]):
        with pytest.raises(ValueError):
            ops.refine_poses_raw(*args, bad_target, steps=2)
    # the sweep's flag: absent unless given, so the parsed namespace of an old command line is unchanged
    off, _ = pea.parse_args(["--exp_path", "e", "--out_path", "o"])
    on, _ = pea.parse_args(["--exp_path", "e", "--out_path", "o", "--refine_steps", "5", "--refine_backend", "fused"])
    assert not hasattr(off, "refine_backend") and on.refine_backend == "fused"
    with pytest.raises(SystemExit):
        pea.parse_args(["--exp_path", "e", "--out_path", "o", "--refine_backend", "hip"])
