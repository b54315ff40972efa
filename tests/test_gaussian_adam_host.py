"""Fitting a scene's Gaussians below the C ABI, without a GPU: the fp64 restatement (tests/gaussian_adam_reference.py) against
torch.optim.Adam; csrc/adam_step.h -- the per-entry arithmetic the kernels of fit.hip run -- through its host instantiation
(libsixdgs_hostcheck.so) under the restatement's own fp32 bound; fit.position_lr and the reset against the reference's numbers
(tests/golden/g15_fit.npz); the default schedule; fit_scene's refusals; what the three entry points answer and refuse without a
device."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussian_adam_reference as R  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_gaussian_adam", "sixdgs_opacity_reset", "sixdgs_fit_scene_workspace_bytes", "sixdgs_fit_scene")


@pytest.fixture(scope="module")
def hc():
    return C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_adam(hc, params, grads, m, v, step, lrs=R.LRS, hyper=R.HYPER):
    """sixdgs_gaussian_adam's per-entry function over float32 arrays (in place) -> the status bits."""
    n = params["xyz"].size // 3
    n_coef = 1 + params["f_rest"].size // (3 * n)
    P = (C.c_void_p * 6)(*[_ptr(params[k]) for k in R.GROUPS])
    G = (C.c_void_p * 6)(*[_ptr(grads.get(k)) for k in R.GROUPS])
    f = C.c_float
    return hc.hc_ga_adam(C.c_longlong(n), n_coef, step, P, G, _ptr(m), _ptr(v), _ptr(np.asarray(lrs, np.float32)), f(hyper["beta1"]), f(hyper["beta2"]),
                         f(hyper["eps"]))


def within(got, r64, r32, what):
    scale, y, limit = R.bounds({"x": r64}, {"x": r32})["x"]
    err = float(np.abs(np.asarray(got, np.float64) - r64).max())
    assert limit <= R.CEILING * scale, f"{what}: the case is unfit (bound {limit:.3e}, scale {scale:.3e})"
    assert np.isfinite(got).all() and err <= limit, f"{what}: {err:.3e} > {limit:.3e} (scale {scale:.3e}, y {y:.3e})"
    return err / limit


def test_fp64_restatement_is_torch_optim_adam():
    """Six groups with six different rates, three steps, eps = 1e-15: 1e-12 of the scale, against something that is not ours."""
    n, n_coef = 37, 4
    params, _, _, grads = R.random_case(n, n_coef, 1)
    tp = {k: torch.from_numpy(params[k].astype(np.float64)).requires_grad_(True) for k in R.GROUPS}
    opt = torch.optim.Adam([{"params": [tp[k]], "lr": lr} for k, lr in zip(R.GROUPS, R.LRS)], lr=0.0, betas=(R.HYPER["beta1"], R.HYPER["beta2"]),
                           eps=R.HYPER["eps"])
    p = {k: a.astype(np.float64) for k, a in params.items()}
    m, v = np.zeros(n * (11 + 3 * n_coef)), np.zeros(n * (11 + 3 * n_coef))
    for step, g in enumerate(grads):
        for k in R.GROUPS:
            tp[k].grad = torch.from_numpy(g[k].astype(np.float64))
        opt.step()
        assert R.adam_step(p, g, m, v, step, R.LRS, np.float64, rounded=False) == 0
        for k in R.GROUPS:
            assert np.abs(tp[k].detach().numpy() - p[k]).max() <= 1e-12 * np.abs(p[k]).max(), (k, step)
    sl = R.slices(n, n_coef)
    for k in R.GROUPS:
        state = opt.state[tp[k]]
        assert np.abs(state["exp_avg"].numpy() - m[sl[k]]).max() <= 1e-12 * np.abs(m[sl[k]]).max(), k
        assert np.abs(state["exp_avg_sq"].numpy() - v[sl[k]]).max() <= 1e-12 * np.abs(v[sl[k]]).max(), k
        assert np.abs(p[k] - params[k]).max() > 0.5 * R.LRS[R.GROUPS.index(k)]          # every group moved by about its rate per step


@pytest.mark.parametrize("n,n_coef", ((1, 1), (65, 4), (257, 16)))
def test_host_instantiation_is_within_its_bound(hc, n, n_coef):
    params, m, v, grads = R.random_case(n, n_coef, 2)
    got = {k: a.copy() for k, a in params.items()}
    gm, gv = m.copy(), v.copy()
    for step, g in enumerate(grads):
        assert host_adam(hc, got, g, gm, gv, step) == 0
    p64, m64, v64, _ = R.run(params, m, v, grads, np.float64)
    p32, m32, v32, _ = R.run(params, m, v, grads, np.float32)
    worst = max(within(gm, m64, m32, "m"), within(gv, v64, v32, "v"))
    for k in R.GROUPS:
        if got[k].size:
            worst = max(worst, within(got[k], p64[k], p32[k], k))
            assert not np.array_equal(got[k], params[k]), k
    print(f"n {n}, n_coef {n_coef}: worst measured / bound {worst:.3f}")


def test_host_rules_frozen_group_not_finite_entry_and_zero_rate(hc):
    n, n_coef = 33, 4
    params, m, v, grads = R.random_case(n, n_coef, 3, steps=1)
    sl = R.slices(n, n_coef)
    # a frozen group: its parameters and its slices of m and v keep their bits; the others move
    g = dict(grads[0], scale=None)
    got, gm, gv = {k: a.copy() for k, a in params.items()}, m.copy(), v.copy()
    assert host_adam(hc, got, g, gm, gv, 0) == 0
    for k in R.GROUPS:
        same = [np.array_equal(got[k].view(np.int32), params[k].view(np.int32)), np.array_equal(gm[sl[k]].view(np.int32), m[sl[k]].view(np.int32)),
                np.array_equal(gv[sl[k]].view(np.int32), v[sl[k]].view(np.int32))]
        assert all(same) if k == "scale" else not any(same), k
    # entries whose gradient is not finite keep p, m and v and set bit 0; every other entry is the run without the plant
    g = {k: a.copy() for k, a in grads[0].items()}
    g["xyz"][5], g["rot"][7], g["f_rest"][0] = np.inf, np.nan, -np.inf
    planted, pm, pv = {k: a.copy() for k, a in params.items()}, m.copy(), v.copy()
    assert host_adam(hc, planted, g, pm, pv, 0) == R.STATUS_NOT_FINITE
    clean, cm, cv = {k: a.copy() for k, a in params.items()}, m.copy(), v.copy()
    host_adam(hc, clean, grads[0], cm, cv, 0)
    for k, i in (("xyz", 5), ("rot", 7), ("f_rest", 0)):
        for arr, src in ((clean[k], params[k]), (cm[sl[k]], m[sl[k]]), (cv[sl[k]], v[sl[k]])):
            arr[i] = src[i]
    assert all(np.array_equal(planted[k], clean[k]) for k in R.GROUPS) and np.array_equal(pm, cm) and np.array_equal(pv, cv)
    r32 = R.run(params, m, v, [g], np.float32)
    assert r32[3] == R.STATUS_NOT_FINITE and all(np.array_equal(r32[0][k][i], params[k][i]) for k, i in (("xyz", 5), ("rot", 7), ("f_rest", 0)))
    # a zero rate still updates m and v, and leaves p
    lrs = list(R.LRS)
    lrs[3] = 0.0
    got, gm, gv = {k: a.copy() for k, a in params.items()}, m.copy(), v.copy()
    assert host_adam(hc, got, grads[0], gm, gv, 0, lrs=lrs) == 0
    assert np.array_equal(got["opacity"], params["opacity"]) and not np.array_equal(gm[sl["opacity"]], m[sl["opacity"]])
    assert not np.array_equal(gv[sl["opacity"]], v[sl["opacity"]]) and not np.array_equal(got["xyz"], params["xyz"])


def test_position_rate_and_reset_against_the_reference_numbers(hc, golden):
    fit = importlib.import_module("6dgs_amd.fit")
    g = golden("g15_fit")
    init, final, delay_mult, max_steps = g["position_lr_args"]
    assert (init, final, delay_mult, int(max_steps)) == (1.6e-4, 1.6e-6, 0.01, 30000) and g["iterations"].tolist() == [1, 2, 100, 1000, 15000, 30000, 40000]
    for i, scale in enumerate(g["spatial_lr_scales"]):
        mine = np.array([fit.position_lr(int(it), init, final, int(max_steps), float(scale), delay_mult) for it in g["iterations"]])
        assert np.abs(mine / g["position_lr"][i] - 1.0).max() <= 1e-12, scale
    assert fit.position_lr(1) == fit.position_lr(1, 1.6e-4, 1.6e-6, 30000, 1.0, 0.01) and fit.position_lr(30000) == pytest.approx(1.6e-6, rel=1e-12)
    assert fit.position_lr(-1) == 0.0 and fit.position_lr(5, 0.0, 0.0) == 0.0
    # the reset: the fp64 restatement is the reference's numbers; the host instantiation and the torch arm's reset within the fp32 bound
    logits, ceiling = g["logits"], float(g["reset_ceiling"])
    assert logits.shape == (64,) and logits[0] == -12.0 and logits[-1] == 12.0
    r64 = R.reset(logits, ceiling, np.float64)
    assert np.abs(r64 - g["reset"]).max() <= 1e-12 * np.abs(g["reset"]).max()
    x32 = logits.astype(np.float32)
    r32 = R.reset(x32, ceiling, np.float32)
    got = x32.copy()
    hc.hc_ga_reset(_ptr(got), C.c_longlong(got.size), 1, C.c_float(ceiling))
    within(got, R.reset(x32.astype(np.float64), ceiling, np.float64), r32, "reset on the host")
    t = torch.from_numpy(x32.copy())
    fit.reset_opacity_(t, ceiling)
    within(t.numpy(), R.reset(x32.astype(np.float64), ceiling, np.float64), r32, "reset of the torch arm")
    assert got.max() <= np.log(ceiling / (1 - ceiling)) + 1e-5 and got[0] == pytest.approx(-12.0, abs=1e-4)
    plain = np.float32([0.0, 0.005, 0.01, 0.5, 1.0])
    hc.hc_ga_reset(_ptr(plain), C.c_longlong(plain.size), 0, C.c_float(ceiling))
    assert plain.tolist() == [0.0, np.float32(0.005), np.float32(0.01), np.float32(0.01), np.float32(0.01)]


def test_default_schedule_visits_every_view_once_per_pass():
    fit = importlib.import_module("6dgs_amd.fit")
    for n_views, steps, batch in ((5, 15, 1), (7, 10, 2), (3, 4, 3), (1, 3, 1)):
        s = fit.default_schedule(n_views, steps, batch, seed=4)
        assert s.shape == (steps, batch) and s.dtype == np.int32
        flat = s.reshape(-1)
        for p0 in range(0, flat.size - n_views + 1, n_views):
            assert sorted(flat[p0:p0 + n_views].tolist()) == list(range(n_views)), p0
        assert len(set(flat[flat.size - flat.size % n_views:].tolist())) == flat.size % n_views
        assert np.array_equal(s, fit.default_schedule(n_views, steps, batch, seed=4))
    assert not np.array_equal(fit.default_schedule(7, 14, 1, seed=0), fit.default_schedule(7, 14, 1, seed=1))


def test_fit_scene_refuses_bad_arguments(syn):
    pkg = importlib.import_module("6dgs_amd")
    fit = importlib.import_module("6dgs_amd.fit")
    assert pkg.fit_scene is fit.fit_scene and fit.GROUPS == ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    images, c2w, K = [np.zeros((8, 8, 3), np.uint8)] * 2, torch.eye(4)[None].repeat(2, 1, 1), torch.tensor([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    for bad in (dict(steps=0), dict(steps=1.5), dict(steps=True), dict(batch=0), dict(backend="hip"), dict(backend=None), dict(groups=()),
                dict(groups=("xyz", "colour")), dict(groups=("xyz", "xyz")), dict(groups=5), dict(position_lr_init=-1.0), dict(position_lr_final=float("inf")),
                dict(position_lr_init=0.0), dict(position_lr_max_steps=0), dict(spatial_lr_scale=float("nan")), dict(feature_lr=-1e-3), dict(opacity_lr=float("inf")),
                dict(scaling_lr=-1.0), dict(rotation_lr=float("nan")), dict(eps=-1e-15), dict(lambda_dssim=1.5), dict(lambda_dssim=-0.1), dict(sh_degree_start=4),
                dict(sh_degree_start=-1), dict(sh_up_every=0), dict(opacity_reset_every=-1), dict(reset_ceiling=0.0), dict(reset_ceiling=1.0),
                dict(downscale=0), dict(downscale=1.5), dict(alpha="blend"), dict(background=(1.0, 1.0)), dict(seed=-1), dict(schedule=[[0], [2], [1]]),
                dict(schedule=[[0, 1]] * 3), dict(schedule=[[0.0], [1.0], [1.0]]), dict(schedule=[[0], [1]])):
        kw = dict(dict(steps=3), **bad)
        with pytest.raises(ValueError):
            fit.fit_scene(scene, images, c2w, K, **kw)
    for bad_call in ((scene, images[:1], c2w, K), (scene, images, c2w[:, :3], K), (scene, images, c2w, K[:2]), (scene, images, c2w * float("nan"), K),
                     ("scene", images, c2w, K)):
        with pytest.raises(ValueError):
            fit.fit_scene(*bad_call, steps=3)
    for backend in ("torch", "fused"):                                  # good arguments get as far as the scene's device
        with pytest.raises(RuntimeError):
            fit.fit_scene(scene, images, c2w, K, steps=3, backend=backend, schedule=[[0], [1], [1]])


def _adam_call(L, **kw):
    """sixdgs_gaussian_adam on (never dereferenced) non-NULL addresses; every call made here is refused or has nothing to do."""
    a = dict(n=10, n_coef=4, step=0, p=256, f_rest=256, g=512, d_f_rest=512, m=1024, v=2048, lr=R.LRS, beta1=0.9, beta2=0.999, eps=1e-15, instances=None,
             max_instances=100, status=256)
    a.update(kw)
    lr = None if a["lr"] is None else (C.c_float * 6)(*a["lr"])
    p, g = a["p"], a["g"]
    return L.sixdgs_gaussian_adam(a["n"], a["n_coef"], a["step"], p, p, a["f_rest"], p, p, p, g, g, a["d_f_rest"], g, g, g, a["m"], a["v"], lr, a["beta1"],
                                  a["beta2"], a["eps"], a["instances"], a["max_instances"], a["status"], None)


def _fit_call(L, **kw):
    a = dict(scene=256, f_rest=256, n_coef=4, n=10, cams=256, views=3, width=8, height=8, scale_modifier=1.0, background=256, target=256, is_u8=0,
             target_stride=3, lam=0.2, steps=2, batch=1, view=[0, 2], lr=[R.LRS, R.LRS], degree=[0, 1], reset=[0, 1], mask=63, beta1=0.9, beta2=0.999,
             eps=1e-15, ceiling=0.01, max_instances=100, m=1024, v=2048, out=256, needed=256, ws=None, ws_bytes=0, logit=1)
    a.update(kw)
    s = a["scene"]
    view = None if a["view"] is None else np.asarray(a["view"], np.int32)
    lr = None if a["lr"] is None else np.asarray(a["lr"], np.float32)
    degree = None if a["degree"] is None else np.asarray(a["degree"], np.int32)
    reset = None if a["reset"] is None else np.asarray(a["reset"], np.uint8)
    return L.sixdgs_fit_scene(s, s, 1, s, s, a["logit"], s, a["f_rest"], a["n_coef"], a["n"], a["cams"], a["views"], a["width"], a["height"],
                              a["scale_modifier"], a["background"], a["target"], a["is_u8"], a["target_stride"], a["lam"], a["steps"], a["batch"], _ptr(view),
                              _ptr(lr), _ptr(degree), _ptr(reset), a["mask"], a["beta1"], a["beta2"], a["eps"], a["ceiling"], a["max_instances"], a["m"],
                              a["v"], a["out"], a["out"], a["needed"], a["ws"], a["ws_bytes"], None)


def test_entry_points_in_header_binding_and_library():
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    ops = importlib.import_module("6dgs_amd.ops")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "fit.hip" in build.SOURCES and "adam_step.h" in build.HEADERS and lib.ABI_VERSION == 10
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES] == [25, 7, 6, 40]
    so = C.CDLL(lib.LIB_PATH)                                              # a missing build fails here, it does not pass
    for name in NAMES:
        assert hasattr(so, name), f"{name} is not exported by the library"
    assert all(hasattr(ops, n) for n in ("gaussian_adam", "gaussian_adam_state", "opacity_reset", "fit_scene_raw", "fit_scene_workspace_bytes"))
    L = lib.load()
    ws = L.sixdgs_fit_scene_workspace_bytes
    # answered without a GPU: the three parts' workspaces at `batch` views, two float images, the gathered rows and targets, the loss,
    # the count and the six gradient arrays, each rounded to 256 B
    n, nc, batch, w, h, cap = 2000, 16, 3, 64, 48, 5000
    parts = (L.sixdgs_raster_views_workspace_bytes(n, batch, w, h, cap) + L.sixdgs_raster_views_backward_workspace_bytes(n, batch, w, h, cap)
             + L.sixdgs_photometric_loss_workspace_bytes(batch, w, h, 1))
    exact = parts + 3 * batch * w * h * 16 + batch * 64 + batch * 4 + 8 + n * (11 + 3 * nc) * 4
    assert exact <= ws(n, nc, batch, w, h, cap) <= exact + 15 * 256 and ws(n, nc, batch, w, h, cap) % 256 == 0
    assert ws(n, nc, 4, w, h, cap) > ws(n, nc, 3, w, h, cap) > ws(n, 4, 3, w, h, cap) > ws(n, 4, 3, 32, h, cap) > ws(1000, 4, 3, 32, h, cap) > ws(1000, 4, 3, 32, h, 4000) > 0
    assert ws(0, 1, 1, 8, 8, 1) > 0
    for bad in ((-1, 4, 1, 8, 8, 10), (1 << 31, 4, 1, 8, 8, 10), (10, 0, 1, 8, 8, 10), (10, 17, 1, 8, 8, 10), (10, 4, 0, 8, 8, 10), (10, 4, 65536, 8, 8, 10),
                (10, 4, 1, 0, 8, 10), (10, 4, 1, 8, 16385, 10), (10, 4, 1, 8, 8, 0), (10, 4, 1, 8, 8, 1 << 31)):
        assert ws(*bad) == 0, bad
    assert ops.fit_scene_workspace_bytes(n, nc, batch, w, h, cap) == ws(n, nc, batch, w, h, cap)
    # sixdgs_fit_scene: refused without a launch
    for bad in (dict(n=-1), dict(n_coef=0), dict(n_coef=17), dict(views=0), dict(views=65536), dict(width=0), dict(height=16385), dict(max_instances=0),
                dict(max_instances=1 << 31), dict(scale_modifier=0.0), dict(scale_modifier=float("nan")), dict(is_u8=2), dict(target_stride=2),
                dict(is_u8=1, target_stride=4), dict(lam=-0.1), dict(lam=float("nan")), dict(steps=0), dict(batch=0), dict(view=[0, 3]), dict(view=[-1, 0]),
                dict(view=None), dict(lr=None), dict(degree=None), dict(reset=None), dict(lr=[R.LRS, (-1.0,) * 6]), dict(lr=[R.LRS, (float("inf"),) * 6]),
                dict(lr=[(float("nan"),) * 6, R.LRS]), dict(degree=[0, 2]), dict(degree=[-1, 0]), dict(degree=[0, 4], n_coef=16), dict(logit=0),
                dict(logit=2), dict(mask=0), dict(mask=64), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("inf")), dict(eps=-1.0), dict(ceiling=0.0),
                dict(ceiling=1.0), dict(ceiling=float("nan")), dict(scene=None), dict(f_rest=None), dict(cams=None), dict(background=None), dict(target=None),
                dict(m=None), dict(v=None), dict(v=1024), dict(out=None), dict(needed=None), dict(scene=258), dict(cams=257), dict(target=258), dict(m=1026),
                dict(out=130), dict(needed=260)):
        assert _fit_call(L, **bad) == -1, bad
    need = ws(10, 4, 1, 8, 8, 100)
    assert _fit_call(L, ws=256, ws_bytes=need - 1) == -2 and _fit_call(L, ws_bytes=0) == -2                # SIXDGS_E_WORKSPACE
    assert _fit_call(L, ws_bytes=need) == -1 and _fit_call(L, ws=128, ws_bytes=need) == -1                 # NULL or misaligned ws
    assert _fit_call(L, logit=0, reset=[0, 0], ws_bytes=0) == -2 and _fit_call(L, n_coef=1, f_rest=None, degree=[0, 0], ws_bytes=0) == -2
    assert _fit_call(L, is_u8=1, target=257, ws_bytes=0) == -2                                             # a byte target needs no alignment
    assert _fit_call(L, batch=2, view=[0, 1, 2, 2], ws_bytes=0) == -2 and _fit_call(L, batch=2, view=[0, 1, 2, 3], ws_bytes=0) == -1
    # sixdgs_gaussian_adam
    for bad in (dict(n=-1), dict(n=1 << 31), dict(n_coef=0), dict(n_coef=17), dict(step=-1), dict(lr=None), dict(lr=(-1.0,) + R.LRS[1:]),
                dict(lr=R.LRS[:5] + (float("inf"),)), dict(lr=(float("nan"),) * 6), dict(beta1=1.0), dict(beta1=-0.5), dict(beta2=1.0),
                dict(beta2=float("nan")), dict(eps=-1.0), dict(eps=float("inf")), dict(max_instances=0), dict(max_instances=1 << 31), dict(m=None),
                dict(v=None), dict(status=None), dict(v=1024), dict(p=None), dict(f_rest=None), dict(p=258), dict(g=514), dict(m=1026), dict(v=2050),
                dict(status=258), dict(instances=260)):
        assert _adam_call(L, **bad) == -1, bad
    assert _adam_call(L, n=0) == 0 and _adam_call(L, n=0, p=None, g=None, m=None, v=None, status=None) == 0 and _adam_call(L, n=0, lr=None) == -1
    # sixdgs_opacity_reset
    assert L.sixdgs_opacity_reset(None, 0, 1, None, None, 0.01, None) == 0
    for bad in ((None, 5, 1, 512, 768, 0.01), (256, -1, 1, 512, 768, 0.01), (256, 1 << 31, 1, 512, 768, 0.01), (256, 5, 2, 512, 768, 0.01),
                (256, 5, 1, 512, 768, 0.0), (256, 5, 1, 512, 768, 1.0), (256, 5, 1, 512, 768, float("nan")), (258, 5, 1, 512, 768, 0.01),
                (256, 5, 1, 514, 768, 0.01), (256, 5, 1, 512, 770, 0.01), (256, 5, 1, 256, 768, 0.01), (256, 5, 1, 512, 256, 0.01), (256, 5, 1, 512, 512, 0.01)):
        assert L.sixdgs_opacity_reset(*bad, None) == -1, bad


def test_raw_wrappers_refuse_before_anything_is_launched(syn):
    ops = importlib.import_module("6dgs_amd.ops")
    d = syn.make_scene(10, 0)
    params = {"xyz": d["xyz"], "f_dc": d["f_dc"], "f_rest": d["f_rest"], "opacity": d["opacity"], "scale": d["log_scale"], "rot": d["rot"]}
    params = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in params.items()}
    state = ops.gaussian_adam_state(params)
    n_coef = 1 + params["f_rest"].shape[1]
    assert state["m"].shape == (10 * (11 + 3 * n_coef),) and state["status"].dtype == torch.int32 and not bool(state["m"].any())
    sl = ops.gaussian_adam_slices(10, n_coef)
    assert [sl[k].start for k in ops.FIT_GROUPS] == [0, 30, 60, 30 * (n_coef + 1), 30 * (n_coef + 1) + 10, 30 * (n_coef + 2) + 10]
    grads = {k: torch.zeros_like(v) for k, v in params.items()}
    with pytest.raises(RuntimeError):                                     # no CPU fallback
        ops.gaussian_adam(params, grads, state, 0, R.LRS)
    with pytest.raises(RuntimeError):
        ops.opacity_reset(params["opacity"])
    for bad in (dict(step=-1), dict(step=0.5), dict(lrs=R.LRS[:5]), dict(lrs=(-1.0,) * 6), dict(beta1=1.0), dict(eps=-1.0), dict(max_instances=0),
                dict(grads={"colour": grads["xyz"]}), dict(grads={"xyz": grads["rot"]}), dict(grads={"xyz": grads["xyz"].double()}),
                dict(state={"m": state["m"], "v": state["v"][:5], "status": state["status"]}), dict(state={"m": state["m"], "v": state["v"]}),
                dict(instances=torch.zeros(1)), dict(params={k: v for k, v in params.items() if k != "rot"}), dict(params=dict(params, rot=params["rot"][:5]))):
        kw = dict(dict(params=params, grads=grads, state=state, step=0, lrs=R.LRS), **bad)
        p, g, s, step, lrs = (kw.pop(k) for k in ("params", "grads", "state", "step", "lrs"))
        with pytest.raises(ValueError):
            ops.gaussian_adam(p, g, s, step, lrs, **kw)
    for bad in (dict(ceiling=0.0), dict(ceiling=1.0), dict(m_opacity=torch.zeros(9)), dict(v_opacity=torch.zeros(10, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.opacity_reset(params["opacity"], **bad)
    cams, target = torch.zeros(3, 16), torch.zeros(3, 8, 8, 3)
    good = dict(views=[[0], [2]], lrs=[R.LRS, R.LRS], sh_degrees=[0, 1])
    with pytest.raises(RuntimeError):
        ops.fit_scene_raw(params, cams, 8, 8, target, **good)
    for bad in (dict(views=[[0], [3]]), dict(views=[0, 1]), dict(views=[[0.0], [1.0]]), dict(lrs=[R.LRS]), dict(lrs=[R.LRS, (-1.0,) * 6]), dict(sh_degrees=[0, 4]),
                dict(sh_degrees=[0]), dict(resets=[1]), dict(resets=[0, 1], opacity_is_logit=False), dict(groups=()), dict(groups=("xyz", "uv")),
                dict(lambda_dssim=2.0), dict(beta2=1.0), dict(eps=-1.0), dict(reset_ceiling=1.0), dict(scale_modifier=0.0), dict(background=(1.0,)),
                dict(max_instances=0)):
        with pytest.raises(ValueError):
            ops.fit_scene_raw(params, cams, 8, 8, target, **dict(good, **bad))
    for bad_target in (target[:1], target.double(), torch.zeros(3, 8, 8, 4, dtype=torch.uint8), torch.zeros(3, 8, 9, 3), torch.zeros(3, 8, 8, 4)[..., :3]):
        with pytest.raises(ValueError):
            ops.fit_scene_raw(params, cams, 8, 8, bad_target, **good)
    with pytest.raises(ValueError):
        ops.fit_scene_raw(params, torch.zeros(3, 12), 8, 8, target, **good)
