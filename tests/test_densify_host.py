"""Adaptive density control without a GPU: csrc/densify_rules.h -- the per-entry rules the kernels of densify.hip run -- through its
host instantiation (libsixdgs_hostcheck.so) against the numpy restatement (tests/densify_reference.py), bit for bit on classification,
candidate order and counts and under the restatement's own fp32 bound on children's positions; values exactly at each threshold;
denom == 0; what the three new entry points answer and refuse without a device; cameras_extent and the fit's schedule against the
reference's formula and a literal walk of its loop; densify=None builds today's arrays."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import densify_reference as D  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sixdgs_densify_stats", "sixdgs_densify_workspace_bytes", "sixdgs_densify", "sixdgs_fit_scene_steps_workspace_bytes",
         "sixdgs_fit_scene_steps")
F = np.float32


@pytest.fixture(scope="module")
def hc():
    return C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_thresholds(hc, opts, scale_is_log=True, opacity_is_logit=True):
    out = np.zeros(4, F)
    f = C.c_float
    hc.hc_dn_thresholds(f(opts["grad_threshold"]), f(opts["percent_dense"]), f(opts["extent"]), f(opts["min_opacity"]), int(scale_is_log),
                        int(opacity_is_logit), _ptr(out))
    return dict(zip(("grad", "dense", "world", "opacity"), out))


def host_round(hc, params, stats, noise, opts, prune_big, screen_size=0, scale_is_log=True, opacity_is_logit=True):
    """densify_rules.h over float32 arrays -> cls [n], avg [n], flags [4,n], child_xyz [n,2,3], child_scale [n,3]."""
    n = params["xyz"].shape[0]
    cls, avg, flags = np.zeros(n, np.int32), np.zeros(n, F), np.zeros((4, n), np.int32)
    cxyz, cscale = np.zeros((n, 2, 3), F), np.zeros((n, 3), F)
    f = C.c_float
    hc.hc_dn_round(C.c_longlong(n), _ptr(params["xyz"]), _ptr(params["opacity"]), _ptr(params["scale"]), _ptr(params["rot"]), int(scale_is_log),
                   int(opacity_is_logit), _ptr(stats["grad_accum"]), _ptr(stats["denom"]), _ptr(stats["max_radii"]), _ptr(noise),
                   f(opts["grad_threshold"]), f(opts["percent_dense"]), f(opts["extent"]), f(opts["min_opacity"]), int(prune_big), int(screen_size),
                   _ptr(cls), _ptr(avg), _ptr(flags), _ptr(cxyz), _ptr(cscale))
    return cls, avg, flags, cxyz, cscale


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("scale_is_log,opacity_is_logit", ((True, True), (False, False)))
def test_thresholds_are_converted_once_in_double(hc, scale_is_log, opacity_is_logit):
    ops = importlib.import_module("6dgs_amd.ops")
    for opts in (D.OPTS, dict(grad_threshold=1e-3, percent_dense=0.02, extent=7.3, min_opacity=0.0), dict(D.OPTS, extent=0.37, min_opacity=0.2)):
        want = D.thresholds(**opts, scale_is_log=scale_is_log, opacity_is_logit=opacity_is_logit)
        got = host_thresholds(hc, opts, scale_is_log, opacity_is_logit)
        mine = ops.densify_thresholds(**opts, scale_is_log=scale_is_log, opacity_is_logit=opacity_is_logit)
        for k in want:
            assert F(got[k]).tobytes() == F(want[k]).tobytes() == F(mine[k]).tobytes(), (k, opts)
    t = D.thresholds(**D.OPTS)
    assert t["dense"] == F(np.log(np.float64(F(0.01)) * 3.0)) and t["opacity"] == F(np.log(np.float64(F(0.005)) / (1 - np.float64(F(0.005)))))
    for bad in (dict(grad_threshold=0.0), dict(percent_dense=0.0), dict(extent=float("inf")), dict(extent=-1.0), dict(min_opacity=1.0), dict(min_opacity=-0.1)):
        with pytest.raises(ValueError):
            ops.densify_thresholds(**dict(D.OPTS, **bad))


@pytest.mark.parametrize("n,scale_is_log,prune_big,screen_size", ((1, True, False, 0), (257, True, True, 0), (2000, True, True, 20), (2000, False, True, 0),
                                                                  (300, False, False, 0)))
def test_host_rules_are_the_restatement(hc, n, scale_is_log, prune_big, screen_size):
    c = D.random_case(n, 4, 10 + n, scale_is_log, scale_is_log)
    t = D.thresholds(**D.OPTS, scale_is_log=scale_is_log, opacity_is_logit=scale_is_log)
    ref = D.round_np(c["params"], c["m"], c["v"], c["stats"], c["noise"], t, prune_big, screen_size, scale_is_log)
    cls, avg, flags, cxyz, cscale = host_round(hc, c["params"], c["stats"], c["noise"], D.OPTS, prune_big, screen_size, scale_is_log, scale_is_log)
    assert np.array_equal(cls, ref["cls"]) and np.array_equal(bits(avg), bits(ref["avg"]))
    if n >= 257:
        assert all((cls == k).sum() > n // 20 for k in (D.KEEP, D.CLONE, D.SPLIT)), "the case does not plant every class"
    # the candidate order: segment after segment, ascending source, the survivors
    seg, src = np.nonzero(flags.reshape(-1))[0] // n, np.nonzero(flags.reshape(-1))[0] % n
    assert np.array_equal(seg, ref["seg"]) and np.array_equal(src, ref["src"])
    assert ref["counts"] == (seg.size, int((cls == D.CLONE).sum()), int((cls == D.SPLIT).sum()), n + int((cls != D.KEEP).sum()) - seg.size)
    assert not flags[0][cls == D.SPLIT].any() and not flags[1][cls != D.CLONE].any() and not flags[2][cls != D.SPLIT].any()
    assert np.array_equal(flags[2], flags[3])
    # child scales bit for bit; child positions against fp64 under the fp32 restatement's own bound
    child = ref["seg"] >= 2
    assert np.array_equal(bits(cscale[ref["src"][child]]), bits(ref["scale"][child]))
    if child.any():
        got = cxyz[ref["src"][child], ref["seg"][child] - 2]
        scale, y, limit = D.xyz_bound(ref["xyz"][child], ref["child_xyz64"][child])
        err = float(np.abs(got.astype(np.float64) - ref["child_xyz64"][child]).max())
        print(f"n {n} log {scale_is_log}: child xyz max |host - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e})")
        assert err <= limit


def test_values_exactly_at_each_threshold_and_denom_zero(hc):
    t = D.thresholds(**D.OPTS)
    up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    # rows: (avg, max scale, opacity, radius) -> what the documented side is
    small, fine = down(t["dense"]), F(2.0)
    rows = [(t["grad"], small, fine, 0),            # avg == grad_threshold: selected (>=) -> clone
            (down(t["grad"]), small, fine, 0),      # just below: kept
            (t["grad"], t["dense"], fine, 0),       # max scale == t_dense: not big (>) -> clone
            (t["grad"], up(t["dense"]), fine, 0),   # just above: split
            (F(0), small, t["opacity"], 0),         # opacity == t_opacity: not pruned (<)
            (F(0), small, down(t["opacity"]), 0),   # just below: pruned
            (F(0), t["world"], fine, 0),            # max scale == t_world: not pruned (>)
            (F(0), up(t["world"]), fine, 0),        # just above: pruned (with prune_big)
            (F(0), small, fine, 20),                # radius == screen_size: not pruned (>)
            (F(0), small, fine, 21)]                # above: pruned (with prune_big and screen_size > 0)
    n = len(rows)
    params = {"xyz": np.zeros((n, 3), F), "rot": np.tile(F([1, 0, 0, 0]), (n, 1)), "opacity": F([r[2] for r in rows]).reshape(n, 1),
              "scale": np.stack([F([r[1], r[1] - 1, r[1] - 2]) for r in rows]), "f_dc": np.zeros((n, 1, 3), F), "f_rest": np.zeros((n, 0, 3), F)}
    stats = {"grad_accum": F([r[0] for r in rows]), "denom": np.ones(n, np.int32), "max_radii": np.int32([r[3] for r in rows])}
    noise = np.zeros((n, 2, 3), F)
    cls, avg, flags, _, _ = host_round(hc, params, stats, noise, D.OPTS, True, 20)
    assert cls.tolist() == [D.CLONE, D.KEEP, D.CLONE, D.SPLIT, D.KEEP, D.KEEP, D.KEEP, D.KEEP, D.KEEP, D.KEEP]
    assert flags[0].tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1, 0] and flags[1].tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert flags[2].tolist() == flags[3].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    ref = D.round_np(params, np.zeros(n * 14, F), np.zeros(n * 14, F), stats, noise, t, True, 20)
    assert np.array_equal(ref["cls"], cls) and ref["counts"][0] == int(flags.sum())
    # prune_big off: neither the world size nor the radius prunes; screen_size 0: the radius does not
    _, _, off, _, _ = host_round(hc, params, stats, noise, D.OPTS, False, 20)
    assert off[0].tolist() == [1, 1, 1, 0, 1, 0, 1, 1, 1, 1]
    _, _, no_screen, _, _ = host_round(hc, params, stats, noise, D.OPTS, True, 0)
    assert no_screen[0].tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1, 1]
    # denom == 0: avg = 0 whatever was accumulated
    stats0 = {"grad_accum": F([1.0, np.inf, np.nan, 0.0] + [0.0] * (n - 4)), "denom": np.zeros(n, np.int32), "max_radii": np.zeros(n, np.int32)}
    cls0, avg0, _, _, _ = host_round(hc, params, stats0, noise, D.OPTS, False, 0)
    assert not avg0.any() and not cls0.any()
    assert not D.classify(stats0["grad_accum"], stats0["denom"], params["scale"], t)[0].any()


def _stats_call(L, **kw):
    a = dict(n=10, views=2, width=16, height=16, cap=100, fwd=256, fwd_bytes=None, bwd=512, bwd_bytes=None, radii=256, acc=256, denom=256, rad=256,
             grad2d=None, status=None)
    a.update(kw)
    fb = L.sixdgs_raster_views_workspace_bytes(10, 2, 16, 16, 100) if a["fwd_bytes"] is None else a["fwd_bytes"]
    bb = L.sixdgs_raster_views_backward_workspace_bytes(10, 2, 16, 16, 100) if a["bwd_bytes"] is None else a["bwd_bytes"]
    return L.sixdgs_densify_stats(a["n"], a["views"], a["width"], a["height"], a["cap"], a["fwd"], fb, a["bwd"], bb, a["radii"], a["acc"], a["denom"],
                                  a["rad"], a["grad2d"], a["status"], None)


def _densify_call(L, **kw):
    a = dict(n=10, n_coef=4, p=256, f_rest=256, log=1, logit=1, m=1024, v=2048, acc=256, denom=256, rad=256, noise=256, grad=2e-4, dense=0.01,
             extent=3.0, opacity=0.005, big=1, screen=0, n_cap=20, out=4096, f_rest_out=4096, m_out=8192, v_out=16384, counts=256, status=256, ws=None,
             ws_bytes=0)
    a.update(kw)
    p, o = a["p"], a["out"]
    return L.sixdgs_densify(a["n"], a["n_coef"], p, p, a["f_rest"], p, p, p, a["log"], a["logit"], a["m"], a["v"], a["acc"], a["denom"], a["rad"],
                            a["noise"], a["grad"], a["dense"], a["extent"], a["opacity"], a["big"], a["screen"], a["n_cap"], o, o, a["f_rest_out"], o, o, o,
                            a["m_out"], a["v_out"], a["counts"], a["status"], a["ws"], a["ws_bytes"], None)


def _steps_call(L, **kw):
    a = dict(scene=256, n=10, views=3, steps=2, batch=1, view=[0, 2], degree=[0, 1], reset=[0, 1], update=[1, 0], stats=[1, 1], first=0, mask=63, m=1024,
             v=2048, out=256, needed=256, acc=256, denom=256, rad=256, ws=None, ws_bytes=0)
    a.update(kw)
    s = a["scene"]
    arr = lambda x, dt: None if x is None else np.asarray(x, dt)  # noqa: E731
    view, degree, reset, update, stats = arr(a["view"], np.int32), arr(a["degree"], np.int32), arr(a["reset"], np.uint8), arr(a["update"], np.uint8), \
        arr(a["stats"], np.uint8)
    lr = np.full((a["steps"] if a["steps"] > 0 else 1, 6), 1e-3, F)
    return L.sixdgs_fit_scene_steps(s, s, 1, s, s, 1, s, s, 4, a["n"], 256, a["views"], 8, 8, 1.0, 256, 256, 0, 3, 0.2, a["steps"], a["batch"], _ptr(view),
                                    _ptr(lr), _ptr(degree), _ptr(reset), _ptr(update), _ptr(stats), a["first"], a["mask"], 0.9, 0.999, 1e-15, 0.01, 100,
                                    a["m"], a["v"], a["out"], a["out"], a["needed"], a["acc"], a["denom"], a["rad"], a["ws"], a["ws_bytes"], None)


def test_entry_points_in_header_binding_and_library():
    lib = importlib.import_module("6dgs_amd._lib")
    build = importlib.import_module("6dgs_amd.build")
    ops = importlib.import_module("6dgs_amd.ops")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sixdgs.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "densify.hip" in build.SOURCES and "densify_rules.h" in build.HEADERS and lib.ABI_VERSION == 10
    assert [len(lib.SIGNATURES[n][1]) for n in NAMES] == [16, 1, 36, 6, 46]
    so = C.CDLL(lib.LIB_PATH)                                              # a missing build fails here, it does not pass
    for name in NAMES:
        assert hasattr(so, name), f"{name} is not exported by the library"
    assert all(hasattr(ops, n) for n in ("densify_stats", "densify_stats_state", "densify", "densify_raw", "densify_buffers", "densify_thresholds",
                                         "fit_scene_steps_raw"))
    L = lib.load()
    # sixdgs_densify_stats: refused, or nothing to do, without a launch
    for bad in (dict(n=-1), dict(n=1 << 31), dict(views=-1), dict(views=65536), dict(width=0), dict(height=16385), dict(cap=0), dict(cap=1 << 31),
                dict(fwd=None), dict(bwd=None), dict(radii=None), dict(acc=None), dict(denom=None), dict(rad=None), dict(radii=258), dict(acc=257),
                dict(denom=258), dict(rad=259), dict(grad2d=258), dict(status=258), dict(fwd=128), dict(bwd=384)):
        assert _stats_call(L, **bad) == -1, bad
    assert _stats_call(L, fwd_bytes=L.sixdgs_raster_views_workspace_bytes(10, 2, 16, 16, 100) - 1) == -2
    assert _stats_call(L, bwd_bytes=L.sixdgs_raster_views_backward_workspace_bytes(10, 2, 16, 16, 100) - 1) == -2
    assert _stats_call(L, views=0, fwd=None) == 0 and _stats_call(L, n=0, bwd=None, acc=None) == 0
    # sixdgs_densify_workspace_bytes: two uint32 arrays of 4 n + 1 and the scan's storage, without a GPU
    ws = L.sixdgs_densify_workspace_bytes
    assert ws(-1) == 0 and ws(1 << 31) == 0 and ws(0) > 0 and ws(0) % 256 == 0
    assert ws(1000) >= 2 * 4 * 4001 + (1 << 20) and ws(70001) > ws(1000) and ops.densify_workspace_bytes(1000) == ws(1000)
    # sixdgs_densify
    for bad in (dict(n=-1), dict(n=1 << 31), dict(n_coef=0), dict(n_coef=17), dict(log=2), dict(logit=-1), dict(grad=0.0), dict(grad=float("nan")),
                dict(grad=float("inf")), dict(dense=0.0), dict(extent=0.0), dict(extent=float("inf")), dict(opacity=-0.1), dict(opacity=1.0),
                dict(opacity=float("nan")), dict(screen=-1), dict(n_cap=-1), dict(n_cap=1 << 31), dict(counts=None), dict(status=None), dict(counts=260),
                dict(status=258), dict(p=None), dict(f_rest=None), dict(out=None), dict(f_rest_out=None), dict(out=256), dict(m=None), dict(v=None),
                dict(acc=None), dict(denom=None), dict(rad=None), dict(noise=None), dict(m_out=None), dict(v_out=None), dict(v_out=8192), dict(m_out=1024),
                dict(v_out=2048), dict(p=258), dict(out=4098), dict(m=1026), dict(noise=257), dict(m_out=8194)):
        assert _densify_call(L, **bad) == -1, bad
    assert _densify_call(L, ws=256, ws_bytes=ws(10) - 1) == -2 and _densify_call(L, ws_bytes=0) == -2
    assert _densify_call(L, ws_bytes=ws(10)) == -1 and _densify_call(L, ws=128, ws_bytes=ws(10)) == -1
    assert _densify_call(L, n_coef=1, f_rest=None, f_rest_out=None) == -2 and _densify_call(L, n_cap=0, out=None, f_rest_out=None, m_out=None, v_out=None) == -2
    # sixdgs_fit_scene_steps: sixdgs_fit_scene's refusals, and its own
    sw = L.sixdgs_fit_scene_steps_workspace_bytes
    base = L.sixdgs_fit_scene_workspace_bytes(2000, 16, 3, 64, 48, 5000)
    assert base + 3 * 2000 * 4 <= sw(2000, 16, 3, 64, 48, 5000) <= base + 3 * 2000 * 4 + 256 and sw(10, 0, 1, 8, 8, 10) == 0 and sw(10, 4, 0, 8, 8, 10) == 0
    assert ops.fit_scene_steps_workspace_bytes(2000, 16, 3, 64, 48, 5000) == sw(2000, 16, 3, 64, 48, 5000)
    for bad in (dict(n=-1), dict(views=0), dict(steps=0), dict(batch=0), dict(view=[0, 3]), dict(view=None), dict(degree=None), dict(reset=None),
                dict(mask=0), dict(first=-1), dict(first=(1 << 31) - 2), dict(scene=None), dict(m=None), dict(v=1024), dict(out=None), dict(needed=260),
                dict(acc=None), dict(denom=None), dict(rad=None), dict(acc=258), dict(denom=257), dict(rad=259)):
        assert _steps_call(L, **bad) == -1, bad
    need = sw(10, 4, 1, 8, 8, 100)
    assert _steps_call(L, ws=256, ws_bytes=need - 1) == -2 and _steps_call(L) == -2 and _steps_call(L, ws_bytes=need) == -1
    assert _steps_call(L, update=None, stats=None, acc=None, denom=None, rad=None) == -2                  # no statistics asked for: no arrays needed
    assert _steps_call(L, stats=[0, 0], acc=None) == -2


def test_raw_wrappers_refuse_before_anything_is_launched(syn):
    ops = importlib.import_module("6dgs_amd.ops")
    c = D.random_case(10, 4, 0)
    params = {k: torch.from_numpy(v) for k, v in c["params"].items()}
    state = {"m": torch.from_numpy(c["m"]), "v": torch.from_numpy(c["v"]), "status": torch.zeros(1, dtype=torch.int32)}
    stats = {k: torch.from_numpy(v) for k, v in c["stats"].items()}
    noise = torch.from_numpy(c["noise"])
    zero = ops.densify_stats_state(10, "cpu")
    assert [(k, v.dtype, tuple(v.shape)) for k, v in zero.items()] == [("grad_accum", torch.float32, (10,)), ("denom", torch.int32, (10,)),
                                                                      ("max_radii", torch.int32, (10,))] and not any(bool(v.any()) for v in zero.values())
    out = ops.densify_buffers(params, 20)
    assert out["f_rest"].shape == (20, 3, 3) and out["m"].shape == (20 * 23,)
    kw = dict(D.OPTS, prune_big=True)
    with pytest.raises(RuntimeError):                                     # no CPU fallback
        ops.densify(params, state, stats, noise, **kw)
    for bad in (dict(grad_threshold=0.0), dict(extent=-1.0), dict(min_opacity=1.0), dict(screen_size=-1), dict(screen_size=0.5), dict(noise=noise[:5]),
                dict(noise=noise.double()), dict(stats=dict(stats, denom=stats["denom"].float())), dict(stats=dict(stats, max_radii=stats["max_radii"][:5])),
                dict(state=dict(state, m=state["m"][:7])), dict(state={"m": state["m"], "v": state["v"]}), dict(out=dict(out, rot=out["rot"][:19])),
                dict(out={k: v for k, v in out.items() if k != "m"}), dict(out=dict(out, v=out["v"][:50])), dict(params=dict(params, rot=params["rot"][:5]))):
        a = dict(dict(params=params, state=state, stats=stats, noise=noise, out=out), **kw)
        a.update(bad)
        p, s, st, nz, o = (a.pop(k) for k in ("params", "state", "stats", "noise", "out"))
        with pytest.raises(ValueError):
            ops.densify_raw(p, s, st, nz, o, **a)
    radii, ws = torch.zeros(2, 10, dtype=torch.int32), torch.zeros(1024, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.densify_stats((ws, 100), ws, radii, stats, 16, 16)
    for bad in ((ws, ws, radii, stats, 16, 16), ((ws, 0), ws, radii, stats, 16, 16), ((ws, 100), None, radii, stats, 16, 16),
                ((ws, 100), ws, radii.long(), stats, 16, 16), ((ws, 100), ws, radii[0], stats, 16, 16), ((ws, 100), ws, radii[:, :5], stats, 16, 16),
                ((ws, 100), ws, radii, zero | {"denom": zero["denom"].long()}, 16, 16), ((ws, 100), ws, radii, stats, 0, 16)):
        with pytest.raises(ValueError):
            ops.densify_stats(*bad)
    with pytest.raises(ValueError):
        ops.densify_stats((ws, 100), ws, radii, stats, 16, 16, status=torch.zeros(1))
    cams, target = torch.zeros(3, 16), torch.zeros(3, 8, 8, 3)
    lrs = [(1e-3,) * 6] * 2
    fit_state = dict(state, instances_needed=torch.zeros(1, dtype=torch.int64))
    good = dict(views=[[0], [2]], lrs=lrs, sh_degrees=[0, 1], updates=[1, 0], stats_steps=[1, 1], stats=stats)
    with pytest.raises(RuntimeError):
        ops.fit_scene_steps_raw(params, cams, 8, 8, target, fit_state, **good)
    for bad in (dict(views=[[0], [3]]), dict(updates=[1]), dict(stats_steps=[1, 0, 1]), dict(stats=None), dict(stats=dict(stats, denom=stats["denom"][:3])),
                dict(first_adam_step=-1), dict(first_adam_step=0.5), dict(max_instances=0), dict(lrs=lrs[:1]), dict(groups=())):
        with pytest.raises(ValueError):
            ops.fit_scene_steps_raw(params, cams, 8, 8, target, fit_state, **dict(good, **bad))
    for bad_state in (state, dict(fit_state, m=state["m"][:5]), dict(fit_state, status=torch.zeros(1)), dict(fit_state, instances_needed=torch.zeros(1))):
        with pytest.raises(ValueError):
            ops.fit_scene_steps_raw(params, cams, 8, 8, target, bad_state, **good)


def test_cameras_extent_is_the_reference_formula():
    fit = importlib.import_module("6dgs_amd.fit")
    rng = np.random.default_rng(5)
    for views in (1, 2, 5, 40):
        c2w = np.tile(np.eye(4), (views, 1, 1))
        c2w[:, :3, 3] = rng.standard_normal((views, 3)) * 3 + 1
        # scene/datasets_utils.py:7-25 on the camera centres as 3 x 1 columns
        cam_centers = np.hstack([m[:3, 3:4] for m in c2w])
        center = np.mean(cam_centers, axis=1, keepdims=True)
        diagonal = np.max(np.linalg.norm(cam_centers - center, axis=0, keepdims=True))
        for arg in (c2w, torch.from_numpy(c2w).float()):
            assert fit.cameras_extent(arg) == pytest.approx(diagonal * 1.1, rel=1e-6, abs=1e-12)
    assert fit.cameras_extent(np.tile(np.eye(4), (1, 1, 1))) == 0.0


@pytest.mark.parametrize("steps,from_iter,until_iter,interval,reset_every,white", ((40, 5, 31, 4, 12, False), (40, 5, 31, 4, 12, True), (30, 0, 100, 7, 10, False),
                                                                                   (25, 8, 9, 3, 5, True), (20, 3, 20, 1, 6, False), (12, 50, 100, 5, 4, False)))
def test_schedule_is_a_literal_walk_of_the_reference_loop(steps, from_iter, until_iter, interval, reset_every, white):
    """The fit is the first `steps` iterations of a longer training (the reference makes no update on its very last iteration)."""
    fit = importlib.import_module("6dgs_amd.fit")
    opts = dict(from_iter=from_iter, until_iter=until_iter, interval=interval, prune_big_after=reset_every, reset_at_from_iter=white)
    plan = fit.densify_plan(steps, opts, reset_every, True)
    walk = D.train_walk(steps + 1, from_iter, until_iter, interval, reset_every, white)
    its = lambda flags: (np.nonzero(flags)[0] + 1).tolist()  # noqa: E731
    upto = lambda xs: [x for x in xs if x <= steps]  # noqa: E731
    assert its(plan["stats"]) == upto(walk["stats"]) and its(plan["round"]) == upto(walk["round"]) and its(plan["reset"]) == upto(walk["reset"])
    assert its(plan["update"]) == upto(walk["update"])
    assert [bool(plan["prune_big"][it - 1]) for it in its(plan["round"])] == walk["prune_big"][:len(its(plan["round"]))]
    assert all(v.dtype == bool and v.shape == (steps,) for v in plan.values())
    assert not fit.densify_plan(steps, opts, reset_every, False)["reset"].any()           # the opacity does not move: no reset


def test_densify_none_builds_todays_arrays():
    fit = importlib.import_module("6dgs_amd.fit")
    for steps, every in ((1, 0), (10, 0), (10, 3), (7, 7)):
        plan = fit.densify_plan(steps, None, every, True)
        assert plan["update"].all() and not plan["stats"].any() and not plan["round"].any() and not plan["prune_big"].any()
        today = (np.arange(steps) + 1) % every == 0 if every > 0 else np.zeros(steps, bool)           # fit_scene's resets before this option
        assert np.array_equal(plan["reset"], today) and plan["reset"].dtype == bool
        assert not fit.densify_plan(steps, None, every, False)["reset"].any()
    assert fit.densify_options({}) == fit.DENSIFY_DEFAULTS and fit.DENSIFY_DEFAULTS["grad_threshold"] == 2e-4 and fit.DENSIFY_DEFAULTS["interval"] == 100
    assert (fit.DENSIFY_DEFAULTS["from_iter"], fit.DENSIFY_DEFAULTS["until_iter"], fit.DENSIFY_DEFAULTS["prune_big_after"]) == (500, 15000, 3000)

    class Options:
        interval, seed = 7, 3
    assert fit.densify_options(Options())["interval"] == 7 and fit.densify_options(Options())["seed"] == 3
    for bad in (dict(interval=0), dict(from_iter=-1), dict(grad_threshold=0.0), dict(percent_dense=float("inf")), dict(extent=0.0), dict(min_opacity=1.0),
                dict(screen_size=-1), dict(seed=1.5), dict(every=3)):
        with pytest.raises(ValueError):
            fit.densify_options(bad)
    # fit_scene refuses bad options before it looks at the scene's device
    pkg = importlib.import_module("6dgs_amd")
    syn = importlib.import_module("6dgs_amd.synthetic")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(10, 0), device="cpu")
    images, c2w, K = [np.zeros((8, 8, 3), np.uint8)] * 2, torch.eye(4)[None].repeat(2, 1, 1), torch.tensor([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    for bad in (dict(interval=0), dict(every=3), dict(min_opacity=-1.0)):
        with pytest.raises(ValueError):
            fit.fit_scene(scene, images, c2w, K, steps=3, densify=bad)
    for backend in ("torch", "fused"):                                  # good options get as far as the scene's device
        with pytest.raises(RuntimeError):
            fit.fit_scene(scene, images, c2w, K, steps=3, backend=backend, densify={})
    noise = fit.round_noise(5, 3, 1, "cpu")
    assert noise.shape == (5, 2, 3) and torch.equal(noise, fit.round_noise(5, 3, 1, "cpu")) and not torch.equal(noise, fit.round_noise(5, 3, 2, "cpu"))


def test_densify_torch_is_the_restatement_on_the_host():
    """fit.densify_torch runs on any device: on the CPU it is the numpy restatement bit for bit, children's positions aside."""
    fit = importlib.import_module("6dgs_amd.fit")
    ops = importlib.import_module("6dgs_amd.ops")
    for n, log, big, screen in ((300, True, True, 20), (300, False, True, 0), (1, True, False, 0)):
        c = D.random_case(n, 4, 40 + n, log, log)
        t = D.thresholds(**D.OPTS, scale_is_log=log, opacity_is_logit=log)
        ref = D.round_np(c["params"], c["m"], c["v"], c["stats"], c["noise"], t, big, screen, log)
        sl = ops.gaussian_adam_slices(n, 4)
        params = {k: torch.from_numpy(v) for k, v in c["params"].items()}
        state = {k: (torch.from_numpy(c["m"][sl[k]]).reshape(params[k].shape), torch.from_numpy(c["v"][sl[k]]).reshape(params[k].shape)) for k in D.GROUPS}
        new, new_state, counts = fit.densify_torch(params, state, {k: torch.from_numpy(v) for k, v in c["stats"].items()}, torch.from_numpy(c["noise"]),
                                                   **D.OPTS, prune_big=big, screen_size=screen, scale_is_log=log, opacity_is_logit=log)
        assert counts == ref["counts"]
        so = ops.gaussian_adam_slices(counts[0], 4)
        for k in D.GROUPS:
            if k != "xyz":
                assert np.array_equal(bits(new[k].numpy()), bits(ref[k])), k
            assert np.array_equal(bits(new_state[k][0].numpy().reshape(-1)), bits(ref["m"][so[k]])), k
            assert np.array_equal(bits(new_state[k][1].numpy().reshape(-1)), bits(ref["v"][so[k]])), k
        child = ref["seg"] >= 2
        assert np.array_equal(bits(new["xyz"].numpy()[~child]), bits(ref["xyz"][~child]))
        if child.any():
            _, _, limit = D.xyz_bound(ref["xyz"][child], ref["child_xyz64"][child])
            assert np.abs(new["xyz"].numpy()[child].astype(np.float64) - ref["child_xyz64"][child]).max() <= limit
