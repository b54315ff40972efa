"""sixdgs_densify on the GPU against the numpy restatement (tests/densify_reference.py) and against fit.densify_torch: bit for bit
on everything except children's positions -- order, copies, child scales, m / v, counts --, children's positions against fp64 under the
restatement's own fp32 bound (expf is the one function not restatable to the bit); sizes around a workgroup and across several scan
blocks; planted classes; the capacity protocol; guard rows behind n_out in all eight outputs; the same bytes twice.  Everything runs
inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import densify_reference as D  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = 12345.5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    importlib.import_module("6dgs_amd")
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def fit(ops):
    return importlib.import_module("6dgs_amd.fit")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def to_gpu(c):
    params = {k: torch.from_numpy(v).cuda() for k, v in c["params"].items()}
    state = {"m": torch.from_numpy(c["m"]).cuda(), "v": torch.from_numpy(c["v"]).cuda(), "status": torch.zeros(1, dtype=torch.int32, device="cuda")}
    stats = {k: torch.from_numpy(v).cuda() for k, v in c["stats"].items()}
    return params, state, stats, torch.from_numpy(c["noise"]).cuda()


def run_raw(ops, c, n_cap, **kw):
    """densify_raw into sentinel-filled buffers of n_cap rows -> (buffers as numpy, counts as a tuple, status)."""
    params, state, stats, noise = to_gpu(c)
    out = ops.densify_buffers(params, n_cap)
    for t in out.values():
        t.fill_(SENTINEL)
    counts = ops.densify_raw(params, state, stats, noise, out, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}, tuple(int(x) for x in counts.cpu()), int(state["status"])


def check_against(out, ref, n_coef, what):
    """The first n_out rows are the restatement's, the rest is untouched."""
    n_out = ref["counts"][0]
    child = ref["seg"] >= 2
    for k in D.GROUPS:
        got = out[k][:n_out]
        assert bits(out[k][n_out:]).size == 0 or (out[k][n_out:] == F(SENTINEL)).all(), f"{what}: rows of {k} behind n_out were written"
        if k == "xyz":
            assert np.array_equal(bits(got[~child]), bits(ref[k][~child])), f"{what}: xyz of originals and clones"
        else:
            assert np.array_equal(bits(got), bits(ref[k])), f"{what}: {k}"
    size = n_out * (11 + 3 * n_coef)
    for k in ("m", "v"):
        assert np.array_equal(bits(out[k][:size]), bits(ref[k])), f"{what}: {k}"
        assert (out[k][size:] == F(SENTINEL)).all(), f"{what}: {k} behind n_out was written"
    if child.any():
        scale, y, limit = D.xyz_bound(ref["xyz"][child], ref["child_xyz64"][child])
        err = float(np.abs(out["xyz"][:n_out][child].astype(np.float64) - ref["child_xyz64"][child]).max())
        print(f"{what}: children's xyz max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
        assert err <= limit, what


@pytest.mark.parametrize("n,n_coef,stored", ((1, 4, True), (255, 1, True), (256, 16, True), (257, 4, False), (2000, 16, False), (2000, 1, True),
                                             (70001, 4, True)))
def test_round_is_the_restatement_and_the_torch_round(ops, fit, n, n_coef, stored):
    """stored: log scales and logit opacities (True) or plain values (False).  A mix of classes with prunable children, prune_big on
    (with screen_size > 0) and off."""
    c = D.random_case(n, n_coef, 100 + n + n_coef, stored, stored)
    t = D.thresholds(**D.OPTS, scale_is_log=stored, opacity_is_logit=stored)
    for prune_big, screen in ((True, 20), (False, 0)):
        what = f"n {n} n_coef {n_coef} stored {stored} prune_big {prune_big}"
        kw = dict(D.OPTS, prune_big=prune_big, screen_size=screen, scale_is_log=stored, opacity_is_logit=stored)
        ref = D.round_np(c["params"], c["m"], c["v"], c["stats"], c["noise"], t, prune_big, screen, stored)
        out, counts, status = run_raw(ops, c, 2 * n + 3, **kw)
        assert counts == ref["counts"] and status == 0, what
        check_against(out, ref, n_coef, what)
        if n >= 255:
            assert all((ref["cls"] == k).any() for k in (D.KEEP, D.CLONE, D.SPLIT)) and ref["counts"][3] > 0 and (ref["seg"] == 3).any()
            if prune_big:       # children of the largest sources are pruned on their own scale; originals by their radius
                pruned_children = 2 * ref["counts"][2] - int((ref["seg"] >= 2).sum())
                assert pruned_children > 0
        # the same bytes twice
        again, counts2, _ = run_raw(ops, c, 2 * n + 3, **kw)
        assert counts2 == counts and all(np.array_equal(bits(out[k]), bits(again[k])) for k in out), what
        # ops.densify (buffers of 2 n rows, one read of n_out) and fit.densify_torch on the GPU
        params, state, stats, noise = to_gpu(c)
        new, new_state, cnt = ops.densify(params, state, stats, noise, **kw)
        assert tuple(int(x) for x in cnt.cpu()) == counts and new["xyz"].shape[0] == counts[0] and new_state["status"] is state["status"]
        assert all(np.array_equal(bits(new[k].cpu().numpy()), bits(out[k][:counts[0]])) for k in D.GROUPS)
        sl, so = ops.gaussian_adam_slices(n, n_coef), ops.gaussian_adam_slices(counts[0], n_coef)
        tstate = {k: (state["m"][sl[k]].reshape(params[k].shape), state["v"][sl[k]].reshape(params[k].shape)) for k in D.GROUPS}
        tnew, tnew_state, tcounts = fit.densify_torch(params, tstate, stats, noise, **kw)
        assert tcounts == counts, what
        child = ref["seg"] >= 2
        for k in D.GROUPS:
            a, b = tnew[k].cpu().numpy(), new[k].cpu().numpy()
            if k == "xyz":
                assert np.array_equal(bits(a[~child]), bits(b[~child])), what
                if child.any():
                    _, _, limit = D.xyz_bound(ref["xyz"][child], ref["child_xyz64"][child])
                    assert np.abs(a[child].astype(np.float64) - ref["child_xyz64"][child]).max() <= limit, what
            else:
                assert np.array_equal(bits(a), bits(b)), (what, k)
            assert torch.equal(tnew_state[k][0].reshape(-1), new_state["m"][so[k]]) and torch.equal(tnew_state[k][1].reshape(-1), new_state["v"][so[k]]), k


def planted(n, n_coef, kind):
    """All keep, all pruned, all clone or all split: every Gaussian of random_case moved to one side of every threshold."""
    c = D.random_case(n, n_coef, 7)
    p, s = c["params"], c["stats"]
    s["denom"][:] = 2
    s["grad_accum"][:] = F(2 * 1e-3) if kind in ("clone", "split") else F(0)
    p["scale"][:] = F(np.log(0.1)) if kind == "split" else F(np.log(0.01))
    p["opacity"][:] = F(-9.0) if kind == "pruned" else F(1.0)
    return c


@pytest.mark.parametrize("n", (1, 257, 2000))
def test_planted_classes_and_the_capacity(ops, n):
    n_coef = 4
    t = D.thresholds(**D.OPTS)
    kw = dict(D.OPTS, prune_big=True, screen_size=0)
    for kind, want in (("keep", (n, 0, 0, 0)), ("pruned", (0, 0, 0, n)), ("clone", (2 * n, n, 0, 0)), ("split", (2 * n, 0, n, 0))):
        c = planted(n, n_coef, kind)
        ref = D.round_np(c["params"], c["m"], c["v"], c["stats"], c["noise"], t, True, 0)
        out, counts, status = run_raw(ops, c, 2 * n, **kw)           # all clone and all split fill n_cap = 2 n exactly
        assert counts == want == ref["counts"] and status == 0, kind
        check_against(out, ref, n_coef, f"n {n} all {kind}")
        if kind == "keep":
            assert all(np.array_equal(bits(out[k][:n]), bits(c["params"][k])) for k in D.GROUPS) and np.array_equal(bits(out["m"][:c["m"].size]), bits(c["m"]))
        if kind == "clone":
            assert all(np.array_equal(bits(out[k][n:]), bits(c["params"][k])) for k in D.GROUPS)
        if kind == "split":
            assert not out["m"].any() and not out["v"].any() and np.array_equal(bits(out["opacity"][:n]), bits(out["opacity"][n:]))
            assert np.array_equal(bits(out["scale"][:n]), bits(c["params"]["scale"] - D.LOG_SPLIT))
        if kind in ("clone", "split"):      # one row short: only counts and bit 1 of the status are written
            short, counts_s, status_s = run_raw(ops, c, 2 * n - 1, **kw)
            assert counts_s == want and status_s == ops.FIT_STATUS_CAPACITY
            assert all((a == F(SENTINEL)).all() for a in short.values()), f"all {kind}: an output was written although n_out > n_cap"
    # n == 0 writes counts = 0
    c = D.random_case(0, n_coef, 1)
    _, counts, status = run_raw(ops, c, 0, **kw)
    assert counts == (0, 0, 0, 0) and status == 0
