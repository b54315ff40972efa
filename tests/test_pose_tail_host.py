"""The least-squares pose tail without a GPU: the fp64 restatement (tests/pose_tail_reference.py) against the g6_pose goldens and against
the CPU oracle over the case generator that tests/test_gpu_pose_tail.py runs on the GPU; what the generator covers.

Measured here (printed by the tests; 16 k x 30 cases = 480 lists):
  oracle centre against the restatement, worst |c - c_64|_inf / (cond(A) max(1, |c_64|_inf)) = 9.41e-07  ->  CENTRE_C = 4 x that = 3.8e-06;
  share of cases with a decision inside rounding = 3 of 480 = 0.62 % (limit 1 %): three k = 1 lists whose fp64 determinant 1 - |d|^2 lies in [0.5e-7, 2e-7]."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_tail_reference as PT  # noqa: E402


def test_reference_against_the_goldens(golden):
    """Keep mask, flags, centre and c2w of every g6_pose case, at the tolerances of test_a17_to_a21_solve_pose."""
    g = golden("g6_pose")
    for name in (str(c) for c in g["cases"]):
        r = PT.pose_tail(g[f"{name}_ori"], g[f"{name}_dir"], g[f"{name}_idx"], g[f"{name}_w"], g[f"{name}_up"], g[f"{name}_gt"])
        assert (r["keep"] == g[f"{name}_keep_mask"]).all() and r["n_kept"] == int(g[f"{name}_keep_mask"].sum()), name
        assert r["singular_rotation"] == bool(g[f"{name}_flags"][0]) and r["nan_pose"] == bool(g[f"{name}_flags"][1]), name
        assert np.abs(r["c2w"] - g[f"{name}_c2w"]).max() < 1e-5, name
        if np.isnan(g[f"{name}_centre"]).any():
            assert r["nan_centre"] and r["status"] & 4 and np.isnan(r["centre"]).all(), name
        else:
            assert np.abs(r["centre"] - g[f"{name}_centre"]).max() < 1e-5, name
            assert np.abs(r["w_final"][r["keep"]] - g[f"{name}_w_final"]).max() < 1e-7, name
        assert abs(r["errors"][0] - float(g[f"{name}_terr"])) < 1e-5 and abs(r["errors"][1] - float(g[f"{name}_aerr"])) < 1e-3, name
        assert PT.status_is_decided(r) and PT.weights_are_decided(r), name


def test_reference_strips_padding_at_any_position():
    c = PT.cases(100)[8]                                                 # a fewdup list
    base = PT.pose_tail(c["ori"], c["dir"], c["idx"], c["val"], c["up"])
    pad = np.array([-1, PT.R, -7, PT.R + 12345, 1 << 40])
    where = np.sort(np.random.default_rng(0).choice(150, size=50, replace=False))
    idx, val = np.empty(150, np.int64), np.full(150, np.nan, np.float32)
    valid = np.ones(150, bool)
    valid[where] = False
    idx[where], idx[valid], val[valid] = pad[np.arange(50) % 5], c["idx"], c["val"]
    r = PT.pose_tail(c["ori"], c["dir"], idx, val, c["up"])
    assert (r["valid"] == valid).all() and r["n_kept"] == base["n_kept"] and r["status"] == base["status"]
    assert np.array_equal(r["centre"], base["centre"]) and np.array_equal(r["c2w"], base["c2w"])
    assert np.array_equal(r["w_final"][valid], base["w_final"]) and (r["w_final"][where] == 0).all() and not r["keep"][where].any()
    empty = PT.pose_tail(c["ori"], c["dir"], pad, np.zeros(5), c["up"])
    assert empty["status"] == 6 and empty["n_kept"] == 0 and np.array_equal(empty["c2w"], np.eye(4)) and (empty["w_final"] == 0).all()


def test_reference_against_the_oracle_over_the_generator(oracle):
    """Two independent statements of the tail (the C oracle in fp32 with its own re-derivation of the isin rule; PyTorch's ops + fp64) on
    every generated list: identical keep masks and kept counts, w_final within 1e-6, the flags, and the oracle's centre error in units
    of cond(A) max(1, |c|) -- the measurement CENTRE_C is made from."""
    worst, worst_at, n, skipped, never = 0.0, None, 0, [], []
    for k in PT.KS:
        cs, refs = PT.reference_cases(k)
        for c, r in zip(cs, refs):
            tag = (c["kind"], k, c["j"], c["note"])
            o = oracle.pose_from_topk(c["ori"], c["dir"], c["idx"], c["val"], c["up"])
            n += 1
            assert (o["keep"] == r["keep"]).all(), tag
            assert o["n_kept"] == r["n_kept"], tag
            if PT.undecided(r):
                skipped.append(tag)
                if c["kind"] in ("allbehind", "parallel", "upsing"):
                    never.append(tag)
            if PT.status_is_decided(r):
                assert bool(o["flags"][0]) == r["singular_rotation"] and bool(o["flags"][1]) == r["nan_pose"], tag
            if PT.centre_is_decided(r):
                assert np.isnan(o["centre"]).any() == r["nan_centre"], tag
            if PT.centre_is_decided(r) and PT.weights_are_decided(r):
                assert np.allclose(o["w_final"], r["w_final"], rtol=0, atol=1e-6, equal_nan=True), tag
            if not PT.undecided(r):
                assert np.abs(o["c2w"][:3, :3] - r["c2w"][:3, :3]).max() <= 2e-4, tag
            if PT.centre_is_decided(r) and not r["nan_centre"]:
                e = float(np.abs(o["centre"] - r["centre"]).max() / (r["cond"] * max(1.0, np.abs(r["centre"]).max())))
                if e > worst:
                    worst, worst_at = e, tag
                assert e <= PT.CENTRE_C, (tag, e)
    print(f"[pose tail] oracle centre against fp64 over {n} lists: worst {worst:.3g} of cond(A) max(1, |c|) at {worst_at}; "
          f"CENTRE_C = {PT.CENTRE_C:.3g} = {PT.CENTRE_C / worst:.2f} x that")
    print(f"[pose tail] decisions inside rounding: {len(skipped)} of {n} = {len(skipped) / n:.2%} {skipped}")
    assert PT.CENTRE_C / 8 <= worst <= PT.CENTRE_C / 2, "CENTRE_C is no longer 4 x the oracle's worst centre error (within a factor of 2): re-measure"
    assert len(skipped) <= PT.SKIP_SHARE * n and not never


def test_generator_reaches_what_it_is_for():
    """Every kind at every k; for every k >= 64 lists on both sides of torch.isin's algorithm switch, and straddle pairs ONE origin apart
    on different sides of it; coordinate coincidences that keep a ray no whole-origin match would; each status bit where it is expected."""
    pairs_across = 0
    for k in PT.KS:
        cs, refs = PT.reference_cases(k)
        assert len(cs) == 30 and {c["kind"] for c in cs} == set(PT.KINDS)
        assert all(c["idx"].shape == (k,) and c["ori"].shape == (PT.R, 3) and len(set(c["idx"].tolist())) == k for c in cs)
        sides = {r["sorting"] for r in refs}
        if k >= 64:
            assert sides == {False, True}, k
            u_lo, u_hi = PT.straddle_counts(k)
            assert u_hi == u_lo + 1 and 3 * u_lo < PT.small_set_threshold(k) <= 3 * u_hi
        st = [(c, r) for c, r in zip(cs, refs) if c["kind"] == "straddle"]
        for (ca, ra), (cb, rb) in zip(st[0::2], st[1::2]):
            u_lo, u_hi = PT.straddle_counts(k)
            assert (ra["n_once"], rb["n_once"]) == (u_lo, u_hi), k
            if u_hi == u_lo + 1:
                differ = (ca["ori"][ca["idx"]] != cb["ori"][cb["idx"]]).any(1)
                assert differ.sum() == 1 and np.array_equal(ca["idx"], cb["idx"]) and np.array_equal(ca["val"], cb["val"])
                pairs_across += int(ra["sorting"] != rb["sorting"])
                if ra["sorting"] != rb["sorting"] and k - u_hi >= 2:
                    assert ra["n_kept"] != rb["n_kept"], k            # the sort-based side keeps copies the small-set side drops
        for c, r in zip(cs, refs):
            if c["kind"] == "alphabet" and not r["sorting"] and r["n_once"]:
                # a ray whose whole origin occurs more than once is kept through a single coordinate
                rows = c["ori"][c["idx"]]
                copies = (rows[:, None, :] == rows[None, :, :]).all(2).sum(1)
                assert (r["keep"] & (copies > 1)).any() or not (copies > 1).any(), (k, c["j"])
            if c["kind"] == "allbehind":
                assert r["status"] == (2 if k > 1 else 6) and not (r["front"][r["keep"]] > 0).any()
            if c["kind"] == "parallel":
                assert r["status"] == 6 and r["det_centre"] == 0.0 and r["n_kept"] == k
            if c["kind"] == "upsing" and k > 1:
                # up exactly along the watch direction: up x watch is exactly 0, the x axis 0 / 0.  A NaN determinant is not < 1e-7, so
                # the singular-rotation bit stays clear and the NaN fall-back answers (in PyTorch, the oracle and the kernel alike);
                # a determinant that is finite and below 1e-7 only comes out of rounding noise, which no test can pin.
                assert r["cross_norm"] == 0.0 and r["status"] == 2 and not r["nan_centre"] and r["n_kept"] == k
                assert (r["front"] > 0.5).all() and np.array_equal(r["c2w"], np.eye(4))
    assert pairs_across >= len([k for k in PT.KS if k >= 64])
