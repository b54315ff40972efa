"""The one-pass image preparation (sixdgs_image_prep), without a GPU: tests/image_prep_reference.py against PyTorch's antialiased bicubic
on the CPU; csrc/image_prep_rules.h -- spans, weights and the launcher's plan -- through its host instantiation
(libsixdgs_hostcheck.so) against that restatement; the plan over every image height from 8 to 4096, where the assertion is that no
band's row window exceeds the rows the launcher reserves in LDS (the kernel clamps silently there); and the fitness of every case of
the GPU tests."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_reference as R  # noqa: E402

torch = pytest.importorskip("torch")

F = np.float32
LDS_BUDGET = 150 * 1024


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(importlib.import_module("6dgs_amd.build").build_hostcheck())
    lib.hc_ip_plan.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.hc_ip_spans.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    lib.hc_ip_span_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    lib.hc_ip_max_window.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
    return lib


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("6dgs_amd.ops")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def plan(hc, batch, height, width, resized_h, resized_w, out_size):
    p, s = np.zeros(5, np.int64), np.zeros(4, F)
    ok = hc.hc_ip_plan(batch, height, width, resized_h, resized_w, out_size, _ptr(p), _ptr(s))
    assert ok == int(p[4])
    return {"kt": int(p[0]), "rb": int(p[1]), "nrmax": int(p[2]), "lds_bytes": int(p[3]), "supported": bool(p[4]), "sh": s[0], "sw": s[1], "sup_h": s[2],
            "sup_w": s[3]}


def case_plan(hc, c):
    return plan(hc, c.batch, c.height, c.width, c.resized_h, c.resized_w, c.out_size)


def ulps(a, ref):
    """|a - ref| in units of ref's fp32 spacing."""
    ref = np.asarray(ref, F)
    return np.abs(np.asarray(a, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


# ---- the reference against PyTorch ------------------------------------------------------------------------------------------------
# (H, W) -> (resized_h, resized_w): downscale, upscale, off-dword odd sizes, one axis each way, an identity axis, a deep downscale of a sliver,
# the smallest image, a tiny odd one.  The whole resize is compared, so every border span is in it.
TORCH_SHAPES = (((300, 400), (256, 341)), ((180, 200), (224, 224)), ((261, 263), (256, 256)), ((200, 400), (256, 256)), ((256, 300), (256, 256)),
                ((1409, 37), (256, 31)), ((2, 2), (1, 1)), ((5, 7), (3, 11)), ((38, 38), (37, 37)))


@pytest.mark.parametrize("shape,resized", TORCH_SHAPES)
def test_reference_is_pytorchs_antialiased_bicubic(shape, resized):
    """With fp64 tap positions the restatement is PyTorch's CPU op in fp64 (<= 1e-12; measured 2e-15); evaluated in fp32 from fp32 tap
    positions it is the same op in fp32 (<= 2e-6; measured 8e-7)."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    v = rng.random((2, shape[0], shape[1], 3), dtype=F)
    t = torch.from_numpy(v).permute(0, 3, 1, 2)
    op64 = torch.nn.functional.interpolate(t.double(), size=resized, mode="bicubic", antialias=True, align_corners=False).numpy()
    op32 = torch.nn.functional.interpolate(t, size=resized, mode="bicubic", antialias=True, align_corners=False).numpy()
    r64 = R.resize_crop(v, resized[0], resized[1], 0, 0, resized[0], resized[1], np.float64, taps=np.float64)
    r32 = R.resize_crop(v, resized[0], resized[1], 0, 0, resized[0], resized[1], np.float32)
    e64, e32 = float(np.abs(r64 - op64).max()), float(np.abs(r32.astype(np.float64) - op32).max())
    print(f"[image_prep] {shape} -> {resized}: fp64 taps vs the fp64 op {e64:.3g}, fp32 vs the fp32 op {e32:.3g}")
    assert r64.dtype == np.float64 and r32.dtype == np.float32
    assert e64 <= 1e-12 and e32 <= 2e-6


# ---- spans and weights ------------------------------------------------------------------------------------------------------------
def test_spans_and_weights_of_every_case_axis(hc):
    """hc_ip_spans (aa_weights of image_prep_rules.h) on both axes of every case, over the crop's output indices: xmin and xsize exactly the
    restatement's, no xsize beyond kt, weights within 4 ulp of the restatement's fp32 weights, every row summing to 1 within 4 ulp (of 1;
    the weights added exactly, in fp64)."""
    worst_w, worst_sum = 0.0, 0.0
    for c in R.CASES:
        p = case_plan(hc, c)
        assert p["supported"], c.name
        for n, resized, i0, scale, support in ((c.height, c.resized_h, c.crop_top, p["sh"], p["sup_h"]), (c.width, c.resized_w, c.crop_left, p["sw"], p["sup_w"])):
            s_ref, sup_ref, _ = R.axis_scale(n, resized)
            assert scale == s_ref and support == sup_ref, c.name
            kt, count = p["kt"], c.out_size
            w, meta, full = np.full((count, kt), np.nan, F), np.zeros((count, 2), np.int32), np.zeros(count, np.int32)
            hc.hc_ip_spans(i0, count, n, scale, support, kt, _ptr(w), _ptr(meta))
            hc.hc_ip_span_sizes(i0, count, n, scale, support, _ptr(full))
            xmin, xsize, w_ref = R.axis_weights(n, resized, i0, count, np.float32)
            assert np.array_equal(meta[:, 0], xmin) and np.array_equal(full, xsize), c.name
            assert int(full.max()) <= kt and np.array_equal(meta[:, 1], xsize), (c.name, int(full.max()), kt)
            assert int(xsize.min()) >= 1 and int(xmin.min()) >= 0 and int((xmin + xsize).max()) <= n, c.name
            K = w_ref.shape[1]
            assert not w[:, K:].any(), c.name                                        # zero beyond the span
            worst_w = max(worst_w, float(ulps(w[:, :K], w_ref).max()))
            sums = w.astype(np.float64).sum(1)
            worst_sum = max(worst_sum, float(np.abs(sums - 1.0).max() / np.spacing(F(1.0))))
            assert float(ulps(w[:, :K], w_ref).max()) <= 4.0, c.name
            assert float(np.abs(sums - 1.0).max()) <= 4.0 * float(np.spacing(F(1.0))), (c.name, n, resized)
    print(f"[image_prep] weights: worst distance from the restatement {worst_w:.3g} ulp, worst row sum {worst_sum:.3g} ulp of 1 from 1")


def test_an_axis_at_scale_one_has_identity_weights(hc):
    """256 rows to 256 rows: every output row's weights are exactly (0, 1, 0, 0) on rows i - 1 .. i + 2 (cut at the edges): the cubic is
    0 at 1 and 2 and 1 at 0, so the row passes through unchanged."""
    c = R.BY_NAME["identity_rows"]
    p = case_plan(hc, c)
    assert p["sh"] == F(1.0) and p["sup_h"] == F(2.0)
    w, meta = np.zeros((256, p["kt"]), F), np.zeros((256, 2), np.int32)
    hc.hc_ip_spans(0, 256, 256, p["sh"], p["sup_h"], p["kt"], _ptr(w), _ptr(meta))
    for i in range(256):
        dense = np.zeros(256, F)
        dense[meta[i, 0]:meta[i, 0] + meta[i, 1]] = w[i, :meta[i, 1]]
        want = np.zeros(256, F)
        want[i] = 1.0
        assert np.array_equal(dense, want), i
    _, _, w_ref = R.axis_weights(256, 256, 0, 256, np.float64)
    assert set(np.unique(w_ref).tolist()) <= {0.0, 1.0} and np.array_equal(w_ref.sum(1), np.ones(256))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_of_the_named_cases(hc):
    """The band height each case is there for, and the two refusals: 2151 x 260 (not even one row's window fits the LDS budget) and
    260 x 4000 (scale 15.6: more than 64 padded taps)."""
    for c in R.CASES:
        p = case_plan(hc, c)
        print(f"[image_prep] plan {c.name}: kt={p['kt']} rb={p['rb']} nrmax={p['nrmax']} lds={p['lds_bytes']}")
        assert p["supported"] and p["lds_bytes"] <= LDS_BUDGET and p["kt"] % 4 == 0 and p["kt"] <= 64, c.name
        if c.rb is not None:
            assert p["rb"] == c.rb, (c.name, p)
    assert sorted({c.rb for c in R.CASES if c.rb is not None}) == [1, 2, 4, 8]
    b, h, w, nh, nw, _, _, s = R.UNSUPPORTED[0]
    p = plan(hc, b, h, w, nh, nw, s)
    assert not p["supported"] and p["kt"] <= 64 and p["rb"] == 0 and p["lds_bytes"] > LDS_BUDGET
    b, h, w, nh, nw, _, _, s = R.UNSUPPORTED[1]
    p = plan(hc, b, h, w, nh, nw, s)
    assert not p["supported"] and p["kt"] > 64


def test_no_band_outgrows_the_rows_the_plan_reserves(hc, ops):
    """Every height from 8 to 4096, square, 4:3 and 3:4, batches 1 and 16, at Resize / CenterCrop pairs (256, 224), (224, 224), (448, 448)
    and (518, 518) with the geometry of ops.image_prep_geometry: wherever the plan takes the shape, every band's row window r1 - r0 (as
    the kernel forms it) is at most nrmax -- the kernel clamps to nrmax silently, so this is what keeps its rows the right ones --, the
    LDS bytes are within 150 KB and kt is a multiple of 4 and at most 64."""
    seen_rb, supported, refused, slack = set(), 0, 0, None
    for resize, crop in ((256, 224), (224, 224), (448, 448), (518, 518)):
        for height in range(8, 4097):
            for width in (height, height * 4 // 3, height * 3 // 4):
                nh, nw, top, left = ops.image_prep_geometry(height, width, resize, crop)
                assert top >= 0 and left >= 0 and top + crop <= nh and left + crop <= nw
                for batch in (1, 16):
                    p = plan(hc, batch, height, width, nh, nw, crop)
                    if not p["supported"]:
                        refused += 1
                        continue
                    supported += 1
                    seen_rb.add(p["rb"])
                    assert p["kt"] % 4 == 0 and 4 <= p["kt"] <= 64 and p["lds_bytes"] <= LDS_BUDGET and p["rb"] in (1, 2, 4, 8), (batch, height, width, p)
                    worst = hc.hc_ip_max_window(height, top, crop, p["rb"], p["sh"], p["sup_h"], p["kt"])
                    assert 1 <= worst <= p["nrmax"], (batch, height, width, resize, crop, worst, p)
                    slack = p["nrmax"] - worst if slack is None else min(slack, p["nrmax"] - worst)
    print(f"[image_prep] plan sweep: {supported} supported, {refused} refused, band heights {sorted(seen_rb)}, least slack nrmax - window = {slack}")
    assert seen_rb == {1, 2, 4, 8} and supported > 20000 and refused > 0


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_is_fit(name):
    """bound = max(FACTOR y, FLOOR scale) stays within CEILING scale: the fp32 evaluation of the restatement is close enough to fp64
    for the case to judge a kernel."""
    d = R.case_data(name)
    print(f"[image_prep] case {name}: scale={d['scale']:.4g} y={d['y']:.3g} bound={d['bound']:.3g} bound/scale={d['bound'] / d['scale']:.3g}")
    assert d["r64"].shape == (d["case"].batch, 3, d["case"].out_size, d["case"].out_size) and np.isfinite(d["r64"]).all()
    assert d["y"] > 0.0 or d["case"].out_size == 1
    assert d["fit"] and d["bound"] <= R.CEILING * d["scale"]
