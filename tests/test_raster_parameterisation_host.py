"""The switches of the two restatements (tests/raster_reference.py, tests/raster_backward_reference.py) without a GPU: raw scales and
raw opacities (scale_is_log / opacity_is_logit off), scale_modifier, and an active SH degree below the stored one, each held against an
identity of the definition in fp64; and the fitness, under the caps the files already have, of every case
tests/test_gpu_raster_parameterisation.py puts to the GPU, so that an unfit input fails here.

The identities run on fp64 tensors given to RB.render directly, so that the raw arrays are exp / sigmoid of the stored ones to fp64
rounding; only the discrete parts (which Gaussians are live, their rectangles and order) see them rounded to fp32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_backward_reference as RB  # noqa: E402
import raster_parameterisation_cases as PC  # noqa: E402
import raster_reference as RR  # noqa: E402

torch = pytest.importorskip("torch")

N, SCENE_SEED, VIEWS, CAM_SEED, WIDTH, HEIGHT = RB.PARAM_BASE
# Both sides of an identity are the same fp64 operations but for the exp / sigmoid / log moved outside the restatement: they differ by
# fp64 rounding (1.1e-16) carried through sums of some thousand terms with cancellation.  1e-9 of the array's largest entry is seven
# orders above that and five below the fp32 rounding a wrong chain rule could hide in (measured: see the tests' output).
IDENTITY = 1e-9


@pytest.fixture(scope="module")
def base(syn):
    scene = syn.make_scene(N, SCENE_SEED)
    rows = RR.camera_rows(syn.make_cameras(VIEWS, CAM_SEED, width=WIDTH, height=HEIGHT))
    g = RB.loss_weights((VIEWS, HEIGHT, WIDTH, 4), np.zeros((VIEWS, HEIGHT, WIDTH), bool))
    return scene, rows, g


def _autograd(t64, rows, g, sh_degree=3, **kw):
    """fp64 image and gradients of sum(g image) by the fp64 arrays t64 (not rounded to fp32 on the way in)."""
    t = {k: torch.from_numpy(np.ascontiguousarray(t64[k], np.float64)).requires_grad_(True) for k in RB.NAMES[:-1]}
    cams = torch.from_numpy(rows.astype(np.float64)).requires_grad_(True)
    image = RB.render(t, cams, WIDTH, HEIGHT, sh_degree, **kw)
    (image * torch.from_numpy(g.astype(np.float64))).sum().backward()
    out = {k: t[k].grad.numpy() for k in RB.NAMES[:-1]}
    out["cams"] = cams.grad.numpy()
    out["image"] = image.detach().numpy()
    return out


def _same(a, b, what):
    scale = float(np.abs(b).max())
    err = float(np.abs(a - b).max())
    print(f"{what}: max difference {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e}")
    assert scale > 0 and err <= IDENTITY * scale, what


def test_raw_scale_and_raw_opacity(base):
    """d / d scale = (d / d log scale) / scale; d / d o = (d / d logit) / (o (1 - o)); the images are equal; no other gradient moves."""
    scene, rows, g = base
    t = {k: np.asarray(scene[k], np.float64) for k in RB.NAMES[:-1]}
    stored = _autograd(t, rows, g)
    s, o = np.exp(t["log_scale"]), 1.0 / (1.0 + np.exp(-t["opacity"]))
    for what, kw, raw in (("raw scale", dict(scale_is_log=False), dict(t, log_scale=s)),
                          ("raw opacity", dict(opacity_is_logit=False), dict(t, opacity=o)),
                          ("both raw", dict(scale_is_log=False, opacity_is_logit=False), dict(t, log_scale=s, opacity=o))):
        got = _autograd(raw, rows, g, **kw)
        want = dict(stored)
        if "scale_is_log" in kw:
            want["log_scale"] = stored["log_scale"] / s
        if "opacity_is_logit" in kw:
            want["opacity"] = stored["opacity"] / (o * (1.0 - o))
        for k in RB.NAMES + ("image",):
            _same(got[k], want[k], f"{what}, {k}")
    # the switches are not ignored: the stored arrays taken as raw values give another image
    assert np.abs(_autograd(dict(t, log_scale=s), rows, g)["image"] - stored["image"]).max() > 1e-3


@pytest.mark.parametrize("m", (0.5, 1.7))
def test_scale_modifier(base, m):
    """scale_modifier = m is log_scale + log m at modifier 1: the same image and the same d log_scale (and everything else); with raw
    scales it is m scale at modifier 1, and d / d scale is m times that one's."""
    scene, rows, g = base
    t = {k: np.asarray(scene[k], np.float64) for k in RB.NAMES[:-1]}
    got = _autograd(t, rows, g, scale_modifier=m)
    want = _autograd(dict(t, log_scale=t["log_scale"] + np.log(m)), rows, g)
    for k in RB.NAMES + ("image",):
        _same(got[k], want[k], f"modifier {m}, {k}")
    assert np.abs(got["image"] - _autograd(t, rows, g)["image"]).max() > 1e-3
    s = np.exp(t["log_scale"])
    raw = _autograd(dict(t, log_scale=s), rows, g, scale_modifier=m, scale_is_log=False)
    _same(raw["image"], want["image"], f"raw scale, modifier {m}, image")
    _same(raw["log_scale"], want["log_scale"] / s, f"raw scale, modifier {m}, d scale")
    _same(raw["log_scale"], m * _autograd(dict(t, log_scale=m * s), rows, g, scale_is_log=False)["log_scale"], f"raw scale, modifier {m}, d scale (2)")


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_active_degree_of_sixteen_stored(base, degree):
    """Degree d of 16 stored coefficients: the image and every gradient of the scene truncated to (d + 1)^2 coefficients, bit for bit;
    exact zeros in d f_rest from coefficient (d + 1)^2 on, and nonzero entries before."""
    scene, rows, g = base
    nb = (degree + 1) ** 2
    full = dict(scene, sh_degree=degree)
    cut = dict(scene, sh_degree=degree, f_rest=scene["f_rest"][:, :nb - 1])
    for dtype in (np.float64, np.float32):
        a = RB.gradients(full, rows, WIDTH, HEIGHT, dtype, g)
        b = RB.gradients(cut, rows, WIDTH, HEIGHT, dtype, g)
        assert a["f_rest"].shape == (N, 15, 3) and not a["f_rest"][:, nb - 1:].any()
        assert degree == 0 or np.abs(a["f_rest"][:, :nb - 1]).max(axis=(0, 2)).min() > 0          # every active coefficient gets some
        assert np.array_equal(a["f_rest"][:, :nb - 1], b["f_rest"])
        for k in RB.NAMES + ("image",):
            if k != "f_rest":
                assert np.array_equal(a[k], b[k]), k
    # RR agrees, and the degree matters
    r = {d: RR.reference_views(dict(scene, sh_degree=d), rows, WIDTH, HEIGHT, np.float64, background=RR.BACKGROUND)["image"] for d in (degree, degree + 1)}
    assert np.array_equal(r[degree], RR.reference_views(cut, rows, WIDTH, HEIGHT, np.float64, background=RR.BACKGROUND)["image"])
    assert np.abs(r[degree] - r[degree + 1]).max() > 1e-3


def test_rr_takes_the_switches(base):
    """RR.reference_views with raw arrays (rounded to fp32, as the kernel gets them) against the stored ones: the same discrete answers on
    decidable Gaussians, and images that differ by the rounding of the raw arrays alone."""
    scene, rows, _ = base
    stored = RR.reference_views(scene, rows, WIDTH, HEIGHT, np.float64, background=RR.BACKGROUND)
    raw = RR.reference_views(RR.raw_scene(scene, False, False), rows, WIDTH, HEIGHT, np.float64, background=RR.BACKGROUND, scale_is_log=False,
                             opacity_is_logit=False)
    dec = stored["decidable"] & raw["decidable"]
    und = stored["undecidable"] | raw["undecidable"]
    assert np.array_equal(stored["radii"][dec], raw["radii"][dec]) and dec.mean() > 0.99 and und.mean() <= RR.MAX_UNDECIDABLE_SHARE
    # 2^-24 relative on a scale moves the covariance by 2^-23 and the power by 2^-23 |power| <= 2^-23 log 255; with the opacity's own
    # 2^-24 an alpha moves by at most 12 x 2^-24 = 7e-7 of itself, and a pixel adds up to some ten of them: 1e-5
    err = float(np.abs(stored["image"] - raw["image"])[~und].max())
    print(f"raw arrays rounded to fp32: the fp64 image moves by {err:.3e}")
    assert 0 < err <= 1e-5


@pytest.mark.parametrize("name,args,kw", RB.PARAM_CASES, ids=[c[0] for c in RB.PARAM_CASES])
def test_every_gpu_case_is_fit(syn, name, args, kw):
    """Undecidable share <= RR.MAX_UNDECIDABLE_SHARE, image bound <= RR.ERROR_CEILING, every gradient bound <= RB.CEILING of its scale;
    the restatement's fp64 image is raster_reference's."""
    c = RB.case(syn, *args, **kw)
    share, limit = c["rr"]["undecidable"].mean(), RR.bound(c["rr"]["rounding"])
    print(f"{name}: undecidable {share:.5f}, image bound {limit:.3e}")
    assert share <= RR.MAX_UNDECIDABLE_SHARE and limit <= RR.ERROR_CEILING
    assert np.abs(c["g64"]["image"] - c["rr"]["r64"]["image"]).max() <= 1e-12
    assert not c["g"][c["rr"]["undecidable"]].any()
    for k, (scale, y, bound) in c["bounds"].items():
        print(f"{name} {k}: scale {scale:.3e}, y / scale {y / scale if scale else 0:.2e}, bound / scale {bound / scale if scale else 0:.2e}")
        if k == "f_rest" and args[6] == 0:          # nothing is active: empty, or exact zeros in both precisions
            assert c["g64"][k].shape == (N, 15 if kw.get("stored_degree") else 0, 3) and not c["g64"][k].any() and not c["g32"][k].any()
            continue
        assert scale > 0 and bound == max(RB.FACTOR * y, RB.FLOOR * scale) and bound <= RB.CEILING * scale, k
    assert (RR.MAX_UNDECIDABLE_SHARE, RR.ERROR_CEILING, RB.FACTOR, RB.FLOOR, RB.CEILING) == (2e-3, 5e-5, 8.0, 1e-6, 1e-4)


def test_default_cases_keep_their_values(syn):
    """The keyword arguments at their defaults name the case the positional call names: one cache entry, the same objects."""
    a = RB.case(syn, *RB.PARAM_BASE, 0)
    b = RB.case(syn, *RB.PARAM_BASE, 0, stored_degree=0, scale_is_log=True, opacity_is_logit=True, scale_modifier=1.0)
    assert a is b and a["rr"] is RR.case(syn, *RB.PARAM_BASE, 0) and a["scene"]["f_rest"].shape == (N, 0, 3)
    assert RB.case(syn, *RB.PARAM_BASE, 0, stored_degree=3)["scene"]["f_rest"].shape == (N, 15, 3)


@pytest.mark.parametrize("which", ("66 000 Gaussians", "early stop A", "early stop B"))
def test_the_large_and_the_early_stop_scenes_are_fit(syn, which):
    """What tests/test_gpu_raster_parameterisation.py asserts of its other scenes from the restatement alone -- the fillers are culled and
    decidable and the image is the 300-Gaussian scene's; every Gaussian of an early-stop scene is in the one tile's list, nothing
    saturates before the stoppers and every pixel stops at the third of them -- and their fitness under the same caps."""
    c = PC.check_big_case(syn)[0] if which[0] == "6" else PC.early_stop_case(which[-1])[0]
    share, limit = c["rr"]["undecidable"].mean(), RR.bound(c["rr"]["rounding"])
    print(f"{which}: undecidable {share:.5f}, image bound {limit:.3e}, instances {c['rr']['r64']['instances']}")
    assert share <= RR.MAX_UNDECIDABLE_SHARE and limit <= RR.ERROR_CEILING
    assert np.abs(c["g64"]["image"] - c["rr"]["r64"]["image"]).max() <= 1e-12
    for k, (scale, y, bound) in c["bounds"].items():
        print(f"{which} {k}: scale {scale:.3e}, y / scale {y / scale if scale else 0:.2e}, bound / scale {bound / scale if scale else 0:.2e}")
        if which[0] == "e" and k in ("rot", "f_rest"):       # isotropic Gaussians of degree 0: no d rot by symmetry, no f_rest
            assert scale <= 1e-12 * c["bounds"]["log_scale"][0]
            continue
        assert scale > 0 and bound <= RB.CEILING * scale, k
