"""The held-out-view metrics without a GPU: the fp64 restatement (tests/metrics_reference.py) against the reference's stored values;
the 8-bit rule on every byte and at its half points; the fitness of every parity case; the PSNR helpers at mse == 0; and the calls
sixdgs_image_metrics and sixdgs_evaluate_views refuse before any device work."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as MR  # noqa: E402
import photometric_reference as PR  # noqa: E402

torch = pytest.importorskip("torch")

# max |fp64 restatement - reference| / scale over the four pairs and both modes, as tools/gen_metrics_golden.py printed it (the
# reference's window is normalised and multiplied out in fp32: the SSIM figure).  The bound is 8 x that; where the two agreed to the
# last bits, 1e-12 of the scale for the fp64 sums' own rounding.
GOLDEN_MEASURED = {"l1": 0.0, "ssim": 9.47e-7, "ssim4": 9.47e-7, "psnr": 3.12e-16, "psnr_channels": 3.12e-16}
GOLDEN_BOUND = {k: max(8.0 * v, 1e-12) for k, v in GOLDEN_MEASURED.items()}
MODES = ("clamp", "u8")
BADARG, WORKSPACE = -1, -2


def restated(r):
    """metrics_reference.evaluate's fp64 result of one view -> the golden file's five quantities."""
    return {"l1": r["l1"][0], "ssim": r["ssim"][0], "ssim4": r["ssim"][0], "psnr": 10.0 * np.log10(1.0 / r["mse"][0]),
            "psnr_channels": (10.0 * np.log10(1.0 / r["mse_c"][0])).mean()}


def test_restatement_against_the_reference(golden):
    g = golden("g17_metrics")
    assert list(g["names"]) == ["r5x7", "r16x16", "r33x17", "shift24x40"]
    for name in g["names"]:
        image, target = g[f"{name}_image"], g[f"{name}_target"]
        assert image.dtype == np.float32 and image.shape == target.shape and image.shape[2] == 3
        assert image.min() < -0.2 and image.max() > 1.2                    # both rules act
        # the bytes a real PNG held are the rule's
        assert np.array_equal(MR.to_byte(image), g[f"{name}_image_u8"]) and np.array_equal(MR.to_byte(target), g[f"{name}_target_u8"])
        for mode in MODES:
            got = restated(MR.evaluate(image[None], target[None], mode == "u8", np.float64))
            for k, v in got.items():
                ref = float(g[f"{name}_{mode}_{k}"])
                print(f"{name} {mode} {k}: {abs(v - ref) / abs(ref):.2e} of the scale (bound {GOLDEN_BOUND[k]:.2e})")
                assert abs(v - ref) <= GOLDEN_BOUND[k] * abs(ref), (name, mode, k)
    assert max(GOLDEN_MEASURED.values()) <= 1e-5                           # more would mean a wrong restatement


def test_the_8_bit_rule_maps_every_byte_to_itself():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(MR.to_byte(PR.u8_value(u)), u)
    assert np.array_equal(MR.to_byte(MR.values(PR.u8_value(u), True)), u)
    # and the byte of a clamped value is the byte of the value: the kernel forms render_u8 from what it staged
    x = np.concatenate([MR.specials(), np.linspace(-0.3, 1.3, 4001).astype(np.float32)])
    assert np.array_equal(MR.to_byte(MR.values(x, False)), MR.to_byte(x)) and np.array_equal(MR.to_byte(MR.values(x, True)), MR.to_byte(x))
    assert MR.to_byte(np.float32("nan")) == 0 and MR.to_byte(np.float32("inf")) == 255 and MR.to_byte(np.float32("-inf")) == 0
    assert MR.values(np.float32("nan"), False) == 0 and MR.values(np.float32("inf"), False) == 1 and MR.values(np.float32("-inf"), False) == 0


def test_the_8_bit_rule_is_not_the_rasterisers_rounding():
    """trunc(x 255 + 0.5) and rint(255 x) disagree at half of the half points: a kernel that reused image_u8's rule fails on the
    planted values."""
    h = MR.half_points()
    differ = MR.to_byte(h) != MR.to_byte_rint(h)
    print(f"{int(differ.sum())} of {h.size} half points differ")
    assert 100 <= int(differ.sum()) <= 155
    planted = MR.inputs(2, 40, 24)["image"][..., :3]
    finite = np.isfinite(planted)
    assert int((MR.to_byte(planted[finite]) != MR.to_byte_rint(planted[finite])).sum()) >= 100
    assert np.isnan(planted).any() and np.isposinf(planted).any() and np.isneginf(planted).any()


@pytest.mark.parametrize("views,height,width", MR.CASES)
def test_every_case_is_fit(views, height, width):
    for quantise in (False, True):
        for u8 in (False, True):
            c = MR.case(views, height, width, quantise, u8)
            for k, (scale, y, bound) in c["bounds"].items():
                print(f"{views}x{height}x{width} quantise={quantise} u8={u8} {k}: y / scale {y / scale:.2e}, bound / scale {bound / scale:.2e}")
                assert scale > 0 and np.isfinite(c["r64"][k]).all() and bound <= PR.CEILING * scale, k
            if quantise:
                # the integer sums' outputs are the fp64 restatement's, rounded once
                e = c["r64"]["exact"]
                assert np.array_equal(e[:, 0], c["r64"]["l1"].astype(np.float32)) or np.abs(e[:, 0] - c["r64"]["l1"]).max() <= 1e-7
                assert np.abs(e[:, 3:] - c["r64"]["mse_c"]).max() <= 1e-7 and np.abs(e[:, 2] - c["r64"]["mse"]).max() <= 1e-7


def test_psnr_helpers():
    ev = importlib.import_module("6dgs_amd.evaluate")
    mse = np.array([0.0, 1.0, 0.25, 1e-4], np.float32)
    for f in (MR.psnr, ev.psnr_of_mse):
        p = f(mse)
        assert p.dtype == np.float32 and np.isposinf(p[0]) and p[1] == 0 and p[3] == np.float32(10.0 * np.log10(1.0 / np.float64(np.float32(1e-4))))
    for f in (MR.psnr_channels, ev.psnr_of_channels):
        assert np.isposinf(f(np.array([[0.0, 0.5, 0.5]], np.float32))[0])
        assert f(np.array([[0.1, 0.01, 0.001]], np.float32))[0] == np.float32(20.0)
    assert np.array_equal(ev.psnr_of_mse(mse), MR.psnr(mse))
    s = ev.summarise(np.array([[0.1, 0.9, 0.01, 0.01, 0.01, 0.01], [0.2, 0.8, 0.0, 0.0, 0.0, 0.0]], np.float32))
    assert s["psnr"][0] == np.float32(20.0) and np.isposinf(s["psnr"][1]) and np.isposinf(s["mean_psnr"])
    assert s["mean_l1"] == torch.tensor([0.1, 0.2]).mean().item() and s["mean_ssim"] == torch.tensor([0.9, 0.8]).mean().item()


# ---- the C entry points: refused before the first HIP call (the pointers are 256-aligned dummy integers, never dereferenced) --------
P = 256
N, V, W, H = 5, 2, 16, 16


def _metrics(L, **kw):
    a = dict(image=P, image_stride=4, target=P, is_u8=0, stride=3, views=V, width=W, height=H, quantise=0, metrics=P, ws=P, ws_bytes=0)
    a.update(kw)
    need = L.sixdgs_image_metrics_workspace_bytes(max(a["views"], 0), W, H)
    return L.sixdgs_image_metrics(a["image"], a["image_stride"], a["target"], a["is_u8"], a["stride"], a["views"], a["width"], a["height"],
                                  a["quantise"], a["metrics"], None, a["ws"], need + a["ws_bytes"], None, None)


def _evaluate(L, **kw):
    a = dict(xyz=P, scale=P, rot=P, opacity=P, f_dc=P, f_rest=P, sh_degree=3, n_coef=16, n=N, cams=P, views=V, width=W, height=H,
             scale_modifier=1.0, background=P, target=P, is_u8=0, stride=3, quantise=1, chunk=2, max_instances=4096, metrics=P, status=P,
             needed=P, ws=P, ws_bytes=0)
    a.update(kw)
    need = L.sixdgs_evaluate_views_workspace_bytes(a["n"], max(a["chunk"], 1), W, H, a["max_instances"])
    return L.sixdgs_evaluate_views(a["xyz"], a["scale"], 1, a["rot"], a["opacity"], 1, a["f_dc"], a["f_rest"], a["sh_degree"], a["n_coef"], a["n"],
                                   a["cams"], a["views"], a["width"], a["height"], a["scale_modifier"], a["background"], a["target"], a["is_u8"],
                                   a["stride"], a["quantise"], a["chunk"], a["max_instances"], a["metrics"], None, a["status"], a["needed"],
                                   a["ws"], need + a["ws_bytes"], None)


SHARED = [(dict(is_u8=1, stride=4), BADARG), (dict(is_u8=2), BADARG), (dict(stride=2), BADARG), (dict(quantise=2), BADARG),
          (dict(quantise=-1), BADARG), (dict(width=0), BADARG), (dict(height=16385), BADARG), (dict(views=-1), BADARG), (dict(views=65536), BADARG),
          (dict(target=None), BADARG), (dict(target=P + 2), BADARG), (dict(metrics=None), BADARG), (dict(metrics=P + 2), BADARG),
          (dict(ws_bytes=-1), WORKSPACE), (dict(ws=P + 128), BADARG), (dict(ws=None), BADARG), (dict(views=0, ws=None, metrics=None), 0)]
METRICS_ROWS = SHARED + [(dict(image_stride=2), BADARG), (dict(image=None), BADARG), (dict(image=P + 1), BADARG)]
EVALUATE_ROWS = SHARED + [(dict(sh_degree=4), BADARG), (dict(sh_degree=2, n_coef=8), BADARG), (dict(scale_modifier=0.0), BADARG),
                          (dict(chunk=0), BADARG), (dict(max_instances=0), BADARG), (dict(cams=None), BADARG), (dict(status=None), BADARG),
                          (dict(needed=None), BADARG), (dict(needed=P + 4), BADARG), (dict(background=None), BADARG),
                          *[({k: None}, BADARG) for k in ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")]]


def refusals():
    L = importlib.import_module("6dgs_amd._lib").load()
    for name, call, rows in (("sixdgs_image_metrics", _metrics, METRICS_ROWS), ("sixdgs_evaluate_views", _evaluate, EVALUATE_ROWS)):
        for kw, status in rows:
            assert call(L, **kw) == status, (name, kw)
        # a bad argument wins over a short workspace; the ws pointer is looked at after the size
        assert call(L, quantise=2, ws_bytes=-1) == BADARG
        assert call(L, ws=P + 128, ws_bytes=-1) == WORKSPACE and call(L, ws=None, ws_bytes=-1) == WORKSPACE
    # a byte target may sit at any address: only the short workspace is left to refuse
    assert _metrics(L, is_u8=1, stride=3, target=P + 1, ws_bytes=-1) == WORKSPACE
    up = lambda x: (x + 255) // 256 * 256      # noqa: E731
    # the workspaces are answered without a GPU: 20 B per tile and view; 0 outside the limits
    assert L.sixdgs_image_metrics_workspace_bytes(2, 260, 272) == up(2 * 17 * 17 * 20)
    assert L.sixdgs_image_metrics_workspace_bytes(1, 16385, 16) == 0 and L.sixdgs_image_metrics_workspace_bytes(65536, 16, 16) == 0
    ev = L.sixdgs_evaluate_views_workspace_bytes(N, 2, W, H, 4096)
    assert ev == (up(L.sixdgs_raster_views_workspace_bytes(N, 2, W, H, 4096)) + up(L.sixdgs_image_metrics_workspace_bytes(2, W, H))
                  + up(2 * H * W * 16) + 256)
    assert L.sixdgs_evaluate_views_workspace_bytes(N, 0, W, H, 4096) == 0 and L.sixdgs_evaluate_views_workspace_bytes(N, 2, W, H, 0) == 0


def test_entry_points_refuse_before_any_device_work():
    refusals()
