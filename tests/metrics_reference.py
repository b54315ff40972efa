"""sixdgs_image_metrics (include/sixdgs.h) restated in numpy and torch on the CPU, on tests/photometric_reference.py's blur and SSIM map.

The two input rules are fp32 by definition and are applied in fp32 for both restatements; from the values on, `evaluate` runs in the
dtype asked for: fp64 is the reference of the GPU tests, the fp32 run's own distance from it sets the bounds, by
photometric_reference.bounds -- bound = max(8 y, 1e-6 scale), a case fit only when the bound stays below 1e-4 scale.  With quantise
the L1 and squared-error sums are integers, so `exact` holds the fp32 outputs every implementation must reproduce to the bit.

Cases: photometric_reference.CASES, inputs drawn from [-0.25, 1.25] so that both rules act, with special values planted in the image and
in the float target: NaN, +-inf, every half point (k + 0.5) / 255 of the 8-bit rule and its fp32 neighbours on either side."""
import numpy as np
import torch

import photometric_reference as PR

CASES = PR.CASES
F255, HALF = np.float32(255.0), np.float32(0.5)
KEYS = ("l1", "ssim", "mse", "mse_c")


def to_byte(x):
    """The 8-bit rule in fp32: trunc(min(max(x * 255 + 0.5, 0), 255)); NaN counts as 0 (fmax and fmin return the other operand)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(x, np.float32) * F255 + HALF
        return np.trunc(np.fmin(np.fmax(t, np.float32(0.0)), F255)).astype(np.uint8)


def to_byte_rint(x):
    """sixdgs_raster_views' image_u8 rule, round(255 clamp(x, 0, 1)) to nearest even: NOT the rule of a saved PNG."""
    with np.errstate(invalid="ignore"):
        return np.rint(F255 * np.fmin(np.fmax(np.asarray(x, np.float32), np.float32(0.0)), np.float32(1.0))).astype(np.uint8)


def values(x, quantise):
    """An fp32 input after the rule, in fp32."""
    x = np.asarray(x, np.float32)
    if quantise:
        return to_byte(x).astype(np.float32) / F255
    return np.fmin(np.fmax(x, np.float32(0.0)), np.float32(1.0))


def half_points():
    """(k + 0.5) / 255 as the fp32 quotient, k = 0 .. 254."""
    return (np.arange(255, dtype=np.float32) + HALF) / F255


def specials():
    h = half_points()
    return np.concatenate([np.array([np.nan, np.inf, -np.inf], np.float32), h, np.nextafter(h, np.float32(-1.0)), np.nextafter(h, np.float32(2.0))])


def psnr(mse):
    """float32(10 log10(1 / mse)), the logarithm in fp64 from the fp32 mse: metrics.py's PSNR of a [1,3,H,W] pair; inf at 0."""
    m = np.asarray(mse, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(1.0 / m)).astype(np.float32)


def psnr_channels(mse_c):
    """The mean of the three channels' PSNRs (train.py's psnr(image, gt).mean() on [3,H,W] tensors), formed in fp64."""
    m = np.asarray(mse_c, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(1.0 / m)).mean(axis=-1).astype(np.float32)


def evaluate(image, target, quantise, dtype, target_is_u8=False):
    """image fp32 [V,H,W,>=3]; target fp32 [V,H,W,>=3] or, with target_is_u8, bytes [V,H,W,3] -> dict of numpy arrays in `dtype`:
    l1, ssim, mse [V], mse_c [V,3]; render_u8 [V,H,W,3]; and with quantise `exact`: the fp32 [V,6] rows' l1 and mse columns from the
    integer sums (NaN in the ssim column)."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    raw = np.asarray(image, np.float32)[..., :3]
    a32 = values(raw, quantise)
    b32 = PR.u8_value(np.asarray(target)[..., :3]) if target_is_u8 else values(np.asarray(target, np.float32)[..., :3], quantise)
    a, b = torch.from_numpy(np.ascontiguousarray(a32)).to(td), torch.from_numpy(np.ascontiguousarray(b32)).to(td)
    v, h, w, _ = a.shape
    n3, n1 = torch.tensor(float(np.float32(3 * h * w)), dtype=td), torch.tensor(float(np.float32(h * w)), dtype=td)
    m = PR.ssim_map(a, b)[0]
    d = a - b
    s_c = (d * d).reshape(v, -1, 3).sum(1)
    out = {"l1": (d.abs().reshape(v, -1).sum(1) / n3).numpy(), "ssim": (m.reshape(v, -1).sum(1) / n3).numpy(),
           "mse": (((s_c[:, 0] + s_c[:, 1]) + s_c[:, 2]) / n3).numpy(), "mse_c": (s_c / n1).numpy(), "render_u8": to_byte(raw)}
    if quantise:
        ua = to_byte(a32).astype(np.int64)
        ub = to_byte(b32).astype(np.int64)
        du = (ua - ub).reshape(v, -1, 3)
        s1, s2 = np.abs(du).sum(axis=(1, 2)), (du * du).sum(axis=1)
        exact = np.full((v, 6), np.nan, np.float32)
        exact[:, 0] = (s1.astype(np.float64) / (255.0 * (3 * h * w))).astype(np.float32)
        exact[:, 2] = (s2.sum(axis=1).astype(np.float64) / (65025.0 * (3 * h * w))).astype(np.float32)
        exact[:, 3:] = (s2.astype(np.float64) / (65025.0 * (h * w))).astype(np.float32)
        out["exact"] = exact
    return out


def bounds(r64, r32):
    return PR.bounds({k: r64[k] for k in KEYS}, {k: r32[k] for k in KEYS})


def inputs(views, height, width, seed=0):
    """image fp32 [V,H,W,4] and float target [V,H,W,4] from [-0.25, 1.25] with the special values planted in their first three
    channels (as many as a quarter of the entries holds, all of them from 32 x 32 pixels on), and a byte target [V,H,W,3]."""
    rng = np.random.default_rng(7000 * seed + 100 * views + 10 * height + width)
    sp = specials()
    out = {"target_u8": rng.integers(0, 256, (views, height, width, 3), dtype=np.uint8)}
    for name in ("image", "target_f"):
        x = (rng.random((views, height, width, 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
        entries = views * height * width * 3
        count = min(sp.size, entries // 4)
        at = rng.choice(entries, size=count, replace=False)
        rgb = x[..., :3].reshape(-1).copy()
        rgb[at] = sp[(np.arange(count) + (height if name == "image" else width)) % sp.size] if count < sp.size else rng.permutation(sp)
        x[..., :3] = rgb.reshape(views, height, width, 3)
        out[name] = x
    return out


_cache = {}


def case(views, height, width, quantise, u8):
    """Inputs, both restatements and the bounds of one parity case (computed once per process, shared, never written)."""
    key = (views, height, width, bool(quantise), bool(u8))
    if key not in _cache:
        x = inputs(views, height, width)
        target = x["target_u8"] if u8 else x["target_f"]
        r64 = evaluate(x["image"], target, quantise, np.float64, u8)
        r32 = evaluate(x["image"], target, quantise, np.float32, u8)
        _cache[key] = {"x": x, "r64": r64, "r32": r32, "bounds": bounds(r64, r32)}
    return _cache[key]
