"""sixdgs_image_prep (include/sixdgs.h; the comment above PrepArgs in csrc/vit.hip) restated in numpy from the operation's definition,
parametrised by dtype: fp64 is the reference of the GPU tests (tests/test_gpu_image_side_edges.py), the fp32 evaluation of the same
text sets the bounds by its own distance from fp64.

What is DEFINITION, evaluated in fp32 one operation at a time as written (none of them can fuse):
  per axis          scale = (float)n / (float)resized,  support = 2 scale if scale >= 1 else 2,  invscale = 1 / scale if scale >= 1 else 1
  per output index  center = scale (i + 0.5),  xmin = max((int)(center - support + 0.5), 0),  xsize = min((int)(center + support + 0.5), n) - xmin,
                    tap argument j: ((j + (xmin - center)) + 0.5) invscale
From those fp32 arguments on, everything is evaluated in `dtype`: the cubic (a = -0.5), the tap-order sum of the weights and the division
by it, the x-reduction and then the y-reduction (each a tap-order sum that starts from the first product), the table value (exact fp32
data) and (v - mean) / std.  PyTorch's fp64 CPU op evaluates the tap POSITIONS in fp64 too; `taps=np.float64` does the same (spans still
the fp32 ones) and is what tests/test_image_prep_host.py compares with that op -- it is 1e-6 .. 2.5e-5 away from the fp32 tap positions
the kernel and PyTorch's GPU op use, a distance of definition, not of rounding, so it is NOT what the kernel is held to.

Bound rule, the one of photometric_reference.py: per case scale = max |r64|, y = max |r32 - r64| of the restatement alone,
bound = max(FACTOR y, FLOOR scale), and a case is fit only when bound <= CEILING scale.
"""
from collections import namedtuple

import numpy as np

from photometric_reference import CEILING, FACTOR, FLOOR

F = np.float32
MEAN = np.asarray((0.485, 0.456, 0.406), F)             # IMAGENET_DEFAULT_MEAN / _STD as the fp32 the entry point receives
STD = np.asarray((0.229, 0.224, 0.225), F)
UNSUPPORTED = ((1, 2151, 260, 256, 256, 16, 16, 224),   # not even a band of one row fits the LDS budget
               (1, 260, 4000, 256, 256, 16, 16, 224))   # scale 15.6 along x: more than 64 padded taps


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def table(kind):
    """'div255': value / 255 as the product builds it (fp32 division); 'random': a fixed non-monotone table in [-1, 2), so that a wrong
    byte lane or channel cannot hide behind neighbouring values."""
    if kind == "div255":
        return np.arange(256, dtype=F) / F(255.0)
    return (np.random.default_rng(20240229).random(256) * 3.0 - 1.0).astype(F)


# ---- one axis ----------------------------------------------------------------------------------------------------------------------
def axis_scale(n, resized):
    """-> (scale, support, invscale), fp32."""
    scale = F(n) / F(resized)
    support = F(2.0) * scale if scale >= F(1.0) else F(2.0)
    invscale = F(1.0) / scale if scale >= F(1.0) else F(1.0)
    return scale, support, invscale


def axis_spans(n, resized, i0, count):
    """Output indices i0 .. i0 + count of the resized grid: -> (xmin [count], xsize [count], center [count] fp32), every step in fp32."""
    scale, support, _ = axis_scale(n, resized)
    i = np.arange(i0, i0 + count).astype(F)
    center = scale * (i + F(0.5))
    lo = ((center - support) + F(0.5)).astype(np.int64)            # C's (int): truncation
    hi = ((center + support) + F(0.5)).astype(np.int64)
    xmin = np.maximum(lo, 0)
    xsize = np.minimum(hi, n) - xmin
    return xmin, xsize, center


def cubic(x, dtype):
    """The a = -0.5 cubic convolution filter, bracketed as the definition writes it."""
    x = np.abs(np.asarray(x, dtype))
    a = dtype(-0.5)
    near = ((a + dtype(2)) * x - (a + dtype(3))) * x * x + dtype(1)
    far = (((x - dtype(5)) * x + dtype(8)) * x - dtype(4)) * a
    return np.where(x < 1, near, np.where(x < 2, far, dtype(0))).astype(dtype)


def axis_weights(n, resized, i0, count, dtype, taps=np.float32):
    """-> (xmin [count], xsize [count], w [count][K] in dtype, zero beyond xsize; K = the largest xsize).  taps = np.float32: the tap
    arguments are the definition's fp32 ones; np.float64: scale, centre and arguments in fp64 as PyTorch's fp64 CPU op forms them."""
    xmin, xsize, center = axis_spans(n, resized, i0, count)
    scale, _, invscale = axis_scale(n, resized)
    K = int(xsize.max())
    j = np.arange(K)
    if taps == np.float32:
        xmc = xmin.astype(F) - center
        arg = ((j.astype(F)[None, :] + xmc[:, None]) + F(0.5)) * invscale
        assert arg.dtype == F
    else:
        s64 = np.float64(n) / np.float64(resized)
        c64 = s64 * (np.arange(i0, i0 + count) + 0.5)
        inv64 = 1.0 / s64 if s64 >= 1.0 else 1.0
        arg = (j[None, :] + xmin[:, None] - c64[:, None] + 0.5) * inv64
    w = np.where(j[None, :] < xsize[:, None], cubic(arg.astype(dtype), dtype), dtype(0)).astype(dtype)
    total = w[:, 0].copy()
    for k in range(1, K):
        total = total + w[:, k]                                      # adding the zeros beyond xsize changes nothing
    return xmin, xsize, (w / total[:, None]).astype(dtype)


def _reduce(v, axis, xmin, w):
    """Tap-order sum along `axis` of v: out[..., o, ...] = v[xmin[o]] w[o][0] + v[xmin[o] + 1] w[o][1] + ..., from the first product."""
    n = v.shape[axis]
    shape = [1] * v.ndim
    shape[axis] = -1
    acc = None
    for k in range(w.shape[1]):
        idx = np.minimum(xmin + k, n - 1)                            # beyond xsize the weight is zero: any finite sample
        p = np.take(v, idx, axis=axis) * w[:, k].reshape(shape)
        acc = p if acc is None else acc + p
    return acc


def resize_crop(values, resized_h, resized_w, top, left, out_h, out_w, dtype, taps=np.float32):
    """values [B][H][W][C] fp32 -> [B][C][out_h][out_w] in dtype: the antialiased bicubic resize to (resized_h, resized_w), of which the
    window that starts at (top, left) is evaluated; rows reduced along x first, then along y."""
    values = np.asarray(values, F)
    _, H, W, _ = values.shape
    ymin, ysize, wy = axis_weights(H, resized_h, top, out_h, dtype, taps)
    xmin, _, wx = axis_weights(W, resized_w, left, out_w, dtype, taps)
    r0, r1 = int(ymin.min()), int((ymin + ysize).max())             # the input rows the window reads
    rows = values[:, r0:r1].astype(dtype)
    alongx = _reduce(rows, 2, xmin, wx)                              # [B][r1 - r0][out_w][C]
    out = _reduce(alongx, 1, ymin - r0, wy)                          # [B][out_h][out_w][C]
    assert out.dtype == dtype
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def evaluate(images_u8, table256, resized_h, resized_w, top, left, out_size, dtype, mean=MEAN, std=STD):
    """images [B][H][W][3] uint8 -> [B][3][out_size][out_size] in dtype = (crop(resize_aa(table256[value])) - mean[c]) / std[c]."""
    values = np.asarray(table256, F)[np.asarray(images_u8)]
    r = resize_crop(values, resized_h, resized_w, top, left, out_size, out_size, dtype)
    m, s = np.asarray(mean, F).astype(dtype), np.asarray(std, F).astype(dtype)
    return ((r - m[None, :, None, None]) / s[None, :, None, None]).astype(dtype)


def bound_of(r64, r32):
    """-> (scale = max |r64|, y = max |r32 - r64|, bound = max(FACTOR y, FLOOR scale), fit)."""
    scale = float(np.abs(r64).max())
    y = float(np.abs(r32.astype(np.float64) - r64).max())
    bound = max(FACTOR * y, FLOOR * scale)
    return scale, y, bound, bound <= CEILING * scale


# ---- the case table ----------------------------------------------------------------------------------------------------------------
# The cases whose geometry ops.image_prep itself produces (border_down, out_*) are also held to 5e-6 of PyTorch's GPU op, a figure stated for
# values / 255 normalised to [-2.2, 2.7]: they take the 'div255' table.  The random table goes to the others.
# rb: the band height the launcher's plan must give (None: whatever it gives; the plan is recorded all the same)
Case = namedtuple("Case", "name branch batch height width resized_h resized_w crop_top crop_left out_size table rb")


def _band(batch, height, rb, why, tab):
    return Case(f"band_b{batch}_h{height}", f"band height rb = {rb}: {why}", batch, height, 260, 256, 256, 16, 16, 224, tab, rb)


def _corner(name, top, left, tab):
    return Case(f"corner_{name}", f"{name} corner crop of a 256 x 341 resize: spans clipped at the image's edge on that side", 2, 300, 400, 256, 341, top, left, 224,
                tab, None)


def _size(s, why, tab, batch=2):
    return Case(f"out_{s}", f"output size {s}: {why}", batch, s + 1, s + 1, s, s, 0, 0, s, tab, None)


CASES = (
    # band heights, through the raw call: width 260 and a 256 x 256 resize keep the buffers small; crop 224 at (16, 16)
    _band(9, 300, 4, "9 x 28 = 252 bands of 8 rows would not fill 256 workgroups", "div255"),
    _band(10, 300, 8, "10 x 28 = 280 bands of 8 rows", "random"),
    _band(10, 1002, 8, "the tallest image whose 8-row bands fit the LDS budget", "div255"),
    _band(10, 1003, 4, "forced by LDS: one row taller than the 8-row limit", "random"),
    _band(1, 1408, 4, "the tallest image whose 4-row bands fit", "div255"),
    _band(1, 1409, 2, "forced by LDS", "random"),
    _band(1, 1834, 2, "the tallest image whose 2-row bands fit", "div255"),
    _band(1, 1835, 1, "forced by LDS", "random"),
    _band(1, 2150, 1, "the tallest image the kernel takes at this geometry", "div255"),
    # borders: the crop is the whole resize, so xmin is clamped to 0 and xsize cut at n on every side, and the spans renormalised
    Case("border_down", "whole resize, downscaled: clipped spans on all four sides", 2, 300, 300, 224, 224, 0, 0, 224, "div255", None),
    Case("border_up", "whole resize, upscaled: clipped spans on all four sides at support 2", 2, 180, 200, 224, 224, 0, 0, 224, "random", None),
    _corner("top_left", 0, 0, "random"),
    _corner("top_right", 0, 117, "div255"),
    _corner("bottom_left", 32, 0, "div255"),
    _corner("bottom_right", 32, 117, "random"),
    # mixed axes
    Case("mixed_up_down", "rows upscaled (200 -> 256), columns downscaled (400 -> 256): kt from the larger support", 2, 200, 400, 256, 256, 16, 16, 224, "random",
         None),
    Case("identity_rows", "rows at scale exactly 1 (256 -> 256): identity weights along y, columns 300 -> 256", 2, 256, 300, 256, 256, 16, 16, 224, "random", None),
    # output sizes, each from the smallest input that gives a downscale
    _size(1, "a single pixel, one ragged band of one row, spans clipped on both sides at once", "div255", batch=4),
    _size(37, "not a multiple of 4; ragged last band (37 = 9 x 4 + 1)", "div255"),
    _size(221, "not a multiple of 4; ragged last band (221 = 55 x 4 + 1)", "div255"),
    _size(448, "the second trip of the x loop (448 > 256)", "div255"),
    _size(518, "DINOv2's own size: second and third trip of the x loop, ragged last band (518 = 129 x 4 + 2)", "div255"),
    # byte alignment between the images of a batch: H W 3 mod 4 = 1 and 2, crop with the last row and column (last taps at the buffer's end)
    Case("bytes_mod1", "batch 3 of 261 x 263 (H W 3 mod 4 = 1): images 1 and 2 start off a dword; last row and column in the crop", 3, 261, 263, 256, 256, 32, 32,
         224, "random", None),
    Case("bytes_mod2", "batch 3 of 262 x 263 (H W 3 mod 4 = 2): images 1 and 2 start off a dword; last row and column in the crop", 3, 262, 263, 256, 256, 32, 32,
         224, "random", None),
)
CASE_NAMES = tuple(c.name for c in CASES)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_images(case):
    """Uniform random bytes (not smooth: every tap matters), fixed per case."""
    rng = np.random.default_rng(7000 + CASE_NAMES.index(case.name))
    return rng.integers(0, 256, (case.batch, case.height, case.width, 3), dtype=np.uint8)


_cache = {}


def case_data(name):
    """Inputs, both evaluations and the bound of one case (computed once per process, shared, never written)."""
    if name not in _cache:
        c = BY_NAME[name]
        u8, tab = case_images(c), table(c.table)
        r64 = evaluate(u8, tab, c.resized_h, c.resized_w, c.crop_top, c.crop_left, c.out_size, np.float64)
        r32 = evaluate(u8, tab, c.resized_h, c.resized_w, c.crop_top, c.crop_left, c.out_size, np.float32)
        scale, y, bound, fit = bound_of(r64, r32)
        for a in (u8, tab, r64, r32):
            a.setflags(write=False)
        _cache[name] = {"case": c, "u8": u8, "table": tab, "r64": r64, "r32": r32, "scale": scale, "y": y, "bound": bound, "fit": fit}
    return _cache[name]


def op_geometry(case, geometry):
    """True where (resized_h, resized_w, crop_top, crop_left) is what `geometry` (ops.image_prep_geometry) gives for a Resize(min side) +
    CenterCrop(out_size) of the case's image: the geometry ops.image_prep produces."""
    resize = min(case.resized_h, case.resized_w)
    return tuple(geometry(case.height, case.width, resize, case.out_size)) == (case.resized_h, case.resized_w, case.crop_top, case.crop_left)
