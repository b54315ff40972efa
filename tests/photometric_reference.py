"""sixdgs_photometric_loss (include/sixdgs.h) restated in torch, parametrised by dtype: fp64 is the reference of the GPU tests, the fp32
restatement follows the header's operation order (the blur's taps in ascending index, x then y; the moments, the SSIM value, the
three derivative maps and the gradient as the header brackets them; only the sums of step 7 are torch's) and its own distance from
fp64 sets the bounds.

Bound rule, the one of raster_backward_reference.py: per array scale = max |x64|, y = max |x32 - x64| of the restatement alone,
bound = max(FACTOR y, FLOOR scale), and a case is fit only when bound <= CEILING scale.  blur(a a) - mu1 mu1 cancels where a window is
flat -- inherent in the formula in fp32 -- so the parity cases are random images, which stay far under the ceiling; the flat and the
smooth image of `hard_case` are held to FACTOR y alone and reported in profiles/photometric_loss.md.
"""
import numpy as np
import torch

FACTOR = 8.0               # two fp32 evaluations in different summation orders, each within y of fp64, and not at the same entry
FLOOR = 1e-6               # of max |x64|
CEILING = 1e-4             # of max |x64|: a case whose bound passes it is not a fit case
C1, C2 = 1e-4, 9e-4

_g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
WINDOW64 = _g / _g.sum()                          # the fp64-normalised Gaussian, sigma 1.5
WINDOW = WINDOW64.astype(np.float32)              # the definition's w: its fp32 roundings (SIXDGS_SSIM_WINDOW)

# (views, height, width): a single pixel; smaller than the window; the window's size; one tile; one past a tile edge both ways;
# several tiles with a part-empty last one; 17 x 17 = 289 tiles per view, more than the 256 the sum kernel stages at a time, two views
CASES = ((1, 1, 1), (2, 5, 7), (1, 11, 11), (1, 16, 16), (3, 17, 33), (2, 40, 24), (2, 272, 260))
LAMBDAS = (0.0, 0.2, 1.0)


def blur(x, window=WINDOW):
    """x [V,H,W,C]: the separable 11-tap correlation, along x then along y, zeros outside, taps added in ascending index."""
    w = [float(v) for v in window]
    v, h, wd, c = x.shape
    pad = torch.zeros(v, h, wd + 10, c, dtype=x.dtype)
    pad[:, :, 5:5 + wd] = x
    acc = w[0] * pad[:, :, 0:wd]
    for k in range(1, 11):
        acc = acc + w[k] * pad[:, :, k:k + wd]
    pad = torch.zeros(v, h + 10, wd, c, dtype=x.dtype)
    pad[:, 5:5 + h] = acc
    acc = w[0] * pad[:, 0:h]
    for k in range(1, 11):
        acc = acc + w[k] * pad[:, k:k + h]
    return acc


def ssim_map(a, b, window=WINDOW):
    """-> (m, d_mu1, d_s1, d_s12), each [V,H,W,3], in the dtype of a and b and the header's bracketing."""
    c1, c2 = torch.tensor(C1, dtype=torch.float32).to(a.dtype), torch.tensor(C2, dtype=torch.float32).to(a.dtype)      # 1e-4f, 9e-4f
    mu1, mu2 = blur(a, window), blur(b, window)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(a * a, window) - mu1sq, blur(b * b, window) - mu2sq, blur(a * b, window) - mu12
    A1, A2, B1, B2 = 2 * mu12 + c1, 2 * s12 + c2, (mu1sq + mu2sq) + c1, (s1 + s2) + c2
    den = B1 * B2
    m = (A1 * A2) / den
    d_s1 = -(m / B2)
    d_s12 = (2 * A1) / den
    d_mu1 = (((2 * mu2) * A2) / den - ((2 * mu1) * m) / B1) - ((2 * mu1) * d_s1 + mu2 * d_s12)
    return m, d_mu1, d_s1, d_s12


def evaluate(image, target, lam, dtype, grad_loss=None, window=WINDOW):
    """image, target: fp32 arrays [V,H,W,>=3] (a uint8 target arrives as its fp32 u / 255); -> dict of numpy arrays in `dtype`:
    loss [V], parts [V,2], grad [V,H,W,3] by the header's two-pass formula."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    a = torch.from_numpy(np.ascontiguousarray(np.asarray(image, np.float32)[..., :3])).to(td)
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(target, np.float32)[..., :3])).to(td)
    v, h, w, _ = a.shape
    lam_t = torch.tensor(float(lam), dtype=torch.float32).to(td)
    n = torch.tensor(float(np.float32(3 * h * w)), dtype=td)
    m, d_mu1, d_s1, d_s12 = ssim_map(a, b, window)
    d = a - b
    l1 = d.abs().reshape(v, -1).sum(1) / n
    ssim = m.reshape(v, -1).sum(1) / n
    loss = (1 - lam_t) * l1 + lam_t * (1 - ssim)
    x = (blur(d_mu1, window) + (2 * a) * blur(d_s1, window)) + b * blur(d_s12, window)
    gl = torch.ones(v, dtype=td) if grad_loss is None else torch.from_numpy(np.asarray(grad_loss, np.float32)).to(td)
    grad = gl.reshape(v, 1, 1, 1) * (((1 - lam_t) / n) * torch.sign(d) - (lam_t / n) * x)
    return {"loss": loss.numpy(), "parts": torch.stack([l1, ssim], 1).numpy(), "grad": grad.numpy()}


def autograd_gradient(image, target, lam, window=WINDOW):
    """d sum_v loss_v / d image in fp64 by torch autograd through the forward formulas alone: what the two-pass formula must equal."""
    a = torch.from_numpy(np.asarray(image, np.float32)[..., :3].astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(np.asarray(target, np.float32)[..., :3].astype(np.float64))
    v, h, w, _ = a.shape
    m = ssim_map(a, b, window)[0]
    n = float(np.float32(3 * h * w))
    loss = (1 - lam) * (a - b).abs().reshape(v, -1).sum(1) / n + lam * (1 - m.reshape(v, -1).sum(1) / n)
    loss.sum().backward()
    return a.grad.numpy()


def bounds(r64, r32):
    """Per array: (scale = max |x64|, y = max |x32 - x64|, bound = max(FACTOR y, FLOOR scale))."""
    out = {}
    for k in r64:
        scale = float(np.abs(r64[k]).max())
        y = float(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        out[k] = (scale, y, max(FACTOR * y, FLOOR * scale))
    return out


def inputs(views, height, width, seed=0):
    """Random images: image fp32 [V,H,W,4] (a fourth channel to plant things in), target bytes [V,H,W,3], a float target [V,H,W,4]
    and grad_loss [V]."""
    rng = np.random.default_rng(1000 * seed + 100 * views + 10 * height + width)
    return {"image": rng.random((views, height, width, 4), dtype=np.float32), "target_u8": rng.integers(0, 256, (views, height, width, 3), dtype=np.uint8),
            "target_f": rng.random((views, height, width, 4), dtype=np.float32), "grad_loss": rng.standard_normal(views).astype(np.float32)}


def u8_value(u):
    """The definition's value of a byte: float(u) / 255.0f in fp32."""
    return np.asarray(u, np.float32) / np.float32(255.0)


_cache = {}


def case(views, height, width, lam, u8, with_grad_loss):
    """Inputs, both restatements and the bounds of one parity case (computed once per process, shared, never written)."""
    key = (views, height, width, lam, u8, with_grad_loss)
    if key not in _cache:
        x = inputs(views, height, width)
        target = u8_value(x["target_u8"]) if u8 else x["target_f"]
        gl = x["grad_loss"] if with_grad_loss else None
        r64 = evaluate(x["image"], target, lam, np.float64, gl)
        r32 = evaluate(x["image"], target, lam, np.float32, gl)
        _cache[key] = {"x": x, "r64": r64, "r32": r32, "bounds": bounds(r64, r32)}
    return _cache[key]


def hard_case(kind, size=48):
    """The images the ceiling excludes: 'smooth' = a sinusoid, 'flat' = 0.7 + 0.01 noise; target = the image plus a little noise."""
    rng = np.random.default_rng(7)
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    if kind == "smooth":
        base = 0.5 + 0.4 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 9.0)[..., None] * np.array([1.0, 0.8, 0.6])
    else:
        base = 0.7 + 0.01 * rng.standard_normal((size, size, 3))
    image = base.astype(np.float32)[None]
    target = (base + 0.02 * rng.standard_normal((size, size, 3))).astype(np.float32)[None]
    return image, target
