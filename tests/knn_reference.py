"""The definition of sixdgs_knn_mean_dist2 (include/sixdgs.h) restated three ways, the clouds it is tested on, and the bounds the
tests use.

    d2(i, j)   = (dx dx + dy dy) + dz dz in fp32, dx = x_j - x_i ..., i != j by index
    mean_d2[i] = ((b0 + b1) + b2) / 3.0f, b0 <= b1 <= b2 the three smallest d2(i, .)

brute_np is that text in numpy fp32 (numpy never contracts), brute_f64 the same in double, brute_torch the same as separate elementwise
torch ops plus topk (each op is its own kernel, so nothing can be fused into a multiply-add); its final division is done by numpy on
the host, so that it does not depend on how a device divides.

BOUNDS (u = 2^-24, the unit roundoff of fp32; coordinates are exact fp32 numbers in every restatement):
  * d2: dx carries one rounding, dx dx that one twice plus its own -> (1 + u)^3; the two additions of non-negative terms add one
    rounding each -> d2_fp32 = d2 (1 + e), |e| <= (1 + u)^5 - 1.  The k-th smallest of values each perturbed by at most a relative e
    is within e of the k-th smallest of the exact values, so the same holds for b0, b1, b2 although fp32 and fp64 may pick different
    points.  The two additions and the division add three roundings: |mean_fp32 - mean| <= ((1 + u)^8 - 1) mean < 9 u mean.
    REL_MEAN = 9 u.  (Underflow does not occur on the clouds below; zeros are exact.)
  * scale = log(sqrt(max(d2, floor))) against fp64 0.5 log(max(d2, floor)) of the SAME fp32 d2: sqrt is correctly rounded, a relative
    u / 2 ... u, which moves the logarithm by at most u absolutely (log(1 + u) <= u); the logarithm itself is within LOG_ULPS = 2 ulp
    of its result (the documented bound of the device's logf is 1 ulp with full range, glibc's and SLEEF's below 1; 2 leaves room for
    either) and the result rounded to fp32 adds half an ulp of it:  |scale - ref| <= u + 2.5 * 2^-23 |ref| + 2^-149.
"""
import functools

import numpy as np

F = np.float32
U = 2.0 ** -24
REL_MEAN = 9 * U
LOG_ULPS = 2.0


def scale_bound(ref):
    return U + (LOG_ULPS + 0.5) * 2.0 ** -23 * np.abs(ref) + 2.0 ** -149


def brute_np(p, chunk=256):
    p = np.ascontiguousarray(p, F)
    n = p.shape[0]
    out = np.empty(n, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        dx, dy, dz = x[None, :] - x[a:b, None], y[None, :] - y[a:b, None], z[None, :] - z[a:b, None]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F
        d2[np.arange(b - a), np.arange(a, b)] = np.inf
        best = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
        out[a:b] = ((best[:, 0] + best[:, 1]) + best[:, 2]) / F(3.0)
    return out


def brute_f64(p, chunk=256):
    p = np.ascontiguousarray(p, F).astype(np.float64)
    n = p.shape[0]
    out = np.empty(n, np.float64)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        d = p[None, :, :] - p[a:b, None, :]
        d2 = (d * d).sum(-1)
        d2[np.arange(b - a), np.arange(a, b)] = np.inf
        out[a:b] = np.partition(d2, 2, axis=1)[:, :3].sum(-1) / 3.0
    return out


def brute_torch(p, chunk=512):
    """p: float32 [n,3] tensor on any device -> numpy float32 [n]."""
    import torch

    n = p.shape[0]
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    sums = torch.empty(n, dtype=torch.float32, device=p.device)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=p.device)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        dx = torch.sub(x[None, :], x[a:b, None])
        dy = torch.sub(y[None, :], y[a:b, None])
        dz = torch.sub(z[None, :], z[a:b, None])
        xx = torch.mul(dx, dx)
        yy = torch.mul(dy, dy)
        zz = torch.mul(dz, dz)
        d2 = torch.add(torch.add(xx, yy), zz)
        rows = torch.arange(b - a, device=p.device)
        d2[rows, rows + a] = inf
        best = torch.topk(d2, 3, dim=1, largest=False, sorted=True).values
        sums[a:b] = torch.add(torch.add(best[:, 0], best[:, 1]), best[:, 2])
    return sums.cpu().numpy() / F(3.0)


# ---- the clouds ---------------------------------------------------------------------------------------------------------------
def uniform(n, seed=0):
    return np.random.default_rng(1000 + seed + n).random((n, 3)).astype(F)


def clustered(n, seed=0):
    """Two Gaussian clusters of very different spread, one lone far outlier and a far pair 1e-3 apart (whose third neighbour lies in
    another cluster), in a shuffled order."""
    rng = np.random.default_rng(2000 + seed)
    wide = n // 2
    tight = n - 3 - wide
    p = np.concatenate([rng.normal(0.0, 1.0, (wide, 3)), rng.normal(0.0, 0.01, (tight, 3)) + (50.0, 0.0, 0.0),
                        [[1e3, 1e3, 1e3]], [[-500.0, -500.0, -500.0]], [[-500.0 + 1e-3, -500.0, -500.0]]]).astype(F)
    return p[rng.permutation(n)]


def plane(n=3001):
    p = uniform(n, 1)
    p[:, 2] = F(0.25)
    return p


def line(n=3000):
    t = np.random.default_rng(3).random(n).astype(F)
    return np.stack([t, F(2) * t, F(3) * t], axis=1).astype(F)


def lattice(side=12):
    g = np.arange(side, dtype=F)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return p[np.random.default_rng(4).permutation(p.shape[0])]


def duplicated(points=300, times=5):
    p = np.repeat(uniform(points, 5), times, axis=0)
    return p[np.random.default_rng(5).permutation(p.shape[0])]


def identical(n):
    return np.tile(np.array([[0.3, -1.7, 2.5]], F), (n, 1))


def offset(n=3000):
    return (uniform(n, 6) + F(4096.0)).astype(F)


def anisotropic(n=3000):
    return (uniform(n, 7) * np.array([1e4, 1.0, 1.0], F)).astype(F)


def sizes(box):
    s = [4, 5, 63, 64, 65, box - 1, box, box + 1, 2 * box + 1, 1023, 1024, 1025, 8193]
    if box != 256:
        s += [255, 256, 257, 513]
    return sorted(set(s))


def cases(box=256):
    """name -> a function making the cloud; every one has n <= 8193."""
    c = {f"uniform{n}": functools.partial(uniform, n) for n in sizes(box)}
    c.update(clustered=functools.partial(clustered, 2997), plane=plane, line=line, lattice=lattice, duplicated=duplicated,
             identical600=functools.partial(identical, 600), identical8193=functools.partial(identical, 8193), offset=offset,
             anisotropic=anisotropic)
    return c


@functools.lru_cache(maxsize=None)
def case(name, box=256):
    """(points, brute_np(points)) of a case, computed once per process and marked read-only."""
    p = np.ascontiguousarray(cases(box)[name](), F)
    want = brute_np(p)
    p.setflags(write=False)
    want.setflags(write=False)
    return p, want


# ---- GaussianModel.create_from_pcd's arithmetic in double (scene/gaussian_model.py:189-228) ---------------------------------------
C0 = 0.28209479177387814


def from_points_f64(points, colors, d2, sh_degree=3, opacity=0.1, min_dist2=1e-7):
    n = points.shape[0]
    d2 = np.maximum(np.asarray(d2, F).astype(np.float64), np.float64(F(min_dist2)))
    return dict(xyz=np.asarray(points, F), f_dc=((np.asarray(colors, F).astype(np.float64) - 0.5) / C0).reshape(n, 1, 3),
                f_rest=np.zeros((n, (sh_degree + 1) ** 2 - 1, 3), F), scale=np.repeat(0.5 * np.log(d2)[:, None], 3, axis=1),
                rot=np.tile(np.array([[1, 0, 0, 0]], F), (n, 1)), opacity=np.full((n, 1), np.log(opacity / (1 - opacity))))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def check_from_points(scene, points, colors, d2, sh_degree=3):
    """The checks shared with the GPU test: everything exact but scale, which is held to knn_reference.scale_bound."""
    want = from_points_f64(points, colors, d2, sh_degree)
    n = points.shape[0]
    got = {k: getattr(scene, "_" + v).detach().cpu().numpy() for k, v in (("xyz", "xyz"), ("f_dc", "features_dc"), ("f_rest", "features_rest"),
                                                                        ("scale", "scaling"), ("rot", "rotation"), ("opacity", "opacity"))}
    assert all(a.dtype == F for a in got.values())
    assert got["xyz"].shape == (n, 3) and np.array_equal(_bits(got["xyz"]), _bits(points))
    assert got["rot"].shape == (n, 4) and np.array_equal(got["rot"], want["rot"])
    assert got["f_rest"].shape == want["f_rest"].shape and not got["f_rest"].any()
    assert scene.active_sh_degree == 0 and scene.max_sh_degree == sh_degree
    assert got["f_dc"].shape == (n, 1, 3) and got["opacity"].shape == (n, 1) and got["scale"].shape == (n, 3)
    # (rgb - 0.5) / C0 in IEEE fp32, the constant rounded to fp32 -- computed on the host, so the same bits for a scene on any device
    assert np.array_equal(_bits(got["f_dc"][:, 0, :]), _bits((np.asarray(colors, F) - F(0.5)) / F(C0)))
    assert np.all(got["opacity"] == got["opacity"][0]) and abs(float(got["opacity"][0, 0]) - want["opacity"][0, 0]) <= 4 * U * abs(want["opacity"][0, 0])
    assert np.all(got["scale"] == got["scale"][:, :1])
    err, bound = np.abs(got["scale"].astype(np.float64) - want["scale"]), scale_bound(want["scale"])
    print(f"scale: max |got - fp64| / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    return got, want
