"""Fit a perturbed stand-in scene back to views of the scene that rendered them, with both backends of fit.fit_scene.

    python tools/fit_standin.py [--gaussians 5000] [--size 112] [--views 8] [--steps 60] [--batch 1] [--rounds 3]
    python tools/fit_standin.py --densify [--keep 0.5] [--enlarge 1.5] [--from_iter 5] [--until_iter 15] [--interval 10] [--grad 5e-3]
    python tools/fit_standin.py --from-points 2000 [--from_iter 5] [--until_iter 15] [--interval 10] [--grad 5e-3]

A stand-in scene (synthetic.make_scene) renders `views` views with renderer="raster"; a copy is perturbed -- colours, opacity logits,
positions and log-scales by Gaussian noise of the given standard deviations -- and fitted to the views.  In one process the two arms
alternate `rounds` times after one warm-up call each, the arrangement of tools/time_refine.py: backend="torch" (autograd and
torch.optim.Adam around the kernels) and backend="fused" (one sixdgs_fit_scene call).  HIP events around the whole fit_scene call --
the target's preparation, the scene's copy and the final read included -- divided by the steps.  Prints ms per step, the loss
histories' largest difference, and the parameters' RMS distance from the rendering scene before and after; asserts nothing.

--densify: the stand-in with a share of its Gaussians removed and the rest enlarged (thinned) is fitted back to the views with and
without densification, on the fused backend and on the torch arm: the rounds, the number of Gaussians and the loss of the first and
last passes of each.

--from-points N: N of the stand-in's centres with their DC colours, as a sparse point cloud would give them, become a scene through
GaussianScene.from_points (isotropic scales from the 3-nearest-neighbour kernel, opacity 0.1, no higher SH) and are fitted to the views
with densify= on both backends: the loss of the first and last passes and the PSNR of the views before and after."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")

ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scale": "_scaling", "rot": "_rotation"}


def perturbed(pkg, scene, sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    out = pkg.GaussianScene(scene.max_sh_degree)
    for k, a in ATTR.items():
        t = getattr(scene, a).clone()
        if sizes.get(k, 0.0) > 0.0:
            t += (sizes[k] * torch.randn(t.shape, generator=gen)).to(t.device)
        setattr(out, a, t)
    return out


def thinned(pkg, scene, keep, enlarge, seed):
    """A random share `keep` of the scene's Gaussians, their scales multiplied by `enlarge`."""
    n = len(scene)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:max(int(keep * n), 1)].sort().values.to(scene._xyz.device)
    out = pkg.GaussianScene(scene.max_sh_degree)
    for k, a in ATTR.items():
        setattr(out, a, getattr(scene, a)[idx].clone() + (float(np.log(enlarge)) if k == "scale" else 0.0))
    return out


def densify_demo(pkg, fit, scene, images, c2w, K, args):
    thin = thinned(pkg, scene, args.keep, args.enlarge, args.seed)
    opts = dict(from_iter=args.from_iter, until_iter=args.until_iter, interval=args.interval, grad_threshold=args.grad)
    print(f"{len(scene)} Gaussians thinned to {len(thin)} (scales x {args.enlarge}), {args.views} views of {args.size} x {args.size}, {args.steps} steps; "
          f"densify {opts}, extent {fit.cameras_extent(c2w):.3f}")
    tail = max(min(args.views // args.batch, args.steps), 1)
    for name, kw in (("fixed n, fused", dict(backend="fused")), ("densify, fused", dict(backend="fused", densify=opts)),
                     ("densify, torch", dict(backend="torch", densify=opts))):
        new, rep = fit.fit_scene(thin, images, c2w, K, steps=args.steps, batch=args.batch, **kw)
        h = rep["loss_history"]
        rounds = rep["rounds"].tolist() if "rounds" in rep else []
        print(f"{name}: n {len(thin)} -> {len(new)}; loss, mean of the first {tail} steps {float(h[:tail].mean()):.5f}, of the last {tail} "
              f"{float(h[-tail:].mean()):.5f}; status {int(rep['status'])}; rounds (iteration, n, clones, splits, pruned, n after): {rounds}")


def psnr(pkg, scene, images, c2w, K):
    """Mean PSNR of the scene's rasterised views against the images: evaluate_views' metrics.py definition, nothing read back but the
    per-view numbers."""
    return float(pkg.evaluate_views(scene, images, c2w, K)["mean_psnr"])


def from_points_demo(pkg, fit, scene, held, images, c2w, K, args):
    n = min(args.from_points, len(scene))
    idx = torch.randperm(len(scene), generator=torch.Generator().manual_seed(args.seed))[:n].sort().values.to(scene._xyz.device)
    colors = (scene._features_dc[idx, 0, :] * 0.28209479177387814 + 0.5).clamp(0.0, 1.0)
    start = pkg.GaussianScene.from_points(scene._xyz[idx], colors, scene.max_sh_degree)
    opts = dict(from_iter=args.from_iter, until_iter=args.until_iter, interval=args.interval, grad_threshold=args.grad)
    sigma = torch.exp(start._scaling[:, 0])
    print(f"{n} of {len(scene)} centres -> from_points: scale quantiles 10 / 50 / 90 % {', '.join(f'{float(q):.4f}' for q in sigma.quantile(torch.tensor([0.1, 0.5, 0.9], device=sigma.device)))}; "
          f"{args.views} views of {args.size} x {args.size}, {args.steps} steps; densify {opts}; PSNR before {psnr(pkg, start, images, c2w, K):.2f} dB")
    tail = max(min(args.views // args.batch, args.steps), 1)
    for backend in ("fused", "torch"):
        new, rep = fit.fit_scene(start, images, c2w, K, steps=args.steps, batch=args.batch, backend=backend, densify=opts, sh_degree_start=0)
        h = rep["loss_history"]
        print(f"{backend}: n {len(start)} -> {len(new)}; loss, mean of the first {tail} steps {float(h[:tail].mean()):.5f}, of the last {tail} "
              f"{float(h[-tail:].mean()):.5f}; PSNR after {psnr(pkg, new, images, c2w, K):.2f} dB; status {int(rep['status'])}; rounds {rep['rounds'].tolist()}")


def rms(a, b):
    return {k: float((getattr(a, attr) - getattr(b, attr)).pow(2).mean().sqrt()) for k, attr in ATTR.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--colour", type=float, default=0.05, help="noise on f_dc")
    ap.add_argument("--opacity", type=float, default=0.5, help="noise on the opacity logits")
    ap.add_argument("--position", type=float, default=0.002, help="noise on xyz")
    ap.add_argument("--log_scale", type=float, default=0.05, help="noise on the log-scales")
    ap.add_argument("--densify", action="store_true", help="fit a thinned copy back, with and without densification")
    ap.add_argument("--from-points", dest="from_points", type=int, default=0, help="start from this many of the stand-in's centres (from_points)")
    ap.add_argument("--keep", type=float, default=0.5, help="--densify: the share of the Gaussians kept")
    ap.add_argument("--enlarge", type=float, default=1.5, help="--densify: the factor on the kept Gaussians' scales")
    ap.add_argument("--from_iter", type=int, default=5)
    ap.add_argument("--until_iter", type=int, default=15)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--grad", type=float, default=5e-3, help="--densify: grad_threshold")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_standin needs a GPU")
    import train_standin as ts
    pkg, _, _, test = ts.modules()
    fit = importlib.import_module("6dgs_amd.fit")
    scene, _, held = ts.build_standin(args.gaussians, args.seed, 2, args.views, args.size, renderer="raster")
    c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in held])
    c2w, K, images = torch.stack(c2w), torch.stack(Ks), [c.image for c in held]
    if args.densify:
        return densify_demo(pkg, fit, scene, images, c2w, K, args)
    if args.from_points:
        return from_points_demo(pkg, fit, scene, held, images, c2w, K, args)
    start = perturbed(pkg, scene, {"f_dc": args.colour, "opacity": args.opacity, "xyz": args.position, "scale": args.log_scale}, args.seed)
    print(f"{args.gaussians} Gaussians, {args.views} views of {args.size} x {args.size}, {args.steps} steps of {args.batch}, {args.rounds} rounds")
    ms, out = {"torch": [], "fused": []}, {}
    for rnd in range(args.rounds + 1):                    # round 0 warms both arms up
        for backend in ("torch", "fused"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            out[backend] = fit.fit_scene(start, images, c2w, K, steps=args.steps, batch=args.batch, backend=backend)
            b.record()
            torch.cuda.synchronize()
            if rnd:
                ms[backend].append(a.elapsed_time(b) / args.steps)
    for backend, v in ms.items():
        print(f"{backend}: ms per step, each round: {', '.join(f'{x:.3f}' for x in v)}; median {np.median(v):.3f}, min {min(v):.3f}, max {max(v):.3f}")
    print(f"fused / torch (medians): {np.median(ms['fused']) / np.median(ms['torch']):.3f}")
    (st, rt), (sf, rf) = out["torch"], out["fused"]
    tail = min(3 * args.views // args.batch, args.steps)
    print(f"first loss torch {float(rt['loss_history'][0].mean()):.5f} (equal bits: {torch.equal(rt['loss_history'][0], rf['loss_history'][0])}); "
          f"mean of the last {tail} steps torch {float(rt['loss_history'][-tail:].mean()):.5f}, fused {float(rf['loss_history'][-tail:].mean()):.5f}; "
          f"max |history difference| {float((rt['loss_history'] - rf['loss_history']).abs().max()):.3e}; status {int(rf['status'])}")
    before, after_t, after_f = rms(start, scene), rms(st, scene), rms(sf, scene)
    for k in ATTR:
        print(f"  rms distance from the rendering scene, {k:8s}: before {before[k]:.3e}, after torch {after_t[k]:.3e}, fused {after_f[k]:.3e}")


if __name__ == "__main__":
    main()
