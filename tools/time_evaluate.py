"""Time the held-out-view metrics: the kernel beside the photometric loss it shares its blurs with, evaluate_views beside rendering and
comparing on the host, and what evaluate= adds to a fused fit.

    python tools/time_evaluate.py [--sizes 200 800] [--views 1 4 32] [--gaussians 500000] [--repeats 5] [--inner 20] [--parts a b c]

  a  ops.image_metrics (quantise off, on, on with the render's bytes) beside ops.photometric_loss without a gradient, on the same
     rasterised fp32 image [V,S,S,4] and uint8 target: the same bytes read, the same blurs.
  b  evaluate_views(quantise=True) beside the way before it: render_views(renderer="raster"), every view read back, PSNR formed in
     numpy from the bytes (the arithmetic tools/fit_standin.py had).  The images are given on the host, as a dataset holds them, and
     once more as GPU tensors.  Windows of --inner-b calls.
  c  fit_scene(backend="fused") on 5000 Gaussians, 8 views of 112 x 112, 60 steps, with and without evaluate= at steps 0, 30 and 60 on
     4 held-out views, and those three evaluations alone.  One call per window.
HIP events around back-to-back calls, the variants' windows alternating in one process, after a warm-up; the median of `repeats`
windows, with their minimum and maximum."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def windows(variants, repeats, inner, warm=2):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def show(r, views=None):
    for k, (med, lo, hi) in r.items():
        per = f", {med / views:8.3f} per view" if views else ""
        print(f"  {k:28s} {med:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}){per}")


def host_psnr(render, scene, held):
    """The way before evaluate_views: every rendered view read back, PSNR in numpy from the bytes."""
    out = render.render_views(scene, held, renderer="raster")
    diff = [(np.asarray(a.image[..., :3], np.float64) - np.asarray(b.image[..., :3], np.float64)) / 255.0 for a, b in zip(out, held)]
    mse = [float((d * d).mean()) for d in diff]
    return float(np.mean([10.0 * np.log10(1.0 / max(m, 1e-12)) for m in mse]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 800])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inner-b", dest="inner_b", type=int, default=3)
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c"])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_evaluate needs a GPU")
    pkg, syn, ops = importlib.import_module("6dgs_amd"), importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")
    render, test = importlib.import_module("6dgs_amd.render"), importlib.import_module("6dgs_amd.test")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(args.gaussians, 0), device="cuda")
    arrays = [scene._xyz, scene._scaling, scene._rotation, scene._opacity, scene._features_dc, scene._features_rest]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for size in args.sizes:
        for views in args.views:
            if not {"a", "b"} & set(args.parts):
                continue
            held = render.render_views(scene, syn.make_cameras(views, 21, width=size, height=size), renderer="raster")
            print(f"{size} x {size}, {views} view(s), {args.gaussians} Gaussians")
            if "a" in args.parts:
                cams = torch.from_numpy(render.camera_rows(held)).cuda()
                image = torch.cat([ops.raster_views(*arrays, 3, cams[v:v + 1].contiguous(), size, size, want_float=True, want_u8=False)
                                   for v in range(views)])
                target = (image[..., :3] * 255 + 8 * torch.randn(image[..., :3].shape, device="cuda", generator=gen)).clamp(0, 255).to(torch.uint8).contiguous()
                ws = torch.empty(max(ops.photometric_loss_workspace_bytes(views, size, size), ops.image_metrics_workspace_bytes(views, size, size)),
                                 dtype=torch.uint8, device="cuda")
                r = windows({"photometric_loss, no gradient": lambda: ops.photometric_loss(image, target, workspace=ws),
                             "image_metrics, clamp": lambda: ops.image_metrics(image, target, quantise=False, workspace=ws),
                             "image_metrics, 8 bit": lambda: ops.image_metrics(image, target, quantise=True, workspace=ws),
                             "image_metrics, 8 bit + render": lambda: ops.image_metrics(image, target, quantise=True, want_render=True, workspace=ws)},
                            args.repeats, args.inner)
                show(r, views)
                base = r["photometric_loss, no gradient"][0]
                print("  image_metrics / photometric_loss: " + ", ".join(f"{k.split(', ', 1)[1]} {v[0] / base:.3f}" for k, v in r.items() if k.startswith("image")))
                del image, target
            if "b" in args.parts:
                c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in held])
                c2w, K = torch.stack(c2w), torch.stack(Ks)
                host_images = [np.ascontiguousarray(c.image[..., :3]) for c in held]
                gpu_images = [torch.from_numpy(im).cuda() for im in host_images]
                new = pkg.evaluate_views(scene, host_images, c2w, K)
                print(f"  mean PSNR: evaluate_views {float(new['mean_psnr']):.4f} dB, on the host from image_u8 {host_psnr(render, scene, held):.4f} dB")
                r = windows({"render_views + host PSNR": lambda: host_psnr(render, scene, held),
                             "evaluate_views, host images": lambda: pkg.evaluate_views(scene, host_images, c2w, K),
                             "evaluate_views, GPU images": lambda: pkg.evaluate_views(scene, gpu_images, c2w, K)}, args.repeats, args.inner_b, warm=1)
                show(r, views)
                old = r["render_views + host PSNR"]
                for k in ("evaluate_views, host images", "evaluate_views, GPU images"):
                    print(f"  {k} / the host's way: {r[k][0] / old[0]:.3f} (faster beyond the spread: {r[k][2] < old[1]})")
            del held
    if "c" in args.parts:
        small = pkg.GaussianScene.from_dict(syn.make_scene(5000, 11), device="cuda")
        cams = render.render_views(small, syn.make_cameras(12, 211, width=112, height=112), renderer="raster")
        c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in cams])
        c2w, K, images = torch.stack(c2w), torch.stack(Ks), [c.image for c in cams]
        start = pkg.GaussianScene(small.max_sh_degree)
        noise = torch.Generator().manual_seed(11)
        for a in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
            t = getattr(small, a).clone()
            setattr(start, a, t + (0.05 * torch.randn(t.shape, generator=noise)).cuda() if a == "_features_dc" else t)
        held = dict(images=images[8:], c2w=c2w[8:], intrinsics=K[8:], at=(0, 30, 60))
        fit = lambda **kw: pkg.fit_scene(start, images[:8], c2w[:8], K[:8], steps=60, backend="fused", **kw)      # noqa: E731
        print("fused fit: 5000 Gaussians, 8 views of 112 x 112, 60 steps; evaluate= at 0, 30, 60 on 4 held-out views")
        r = windows({"fit": fit, "fit with evaluate=": lambda: fit(evaluate=held),
                     "three evaluate_views calls": lambda: [pkg.evaluate_views(start, held["images"], held["c2w"], held["intrinsics"], quantise=False)
                                                            for _ in range(3)]}, args.repeats, 1, warm=1)
        show(r)
        extra = r["fit with evaluate="][0] - r["fit"][0]
        print(f"  evaluate= adds {extra:.3f} ms: the evaluations' own {r['three evaluate_views calls'][0]:.3f} ms, the segment cuts and their reads "
              f"{extra - r['three evaluate_views calls'][0]:.3f} ms")
        print("  evaluations:", fit(evaluate=held)[1]["evaluations"])


if __name__ == "__main__":
    main()
