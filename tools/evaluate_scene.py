"""Score a fitted scene on its held-out views and write the reference's results.json and per_view.json.

    python tools/evaluate_scene.py --ply point_cloud.ply --source <dataset directory> --out <directory> [--iteration 30000]
                                   [--images images] [--white_background] [--sh_degree 3] [--chunk 8] [--write-images DIR]
    python tools/evaluate_scene.py --standin --out <directory> [--gaussians 2000] [--views 4] [--size 64] [--perturb 0.05]

The scene PLY is rendered from the poses of the source's test views (datasets.load_data with eval on: COLMAP, Blender or Tanks and
Temples layouts) and compared with their images by evaluate_views(quantise=True): metrics.py's definition, both sides through the
8-bit rule of a saved PNG.  --standin takes a synthetic scene and rasterised views of it instead of files (--perturb: noise on the
colours of the evaluated copy).  Written to --out, in metrics.py's layout with values where its lines 92-110 put mis-bound names:

    results.json     {"ours_<iteration>": {"SSIM": mean, "PSNR": mean}}
    per_view.json    {"ours_<iteration>": {"SSIM": {"00000.png": value, ...}, "PSNR": {...}}}

LPIPS is absent: no VGG weights exist offline.  --write-images DIR saves the renders and the ground truth as PNG (renders/ and gt/,
render.py's names).  main(argv) returns the two dicts."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def standin_views(gaussians: int, views: int, size: int, seed: int, perturb: float = 0.0):
    """-> (the scene to evaluate, held-out CameraInfo views drawn by the rasteriser from the unperturbed scene)."""
    pkg, syn = importlib.import_module("6dgs_amd"), importlib.import_module("6dgs_amd.synthetic")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(gaussians, seed), device="cuda")
    held = pkg.render_views(scene, syn.make_cameras(views, seed + 200, width=size, height=size), renderer="raster")
    if perturb > 0.0:
        noise = torch.randn(scene._features_dc.shape, generator=torch.Generator().manual_seed(seed))
        scene._features_dc = scene._features_dc + (perturb * noise).to(scene._features_dc.device)
    return scene, held


def posed(cams):
    test = importlib.import_module("6dgs_amd.test")
    c2w, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in cams])
    images = [np.ascontiguousarray(np.asarray(c.image)[..., :3]) for c in cams]
    return images, torch.stack(c2w), torch.stack(Ks)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ply")
    ap.add_argument("--source")
    ap.add_argument("--images", default="images")
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--standin", action="store_true")
    ap.add_argument("--out", required=True)
    ap.add_argument("--iteration", type=int, default=30000)
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--write-images", dest="write_images")
    ap.add_argument("--gaussians", type=int, default=2000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--perturb", type=float, default=0.05)
    args = ap.parse_args(argv)
    if args.standin == bool(args.ply or args.source) or bool(args.ply) != bool(args.source):
        ap.error("give --ply and --source, or --standin")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_scene needs a GPU")
    pkg = importlib.import_module("6dgs_amd")
    if args.standin:
        scene, cams = standin_views(args.gaussians, args.views, args.size, args.seed, args.perturb)
        background = (1.0, 1.0, 1.0)
    else:
        datasets = importlib.import_module("6dgs_amd.datasets")
        scene = pkg.GaussianScene.load_ply(args.ply, args.sh_degree, device="cuda")
        info = datasets.load_data(datasets.dotdict(source_path=args.source, images=args.images, eval=True, white_background=args.white_background))
        cams = list(info.test_cameras)
        if not cams:
            raise SystemExit(f"{args.source} has no test views")
        background = (1.0, 1.0, 1.0) if args.white_background else (0.0, 0.0, 0.0)
    images, c2w, K = posed(cams)
    r = pkg.evaluate_views(scene, images, c2w, K, quantise=True, chunk=args.chunk, background=background, return_renders=bool(args.write_images))
    names = ["{0:05d}.png".format(i) for i in range(len(cams))]
    method = f"ours_{args.iteration}"
    results = {method: {"SSIM": float(r["mean_ssim"]), "PSNR": float(r["mean_psnr"])}}
    per_view = {method: {"SSIM": dict(zip(names, map(float, r["ssim"]))), "PSNR": dict(zip(names, map(float, r["psnr"])))}}
    os.makedirs(args.out, exist_ok=True)
    for name, d in (("results.json", results), ("per_view.json", per_view)):
        with open(os.path.join(args.out, name), "w") as fp:
            json.dump(d, fp, indent=True)
    if args.write_images:
        from PIL import Image
        renders = r["renders"].cpu().numpy()
        for sub, arrays in (("renders", renders), ("gt", images)):
            os.makedirs(os.path.join(args.write_images, sub), exist_ok=True)
            for name, a in zip(names, arrays):
                Image.fromarray(np.ascontiguousarray(a)).save(os.path.join(args.write_images, sub, name))
    print(f"{len(cams)} views, status {r['status']}:  SSIM {results[method]['SSIM']:.7f}  PSNR {results[method]['PSNR']:.7f}")
    return results, per_view


if __name__ == "__main__":
    main()
