"""Contribution-based pruning and importance sampling on a stand-in scene with a trained scorer: what share of the Gaussians the training
views never use, whether the scene renders to the same bytes without them, and what either does to the estimator.

    python tools/contrib_standin.py [--gaussians 5000] [--iterations 1500] [--size 224] [--keep-fraction 0.5] [--renderer disc|raster]

Scene, views and training are tools/train_standin.py's (make_scene, 50 training and 16 held-out views rendered by render_views,
train_id_module(batched_window=True) on the full scene).  The contributions are measured on the training cameras
(ops.scene_contrib_raw), and the inert share also on the first 1, 2, 4 ... of them.  Then, on the trained weights, test_pose_estimation
over the training and the held-out views with rays emitted from: the full scene and the scene without its inert Gaussians, each uniformly
(the reference's randperm of 1000 ellipsoids) and with importance = weight; the heaviest --keep-fraction uniformly; every valid Gaussian
of the full scene, of the scene without its inert ones and of its heaviest --keep-fraction.
Per variant: rays, wall time per pose (the whole of test_pose_estimation after a warm-up, divided by the views), median errors.
Prints markdown; a number that was not measured is not written."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")
import train_standin as TS  # noqa: E402


def scene_arrays(s):
    return (s._xyz, s._scaling, s._rotation, s._opacity, s._features_dc, s._features_rest, int(s.active_sh_degree))


def timed_errors(idm, cams, rays, up):
    """pose_errors after a warm-up on two views -> (translation, rotation, unusable, seconds per view)."""
    TS.pose_errors(idm, cams[:2], rays, up)
    torch.cuda.synchronize()
    t0 = time.time()
    t, r, bad = TS.pose_errors(idm, cams, rays, up)
    torch.cuda.synchronize()
    return t, r, bad, (time.time() - t0) / len(cams)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--train-views", type=int, default=50)
    ap.add_argument("--held-views", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--keep-fraction", type=float, default=0.5)
    ap.add_argument("--renderer", choices=["disc", "raster"], default="disc", help="what renders the query images (tools/train_standin.py's default: disc)")
    ap.add_argument("--ckpt", default="id_module.th", help="where the trained checkpoint is written (default: the current directory)")
    args = ap.parse_args()
    pkg, _, ops, _ = TS.modules()
    render = importlib.import_module("6dgs_amd.render")
    contribution = importlib.import_module("6dgs_amd.contribution")
    torch.manual_seed(0)
    scene, train_cams, held_cams = TS.build_standin(args.gaussians, args.seed, args.train_views, args.held_views, args.size, renderer=args.renderer)
    n, size = len(scene), args.size
    rows = torch.from_numpy(render.camera_rows(train_cams)).cuda()
    held_rows = torch.from_numpy(render.camera_rows(held_cams)).cuda()
    torch.cuda.synchronize()
    t0 = time.time()
    raw = ops.scene_contrib_raw(*scene_arrays(scene), rows, size, size, chunk=8)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    contrib = {k: raw[k] for k, _ in ops.CONTRIB}
    inert = (contrib["pixels"] == 0) & (contrib["stops"] == 0)
    pruned, keep = pkg.prune_by_contribution(scene, contrib, drop_inert=True)
    heavy, keep_heavy = pkg.prune_by_contribution(scene, contrib, drop_inert=True, keep_fraction=args.keep_fraction)
    L = ["## Stand-in scene: pruning and importance sampling", "",
         "Command: `" + " ".join(["python tools/contrib_standin.py"] + sys.argv[1:]) + "`", "",
         f"`make_scene({args.gaussians}, {args.seed})`, {args.train_views} training and {args.held_views} held-out views of {size} x {size} rendered by "
         f"`render_views(renderer={args.renderer!r})`; contributions over the training cameras, `chunk=8`: {seconds * 1e3:.1f} ms wall for the whole call "
         f"({raw['instances_needed']} instances in the largest chunk).", "",
         f"* inert for the training views (no pixel added it, it stopped none): **{int(inert.sum())} of {n} ({100.0 * float(inert.float().mean()):.1f} %)**; "
         f"seen in no view but stopping pixels: {int(((contrib['pixels'] == 0) & (contrib['stops'] > 0)).sum())}",
         f"* views a Gaussian is seen in: median {int(contrib['seen'].median())}, max {int(contrib['seen'].max())} of {args.train_views}; "
         f"peak alpha T: median {float(contrib['peak'].median()):.3f}; share of the total weight carried by the heaviest tenth: "
         f"{float(contrib['weight'].sort(descending=True).values[:max(n // 10, 1)].sum() / contrib['weight'].sum()):.3f}"]
    shares = []
    for m in sorted({1, 2, 4, 8, 16, args.train_views}):
        if m <= args.train_views:
            part = ops.scene_contrib_raw(*scene_arrays(scene), rows[:m], size, size, chunk=8)
            shares.append(f"{m}: {100.0 * float(((part['pixels'] == 0) & (part['stops'] == 0)).float().mean()):.1f} %")
    L.append("* inert share against the number of training views measured (the first m): " + ", ".join(shares))
    # the exact end-to-end property, on the views measured and -- for comparison, not a guarantee -- on the held-out ones
    def renders(s, cams):
        return ops.raster_views(*scene_arrays(s), cams, size, size, channels=4, want_float=True)

    for name, cams in (("training", rows), ("held-out", held_rows)):
        (ff, fu), (pf, pu) = renders(scene, cams), renders(pruned, cams)
        same = torch.equal(ff, pf) and torch.equal(fu, pu)
        differing = int((fu != pu).any(dim=-1).sum())
        L.append(f"* renders of the scene without its inert Gaussians, {name} views: {'BYTE-EQUAL (float and uint8)' if same else f'{differing} pixels differ'}")
        if name == "training" and not same:
            raise SystemExit("the pruned scene's training views are not byte-equal")
    idm = TS.fresh_scorer().eval()
    up = TS.model_up_of(train_cams)
    t0 = time.time()
    TS.train(idm, scene, train_cams, held_cams, args.ckpt, args.iterations)
    torch.cuda.synchronize()
    L += ["", f"Scorer trained on the full scene as `tools/train_standin.py` does ({args.iterations} iterations, {time.time() - t0:.1f} s).  "
          "Errors: median over the views, translation of the camera centre in scene units / rotation in degrees; time: wall seconds of "
          "`test_pose_estimation` per view.", "",
          "| emitting Gaussians | selection | ellipsoids | rays | s / pose | train t / r | held t / r | unusable |", "|---|---|---|---|---|---|---|---|"]
    w = contrib["weight"]
    variants = [("full scene", "uniform, 1000", scene, dict()),
                ("full scene", "importance = weight, 1000", scene, dict(importance=w)),
                ("without inert", "uniform, 1000", pruned, dict()),
                ("without inert", "importance = weight, 1000", pruned, dict(importance=w[keep])),
                (f"heaviest {args.keep_fraction:g} by weight", "uniform, 1000", heavy, dict()),
                ("full scene", "every valid Gaussian", scene, dict(max_ellipsoids=-1)),
                ("without inert", "every valid Gaussian", pruned, dict(max_ellipsoids=-1)),
                (f"heaviest {args.keep_fraction:g} by weight", "every valid Gaussian", heavy, dict(max_ellipsoids=-1))]
    for where, how, s, kw in variants:
        torch.manual_seed(1)
        ori, dr, rgb, src = pkg.generate_all_possible_rays(s, return_src=True, **kw)
        rays = (ori, dr, rgb)
        tt, tr, tb, sec_t = timed_errors(idm, list(train_cams), rays, up)
        ht, hr, hb, sec_h = timed_errors(idm, list(held_cams), rays, up)
        sec = (sec_t * len(train_cams) + sec_h * len(held_cams)) / (len(train_cams) + len(held_cams))
        L.append(f"| {where} ({len(s)}) | {how} | {int(torch.unique(src).numel())} | {ori.shape[0]} | {sec:.4f} | {TS._med(tt):.3f} / {TS._med(tr):.1f} | "
                 f"{TS._med(ht):.3f} / {TS._med(hr):.1f} | {int(tb.sum() + hb.sum())} |")
    L.append("")
    print("\n".join(L))


if __name__ == "__main__":
    main()
