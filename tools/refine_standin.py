"""Measure pose refinement (6dgs_amd/refine.py) on a stand-in scene.

    python tools/refine_standin.py [--gaussians 5000] [--size 224] [--views 8] [--steps 100] [--downscale 2] [--iterations 600] [--backend torch|fused]
                                   [--levels 8:30:4e-3,4:30:2e-3,2:40:1e-3]

Builds synthetic.make_scene, renders held-out views with renderer="raster" (so the query images are the scene's own renderer's), and
refines from two kinds of start:
  perturbed   the true camera moved by tools/raster_fit.py's offset (about 0.054 scene units and 1.5 degrees, signs alternating over the
              views) and by 2 x and 4 x that offset
  estimator   the poses test_pose_estimation gives on a scorer trained on rendered views of the same scene (tools/train_standin.py's
              functions, `iterations` iterations; 0 skips this part)
Reports per kind the centre and rotation error before and after (median and how many views improved), the loss before and after, and
the milliseconds of a refinement step split into raster forward, loss, raster backward and the rest (HIP events around each part
of a hand-written step on the same views; the rest is compose, its autograd, Adam and the host in between).
--backend fused runs every refinement as one library call (refine_poses(..., backend="fused")); the split is of the torch step either way.
--levels runs every start a second time with that coarse-to-fine schedule (downscale:steps:lr per level) and prints the two arms one
under the other, with how many views kept their input pose.
Nothing is asserted: what comes out is reported, a negative result included."""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")

OFFSET = (0.03, -0.02, 0.04, 0.02, -0.015, 0.01)


def summarise(name, refine, gt, start, out):
    t0, a0 = refine.pose_errors(gt, start)
    t1, a1 = refine.pose_errors(gt, out["c2w"])
    better = int(((t1 < t0) & (a1 < a0)).sum())
    print(f"{name}: {len(t0)} views; centre error median {float(t0.nanmedian()):.4f} -> {float(t1.nanmedian()):.4f} (max {float(t0.max()):.4f} -> "
          f"{float(t1.max()):.4f}), rotation error median {float(a0.nanmedian()):.3f} -> {float(a1.nanmedian()):.3f} deg (max {float(a0.max()):.3f} -> "
          f"{float(a1.max()):.3f}); both errors fell on {better} views; loss median {float(out['loss_start'].median()):.5f} -> "
          f"{float(out['loss_best'].median()):.5f}; best step median {int(out['best_step'].median())}"
          + (f"; kept the input on {int(out['kept_input'].sum())} views" if "kept_input" in out else ""), flush=True)


def step_split(refine, autograd, ops, scene, images, start, K, downscale, repeats=20):
    """ms of one refinement step's parts on these views, median over `repeats` steps after 3 warm-up steps."""
    tensors, sh_degree = refine._scene_tensors(scene)
    dev = tensors[0].device
    target, ox, oy = refine.prepare_target(refine._stack_images(images, dev), downscale)
    views, height, width = target.shape[0], int(target.shape[1]), int(target.shape[2])
    rows0 = torch.cat([torch.linalg.inv(start.cpu())[:, :3, :].reshape(views, 12), refine.scaled_intrinsics(K.cpu(), downscale, ox, oy)], 1).to(dev)
    delta = torch.zeros(views, 6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([delta], lr=2e-3)
    parts = []
    for it in range(repeats + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        rows = refine.compose(rows0, delta)
        ev[1].record()
        image, state = ops.raster_views(*tensors, sh_degree, rows, width, height, want_float=True, want_u8=False, want_state=True)
        ev[2].record()
        loss, grad = ops.photometric_loss(image, target, want_grad=True)
        ev[3].record()
        d_cams = ops.raster_views_backward(*tensors, sh_degree, rows, width, height, grad, state, want=("cams",))[6]
        ev[4].record()
        opt.zero_grad()
        rows.backward(d_cams)
        opt.step()
        ev[5].record()
        torch.cuda.synchronize()
        if it >= 3:
            parts.append([ev[i].elapsed_time(ev[i + 1]) for i in range(5)])
    m = np.median(np.asarray(parts), axis=0)
    print(f"one step on {views} views at {width} x {height}: raster forward {m[1]:.3f} ms, loss (forward + gradient) {m[2]:.3f}, raster backward "
          f"(cams) {m[3]:.3f}, the rest {m[0] + m[4]:.3f} (compose {m[0]:.3f}; its backward and Adam {m[4]:.3f}); together {m.sum():.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=600, help="training iterations of the stand-in scorer (0: skip the estimator part)")
    ap.add_argument("--backend", choices=("torch", "fused"), default="torch", help="refine.refine_poses' backend")
    ap.add_argument("--levels", default=None, help="a second arm: a coarse-to-fine schedule, downscale:steps:lr per level, comma separated")
    ap.add_argument("--ckpt", default=os.path.join(tempfile.gettempdir(), "refine_standin_id_module.th"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_standin needs a GPU")
    import train_standin as ts
    pkg, syn, ops, test = ts.modules()
    refine, autograd = importlib.import_module("6dgs_amd.refine"), importlib.import_module("6dgs_amd.autograd")
    scene, train_cams, held = ts.build_standin(args.gaussians, args.seed, 50, args.views, args.size, renderer="raster")
    gt, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in held])
    gt, K = torch.stack(gt), torch.stack(Ks)
    images = [c.image for c in held]
    rows = torch.from_numpy(importlib.import_module("6dgs_amd.render").camera_rows(held))
    kw = dict(steps=args.steps, downscale=args.downscale, backend=args.backend)
    arms = [("one level", kw)]
    if args.levels:
        arms.append((f"levels {args.levels}", dict(levels=refine.parse_levels(args.levels), backend=args.backend)))
    print(f"{args.gaussians} Gaussians, {args.views} held-out {args.size} x {args.size} views (renderer raster), {args.steps} steps, downscale {args.downscale}, "
          f"backend {args.backend}")
    for name, mult in (("perturbed x 1", 1.0), ("perturbed x 2", 2.0), ("perturbed x 4", 4.0)):
        off = torch.tensor([[mult * o * (1 if v % 2 == 0 else -1) for o in OFFSET] for v in range(args.views)], dtype=torch.float32)
        w2c = torch.eye(4).repeat(args.views, 1, 1)
        w2c[:, :3, :] = refine.compose(rows, off)[:, :12].reshape(-1, 3, 4)
        start = torch.linalg.inv(w2c)
        for arm, arm_kw in arms:
            out = refine.refine_poses(scene, images, start, K, **arm_kw)
            summarise(f"{name}, {arm}", refine, gt, start, {k: v.cpu() for k, v in out.items() if torch.is_tensor(v)})
        if mult == 1.0:
            step_split(refine, autograd, ops, scene, images, start, K, args.downscale)
    if args.iterations > 0:
        idm = ts.fresh_scorer(0)
        rays = pkg.generate_all_possible_rays(scene)
        os.makedirs(os.path.dirname(os.path.abspath(args.ckpt)), exist_ok=True)
        ts.train(idm, scene, train_cams, held, args.ckpt, args.iterations)
        results, *_ = pkg.test_pose_estimation(list(held), idm, *rays, ts.model_up_of(train_cams), verbose=False)
        for arm, arm_kw in arms:
            refined = refine.refine_results(scene, list(held), [dict(r) for r in results], **arm_kw)
            done = [r for r in refined if "refined_c2w" in r]
            start = torch.tensor([r["pred_c2w"] for r in done])
            out = {"c2w": torch.tensor([r["refined_c2w"] for r in done]), "loss_start": torch.tensor([r["photometric_loss_before"] for r in done]),
                   "loss_best": torch.tensor([r["photometric_loss_after"] for r in done]), "best_step": torch.zeros(len(done), dtype=torch.int64)}
            summarise(f"estimator ({args.iterations} training iterations; best step not kept by refine_results), {arm}", refine,
                      torch.tensor([r["gt_c2w"] for r in done]), start, out)


if __name__ == "__main__":
    main()
