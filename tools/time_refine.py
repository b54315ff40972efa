"""Time refine.refine_poses' two backends against each other on a stand-in scene.

    python tools/time_refine.py [--gaussians 5000] [--size 224] [--views 8] [--downscale 2] [--steps 50] [--rounds 3]
                                [--levels 8:30:4e-3,4:30:2e-3,2:40:1e-3]

In one process the two arms alternate `rounds` times after one warm-up call each: backend="torch" (autograd and torch.optim.Adam around the
kernels) and backend="fused" (one sixdgs_refine_poses call).  HIP events around the whole refine_poses call -- the target's
preparation, the host inversions and the final read included -- divided by the steps + 1 evaluations.  tools/refine_standin.py's
step_split on the same views puts the three kernel parts beside them.  Prints the medians and the spread; asserts nothing.
--levels times a coarse-to-fine schedule instead: every level alone as a one-level schedule, then the whole schedule, the two arms
alternating as above (the torch arm of a schedule is autograd around the kernels with ops.pose_step for the camera); the divisor is the
number of evaluations (each level's steps + 1, plus the input's)."""
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


def time_levels(args, refine, scene, images, start, K):
    levels = refine.parse_levels(args.levels)
    print(f"{args.gaussians} Gaussians, {args.views} views of {args.size} x {args.size}, levels {args.levels}, {args.rounds} rounds")
    for name, plan in [(f"level {lv[0]}:{lv[1]}:{lv[2]:g} alone", [lv]) for lv in levels] + [("the whole schedule", levels)]:
        evaluations = sum(lv[1] + 1 for lv in plan) + 1
        ms = {"torch": [], "fused": []}
        out = {}
        for rnd in range(args.rounds + 1):                # round 0 warms both arms up
            for backend in ("torch", "fused"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                out[backend] = refine.refine_poses(scene, images, start, K, levels=plan, backend=backend)
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    ms[backend].append(a.elapsed_time(b) / evaluations)
        geo = out["fused"]["levels"]
        print(f"{name} ({', '.join(str(g['width']) + ' x ' + str(g['height']) for g in geo)}; {evaluations} evaluations): ms per evaluation "
              + "; ".join(f"{b} median {np.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})" for b, v in ms.items())
              + f"; fused / torch {np.median(ms['fused']) / np.median(ms['torch']):.3f}; loss_input equal bits "
              f"{torch.equal(out['torch']['loss_input'], out['fused']['loss_input'])}; kept torch {int(out['torch']['kept_input'].sum())}, "
              f"fused {int(out['fused']['kept_input'].sum())}; status {out['fused']['status'].tolist()}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--levels", default=None, help="time this coarse-to-fine schedule (downscale:steps:lr per level, comma separated)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_refine needs a GPU")
    import refine_standin as rs
    import train_standin as ts
    pkg, syn, ops, test = ts.modules()
    refine, autograd = importlib.import_module("6dgs_amd.refine"), importlib.import_module("6dgs_amd.autograd")
    scene, _, held = ts.build_standin(args.gaussians, args.seed, 2, args.views, args.size, renderer="raster")
    gt, Ks = zip(*[test.gt_pose_and_intrinsics(c, "cpu") for c in held])
    K = torch.stack(Ks)
    images = [c.image for c in held]
    rows = torch.from_numpy(importlib.import_module("6dgs_amd.render").camera_rows(held))
    off = torch.tensor([[o * (1 if v % 2 == 0 else -1) for o in rs.OFFSET] for v in range(args.views)], dtype=torch.float32)
    w2c = torch.eye(4).repeat(args.views, 1, 1)
    w2c[:, :3, :] = refine.compose(rows, off)[:, :12].reshape(-1, 3, 4)
    start = torch.linalg.inv(w2c)
    if args.levels:
        time_levels(args, refine, scene, images, start, K)
        return
    print(f"{args.gaussians} Gaussians, {args.views} views of {args.size} x {args.size}, downscale {args.downscale}, {args.steps} steps, {args.rounds} rounds")
    ms = {"torch": [], "fused": []}
    out = {}
    for rnd in range(args.rounds + 1):                    # round 0 warms both arms up
        for backend in ("torch", "fused"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            out[backend] = refine.refine_poses(scene, images, start, K, steps=args.steps, downscale=args.downscale, backend=backend)
            b.record()
            torch.cuda.synchronize()
            if rnd:
                ms[backend].append(a.elapsed_time(b) / (args.steps + 1))
    for backend, v in ms.items():
        print(f"{backend}: ms per step, each round: {', '.join(f'{x:.3f}' for x in v)}; median {np.median(v):.3f}, min {min(v):.3f}, max {max(v):.3f}")
    print(f"fused / torch (medians): {np.median(ms['fused']) / np.median(ms['torch']):.3f}")
    t, f = out["torch"], out["fused"]
    print(f"loss start {t['loss_start'].median():.5f} (equal bits: {torch.equal(t['loss_start'], f['loss_start'])}); best torch {t['loss_best'].median():.5f}, "
          f"fused {f['loss_best'].median():.5f}; max |history difference| {float((t['loss_history'] - f['loss_history']).abs().max()):.3e}; "
          f"status {f['status'].tolist()}")
    rs.step_split(refine, autograd, ops, scene, images, start, K, args.downscale)


if __name__ == "__main__":
    main()
