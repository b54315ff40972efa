"""Two short demonstrations of the rasteriser's gradients (autograd.raster_views): Adam on an L1 photometric loss against views
rendered from the true state of make_scene.

    python tools/raster_fit.py [--gaussians 20000] [--size 128] [--steps 200] [--views 4] [--loss l1|dssim]

  (a) pose      one camera perturbed by a small translation and rotation; a 6-vector (translation, axis-angle) composed onto the
                perturbed w2c row in torch is optimised, the scene is fixed.  Error: translation (scene units) and rotation (degrees)
                of the composed camera against the true one.
  (b) colours   the scene's f_dc and opacities perturbed; they are optimised against `views` fixed cameras.  Error: RMS of f_dc and
                of the opacity logits against the true ones.
--loss dssim runs (a) on autograd.photometric_loss, (1 - 0.2) L1 + 0.2 (1 - SSIM), instead of the L1 composed in torch (the default,
which profiles/raster_backward.md recorded).  rodrigues and compose live in 6dgs_amd/refine.py, which batches (a) as refine_poses.
Prints loss and parameter error every 10 steps.  No thresholds: a demonstration (profiles/raster_backward.md keeps its output)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BACKGROUND = (1.0, 1.0, 1.0)


def pose_error(row, true):
    a, b = row[:12].reshape(3, 4).detach().double(), true[:12].reshape(3, 4).double()
    ca, cb = -a[:, :3].T @ a[:, 3], -b[:, :3].T @ b[:, 3]                   # camera centres
    cos = ((a[:, :3] @ b[:, :3].T).trace() - 1) / 2
    return float((ca - cb).norm()), float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=20_000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--loss", choices=["l1", "dssim"], default="l1", help="(a): L1 composed in torch, or the fused L1 + D-SSIM loss")
    args = ap.parse_args()
    syn, ops = importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")
    autograd, render = importlib.import_module("6dgs_amd.autograd"), importlib.import_module("6dgs_amd.render")
    compose = importlib.import_module("6dgs_amd.refine").compose
    sc = syn.make_scene(args.gaussians, 0)
    scene = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")]
    rows = torch.from_numpy(render.camera_rows(syn.make_cameras(args.views, 21, width=args.size, height=args.size))).cuda()
    size = (args.size, args.size)
    target = ops.raster_views(*scene, 3, rows, *size, want_float=True, want_u8=False, background=BACKGROUND)

    print(f"(a) pose: {args.gaussians} Gaussians, {args.size} x {args.size}, one view, Adam lr 2e-3 on (translation, axis-angle)")
    off = torch.tensor([0.03, -0.02, 0.04, 0.02, -0.015, 0.01], device="cuda")      # ~0.05 scene units, ~1.5 degrees
    start = compose(rows[0], off).detach()
    delta = torch.zeros(6, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([delta], lr=2e-3)
    for step in range(args.steps + 1):
        row = compose(start, delta)
        image = autograd.raster_views(*scene, 3, row[None], *size, background=BACKGROUND)
        if args.loss == "dssim":
            loss = autograd.photometric_loss(image, target[:1], 0.2).sum()
        else:
            loss = (image[..., :3] - target[:1, ..., :3]).abs().mean()
        if step % 10 == 0:
            terr, rerr = pose_error(row, rows[0])
            print(f"  step {step:4d}: {'L1' if args.loss == 'l1' else 'L1 + D-SSIM'} {float(loss.detach()):.5f}, centre error {terr:.5f}, rotation error {rerr:.4f} deg")
        opt.zero_grad()
        loss.backward()
        opt.step()

    print(f"(b) colours: f_dc + N(0, 0.5), opacity logits + N(0, 1); {args.views} fixed views, Adam lr 2e-2")
    gen = torch.Generator(device="cuda").manual_seed(3)
    f_dc = (scene[4] + 0.5 * torch.randn(scene[4].shape, device="cuda", generator=gen)).requires_grad_(True)
    opacity = (scene[3] + torch.randn(scene[3].shape, device="cuda", generator=gen)).requires_grad_(True)
    opt = torch.optim.Adam([f_dc, opacity], lr=2e-2)
    for step in range(args.steps + 1):
        image = autograd.raster_views(scene[0], scene[1], scene[2], opacity, f_dc, scene[5], 3, rows, *size, background=BACKGROUND)
        loss = (image[..., :3] - target[..., :3]).abs().mean()
        if step % 10 == 0:
            print(f"  step {step:4d}: L1 {float(loss.detach()):.5f}, f_dc RMS error {float((f_dc - scene[4]).pow(2).mean().sqrt()):.4f}, "
                  f"opacity logit RMS error {float((opacity - scene[3]).pow(2).mean().sqrt()):.4f}")
        opt.zero_grad()
        loss.backward()
        opt.step()


if __name__ == "__main__":
    main()
