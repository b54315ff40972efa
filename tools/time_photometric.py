"""Time the fused photometric loss (ops.photometric_loss) against the same loss composed in PyTorch on the GPU, and against the
rasteriser it follows in a refinement step.

    python tools/time_photometric.py [--sizes 200 800] [--views 1 4] [--gaussians 500000] [--repeats 5] [--inner 20]

Per size and number of views: the image is fp32 [V,S,S,4] (the rasteriser's), the target uint8 [V,S,S,3].
  fused      ops.photometric_loss, the loss alone and with want_grad (one C call either way)
  composed   (1 - 0.2) L1 + 0.2 (1 - SSIM) with F.conv2d of the 11 x 11 window, groups = 3, padding 5, on [V,3,S,S] fp32 tensors laid out
             beforehand (the layout change is not timed); its gradient by autograd
  raster     ops.raster_views (float image) + ops.raster_views_backward (all seven gradients) of make_scene(N, 0) at the same size,
             exact instance capacity, for the share the loss takes of a refinement step's GPU work
HIP events around `inner` back-to-back calls, the windows of the variants alternating; the median of `repeats` windows after a
warm-up window each.  There is no earlier version of this loss to compare with: the composition is the yardstick.  Prints ms per call,
fused / composed, and fused (with gradient) / (raster forward + backward)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAMBDA = 0.2


def window(device):
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    w = torch.from_numpy((g / g.sum()).astype(np.float32)).to(device)
    return (w[:, None] * w[None, :]).expand(3, 1, 11, 11).contiguous()


def composed(a, b, win):
    """a, b [V,3,S,S] -> loss [V]."""
    mu1, mu2 = F.conv2d(a, win, padding=5, groups=3), F.conv2d(b, win, padding=5, groups=3)
    s1 = F.conv2d(a * a, win, padding=5, groups=3) - mu1 * mu1
    s2 = F.conv2d(b * b, win, padding=5, groups=3) - mu2 * mu2
    s12 = F.conv2d(a * b, win, padding=5, groups=3) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    return (1 - LAMBDA) * (a - b).abs().mean(dim=(1, 2, 3)) + LAMBDA * (1 - m.mean(dim=(1, 2, 3)))


def windows(variants, repeats, inner):
    """variants: name -> callable.  -> name -> median ms per call over `repeats` windows of `inner` calls, the variants alternating."""
    for fn in variants.values():
        for _ in range(3):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 800])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_photometric needs a GPU")
    syn, ops = importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")
    render = importlib.import_module("6dgs_amd.render")
    sc = syn.make_scene(args.gaussians, 0)
    scene = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + [3]
    win = window("cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for size in args.sizes:
        for views in args.views:
            cams = torch.from_numpy(render.camera_rows(syn.make_cameras(views, 21, width=size, height=size))).cuda()
            image, count, state = ops.raster_views(*scene, cams, size, size, want_float=True, want_u8=False, want_instances=True, want_state=True)
            fws = torch.empty(ops.raster_views_workspace_bytes(args.gaussians, views, size, size, count), dtype=torch.uint8, device="cuda")
            bws = torch.empty(ops.raster_views_backward_workspace_bytes(args.gaussians, views, size, size, count), dtype=torch.uint8, device="cuda")
            target = (image[..., :3] * 255 + 8 * torch.randn(image[..., :3].shape, device="cuda", generator=gen)).clamp(0, 255).to(torch.uint8).contiguous()
            ws = torch.empty(ops.photometric_loss_workspace_bytes(views, size, size, True), dtype=torch.uint8, device="cuda")
            a_t = image[..., :3].permute(0, 3, 1, 2).contiguous()
            # u / 255 correctly rounded, as the fused call forms it (torch's division on the GPU is not: one ulp off where the image is
            # exactly u / 255 turns sign(0) = 0 of the L1 term into +-1)
            b_t = torch.from_numpy(target.cpu().numpy().astype(np.float32) / np.float32(255.0)).cuda().permute(0, 3, 1, 2).contiguous()
            a_g = a_t.clone().requires_grad_(True)
            grad = torch.randn(image.shape, device="cuda", generator=gen)
            # the two agree before they are timed
            fused_loss, fused_grad = ops.photometric_loss(image, target, lambda_dssim=LAMBDA, want_grad=True, workspace=ws)
            ref = composed(a_g, b_t, win)
            ref.sum().backward()
            d_loss = float((fused_loss - ref.detach()).abs().max())
            d_grad = float((fused_grad[..., :3].permute(0, 3, 1, 2) - a_g.grad).abs().max() / a_g.grad.abs().max())
            state_box = [state]

            def raster_fwd():
                state_box[0] = ops.raster_views(*scene, cams, size, size, want_float=True, want_u8=False, want_state=True, max_instances=count,
                                                workspace=fws)[1]

            def composed_grad():
                a_g.grad = None
                composed(a_g, b_t, win).sum().backward()

            def composed_fwd():
                with torch.no_grad():
                    composed(a_t, b_t, win)

            r = windows({
                "fused_fwd": lambda: ops.photometric_loss(image, target, lambda_dssim=LAMBDA, workspace=ws),
                "composed_fwd": composed_fwd,
                "fused_grad": lambda: ops.photometric_loss(image, target, lambda_dssim=LAMBDA, want_grad=True, workspace=ws),
                "composed_grad": composed_grad,
                "raster_fwd": raster_fwd,
                "raster_bwd": lambda: ops.raster_views_backward(*scene, cams, size, size, grad, state_box[0], workspace=bws),
            }, args.repeats, args.inner)
            raster = r["raster_fwd"][0] + r["raster_bwd"][0]
            print(f"{size} x {size}, {views} view(s): max |fused - composed| loss {d_loss:.2e}, gradient {d_grad:.2e} of its scale")
            for k, (med, lo, hi) in r.items():
                print(f"  {k:14s} {med:8.3f} ms per call (min {lo:.3f}, max {hi:.3f}), {med / views:8.3f} per view")
            print(f"  fused / composed: forward {r['fused_fwd'][0] / r['composed_fwd'][0]:.3f}, forward + gradient "
                  f"{r['fused_grad'][0] / r['composed_grad'][0]:.3f}; fused forward + gradient / (raster forward + backward, {args.gaussians} Gaussians) "
                  f"{r['fused_grad'][0] / raster:.3f}")


if __name__ == "__main__":
    main()
