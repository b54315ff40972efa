"""Time the contribution pass (ops.raster_contrib: walk, gather) against the forward it reads and against the only other route to a
Gaussian's summed alpha T: ops.raster_views_backward with a red-only gradient.

    python tools/time_contrib.py [--gaussians 500000] [--shapes 1x800 8x200] [--repeats 5]

Scene make_scene(N, 0), cameras make_cameras(V, 21); a shape is VIEWSxSIDE.  HIP events inside the library calls.  Each launch runs with
the exact instance capacity (found by a first call).  Per shape: the forward's stages of the same call (no image: the blend does not
run), walk and gather, and the backward route's stages -- blend_bwd and project_bwd with only d f_dc wanted and grad_image = (1, 0, 0, 0).
Milliseconds per launch, the median of the repeats after a warm-up."""
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
from time_raster import slot_ms  # noqa: E402

FORWARD_STAGES = ("project", "scan", "emit", "sort", "ranges")
CONTRIB_STAGES = ("walk", "gather")
BACKWARD_STAGES = ("blend_bwd", "project_bwd")


def median_slots(lib, Profile, repeats, launch):
    rows = []
    for _ in range(repeats + 1):          # (the first launch is the warm-up)
        prof = Profile()
        launch(prof)
        torch.cuda.synchronize()
        rows.append(slot_ms(lib, Profile, prof))
    return np.median(np.asarray(rows[1:]), axis=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--shapes", nargs="+", default=["1x800", "8x200"], help="VIEWSxSIDE per entry")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    syn, ops = importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")
    _lib = importlib.import_module("6dgs_amd._lib")
    render = importlib.import_module("6dgs_amd.render")
    lib = _lib.load()
    n = args.gaussians
    sc = syn.make_scene(n, 0)
    scene = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + [3]
    for shape in args.shapes:
        views, side = (int(x) for x in shape.split("x"))
        cams = torch.from_numpy(render.camera_rows(syn.make_cameras(views, 21, width=side, height=side))).cuda()
        count = ops.raster_views(*scene, cams, side, side, want_u8=False, want_instances=True)
        ws = torch.empty(ops.raster_views_workspace_bytes(n, views, side, side, count), dtype=torch.uint8, device="cuda")
        cws = torch.empty(ops.raster_contrib_workspace_bytes(n, views, side, side, count), dtype=torch.uint8, device="cuda")
        bws = torch.empty(ops.raster_views_backward_workspace_bytes(n, views, side, side, count), dtype=torch.uint8, device="cuda")
        fwd = median_slots(lib, _lib.Profile, args.repeats, lambda prof: ops.raster_views(
            *scene, cams, side, side, want_u8=False, want_state=True, max_instances=count, workspace=ws, profile=prof))
        state = ops.raster_views(*scene, cams, side, side, want_u8=False, want_state=True, max_instances=count, workspace=ws)
        acc = ops.contrib_state(n, "cuda")
        con = median_slots(lib, _lib.Profile, args.repeats, lambda prof: ops.raster_contrib(state, n, views, side, side, acc, workspace=cws,
                                                                                            profile=prof))
        got = ops.raster_contrib(state, n, views, side, side, want_views=True, workspace=cws)
        grad = torch.zeros(views, side, side, 4, device="cuda")
        grad[..., 0] = 1.0
        bwd = median_slots(lib, _lib.Profile, args.repeats, lambda prof: ops.raster_views_backward(
            *scene, cams, side, side, grad, state, want=("f_dc",), workspace=bws, profile=prof))
        inert = float(((got["pixels"] == 0) & (got["stops"] == 0)).float().mean())
        print(f"{n} Gaussians, {views} view(s) of {side} x {side}: {count} instances; {100 * inert:.1f} % of the Gaussians inert; "
              f"{int(got['pixels'].sum())} adds, {int(got['stops'].sum())} stops; workspaces forward {ws.numel() / 2 ** 20:.0f} MiB, "
              f"contribution {cws.numel() / 2 ** 20:.0f} MiB, backward {bws.numel() / 2 ** 20:.0f} MiB")
        print("  forward without an image, ms per launch: " + ", ".join(f"{s} {m:.3f}" for s, m in zip(FORWARD_STAGES, fwd)) + f"; together {fwd.sum():.3f}")
        print("  contribution: " + ", ".join(f"{s} {m:.3f}" for s, m in zip(CONTRIB_STAGES, con)) + f"; together {con.sum():.3f}")
        print("  backward route (red-only gradient, d f_dc only): " + ", ".join(f"{s} {m:.3f}" for s, m in zip(BACKWARD_STAGES, bwd)) +
              f"; together {bwd.sum():.3f}; contribution / backward route {con.sum() / bwd.sum():.2f}")


if __name__ == "__main__":
    main()
