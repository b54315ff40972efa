"""Time ops.raster_views stage by stage (HIP events inside the library call: project, scan, emit, sort, ranges, blend).

    python tools/time_raster.py [--gaussians 500000] [--size 800] [--views 1 4] [--repeats 5] [--backward]

Scene make_scene(N, 0), cameras make_cameras(V, 21).  Each launch runs with the exact instance capacity (found by a first call), so the
sort runs over no padding.  Prints the instances per view and, per stage, the median milliseconds per view.  --backward also times
ops.raster_views_backward (blend_bwd, project_bwd, cams; all seven gradients, standard-normal grad_image) on the forward's state, and
prints the backward / forward ratio of the stages together."""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = ("project", "scan", "emit", "sort", "ranges", "blend")
BACKWARD_STAGES = ("blend_bwd", "project_bwd", "cams")


def slot_ms(lib, Profile, prof):
    """Milliseconds of every slot of `prof` (the events are destroyed, the struct is reset)."""
    out = []
    for i in range(prof.count):
        one = Profile()
        one.count, one.start[0], one.stop[0] = 1, prof.start[i], prof.stop[i]
        ms = C.c_double(0.0)
        if lib.sixdgs_profile_collect(C.byref(one), C.byref(ms), None, None, None) != 0:
            raise RuntimeError("sixdgs_profile_collect failed")
        out.append(ms.value)
    prof.count = 0
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--backward", action="store_true", help="also time ops.raster_views_backward on the forward's state")
    args = ap.parse_args()
    syn, ops = importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")
    _lib = importlib.import_module("6dgs_amd._lib")
    render = importlib.import_module("6dgs_amd.render")
    lib = _lib.load()
    sc = syn.make_scene(args.gaussians, 0)
    scene = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("xyz", "log_scale", "rot", "opacity", "f_dc", "f_rest")] + [3]
    for views in args.views:
        cams = torch.from_numpy(render.camera_rows(syn.make_cameras(views, 21, width=args.size, height=args.size))).cuda()
        _, count = ops.raster_views(*scene, cams, args.size, args.size, want_instances=True)
        ws = torch.empty(ops.raster_views_workspace_bytes(args.gaussians, views, args.size, args.size, count), dtype=torch.uint8, device="cuda")
        rows, wall = [], []
        for _ in range(args.repeats):
            prof = _lib.Profile()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.raster_views(*scene, cams, args.size, args.size, max_instances=count, workspace=ws, profile=prof)
            b.record()
            torch.cuda.synchronize()
            rows.append(slot_ms(lib, _lib.Profile, prof))
            wall.append(a.elapsed_time(b))
        med = np.median(np.asarray(rows), axis=0) / views
        print(f"{args.gaussians} Gaussians, {args.size} x {args.size}, {views} view(s) per launch: {count / views:.0f} instances per view, "
              f"workspace {ws.numel() / 2 ** 20:.0f} MiB")
        print("  ms per view, median of %d launches: " % args.repeats + ", ".join(f"{s} {m:.3f}" for s, m in zip(STAGES, med)) +
              f"; stages together {med.sum():.3f}; whole call (events around it, with the read of the count) {np.median(wall) / views:.3f}")
        if not args.backward:
            continue
        image, state = ops.raster_views(*scene, cams, args.size, args.size, max_instances=count, workspace=ws, want_float=True, want_u8=False,
                                        want_state=True)
        grad = torch.randn(image.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        bws = torch.empty(ops.raster_views_backward_workspace_bytes(args.gaussians, views, args.size, args.size, count), dtype=torch.uint8,
                          device="cuda")
        rows, wall = [], []
        for _ in range(args.repeats + 1):       # (the first launch is the warm-up)
            prof = _lib.Profile()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.raster_views_backward(*scene, cams, args.size, args.size, grad, state, workspace=bws, profile=prof)
            b.record()
            torch.cuda.synchronize()
            rows.append(slot_ms(lib, _lib.Profile, prof))
            wall.append(a.elapsed_time(b))
        bmed = np.median(np.asarray(rows[1:]), axis=0) / views
        print("  backward, ms per view: " + ", ".join(f"{s} {m:.3f}" for s, m in zip(BACKWARD_STAGES, bmed)) +
              f"; stages together {bmed.sum():.3f}; whole call {np.median(wall[1:]) / views:.3f}; backward / forward {bmed.sum() / med.sum():.2f}; "
              f"workspace {bws.numel() / 2 ** 20:.0f} MiB")


if __name__ == "__main__":
    main()
