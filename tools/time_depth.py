"""Time the depth pass (ops.raster_depth: walk) beside the two walks of the same list it is modelled on, in one process: the forward's
blend and the contribution pass's walk.

    python tools/time_depth.py [--gaussians 500000] [--shapes 1x800 4x800] [--repeats 7]

Scene make_scene(N, 0), cameras make_cameras(V, 21); a shape is VIEWSxSIDE.  HIP events inside the library calls.  Each launch runs with
the exact instance capacity (found by a first call).  Per shape: the forward's stages with the float image, the contribution pass's walk
and gather, and the depth walk with the four maps, with the maps and median points, and with alpha alone.  Milliseconds per launch, the
median of the repeats after a warm-up; the launches of the three passes alternate, so that none of them has the clocks to itself."""
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

FORWARD_STAGES = ("project", "scan", "emit", "sort", "ranges", "blend")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--shapes", nargs="+", default=["1x800", "4x800"], help="VIEWSxSIDE per entry")
    ap.add_argument("--repeats", type=int, default=7)
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
        forward = lambda prof=None: ops.raster_views(*scene, cams, side, side, want_float=True, want_u8=False, want_state=True,      # noqa: E731
                                                     max_instances=count, workspace=ws, profile=prof)
        image, state = forward()
        acc = ops.contrib_state(n, "cuda")
        passes = {"forward": forward,
                  "contribution": lambda prof: ops.raster_contrib(state, n, views, side, side, acc, workspace=cws, profile=prof),
                  "depth, four maps": lambda prof: ops.raster_depth(state, n, views, side, side, profile=prof),
                  "depth, four maps and median points": lambda prof: ops.raster_depth(state, n, views, side, side, cams=cams, points="median", profile=prof),
                  "depth, alpha alone": lambda prof: ops.raster_depth(state, n, views, side, side, want=("alpha",), profile=prof)}
        rows = {k: [] for k in passes}
        for _ in range(args.repeats + 1):          # (the first round is the warm-up)
            for k, launch in passes.items():
                prof = _lib.Profile()
                launch(prof)
                torch.cuda.synchronize()
                rows[k].append(slot_ms(lib, _lib.Profile, prof))
        ms = {k: np.median(np.asarray(v[1:]), axis=0) for k, v in rows.items()}
        got = ops.raster_depth(state, n, views, side, side)
        assert torch.equal(got["alpha"], image[..., 3])
        print(f"{n} Gaussians, {views} view(s) of {side} x {side}: {count} instances, {count / (views * ((side + 15) // 16) ** 2):.0f} per tile; "
              f"{100 * float((got['median_index'] >= 0).float().mean()):.1f} % of the pixels have a median, mean alpha {float(got['alpha'].mean()):.3f}")
        print("  forward with the float image, ms per launch: " + ", ".join(f"{s} {m:.3f}" for s, m in zip(FORWARD_STAGES, ms["forward"])))
        print("  contribution: " + ", ".join(f"{s} {m:.3f}" for s, m in zip(("walk", "gather"), ms["contribution"])))
        for k in list(passes)[2:]:
            print(f"  {k}: walk {ms[k][0]:.3f} ({ms[k][0] / ms['forward'][5]:.2f} of the blend, {ms[k][0] / ms['contribution'][0]:.2f} of the contribution walk)")


if __name__ == "__main__":
    main()
