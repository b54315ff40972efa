"""Time the target pyramid kernel against refine.prepare_target run once per level.

    python tools/time_pyramid.py [--views 8] [--size 800] [--levels 8,4,2] [--repeats 20]

On random bytes, for RGB, RGBA with the fourth channel ignored and RGBA composited over white: HIP events around one
ops.target_pyramid call for all levels (sixdgs_target_pyramid: one kernel launch per level) and around prepare_target called per level
(a chain of torch ops each), `repeats` times after 3 warm-up calls; the bytes the kernel must move (the crop read once per level, the
targets written) over its median time.  Also the largest difference between the two arms' targets.  Prints medians; asserts nothing."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats):
    ms = []
    for it in range(repeats + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            ms.append(a.elapsed_time(b))
    return out, float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--levels", default="8,4,2")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pyramid needs a GPU")
    importlib.import_module("6dgs_amd")
    ops, refine = importlib.import_module("6dgs_amd.ops"), importlib.import_module("6dgs_amd.refine")
    ds = [int(d) for d in args.levels.split(",")]
    print(f"{args.views} views of {args.size} x {args.size}, levels {ds}, {args.repeats} repeats")
    for channels, alpha in ((3, "ignore"), (4, "ignore"), (4, "composite")):
        images = torch.randint(0, 256, (args.views, args.size, args.size, channels), dtype=torch.uint8, device="cuda")
        composite = alpha == "composite"
        kernel, k_ms, k_lo, k_hi = timed(lambda: ops.target_pyramid(images, ds, composite=composite), args.repeats)
        chain, c_ms, c_lo, c_hi = timed(lambda: [refine.prepare_target(images, d, alpha)[0] for d in ds], args.repeats)
        read = sum(args.views * (args.size // d * d) ** 2 * (channels if composite or channels == 3 else 3) for d in ds)
        wrote = sum(k.numel() * 4 for k in kernel)
        diff = max(float((k - (c.float() / 255.0 if c.dtype == torch.uint8 else c)).abs().max()) for k, c in zip(kernel, chain))
        print(f"{channels} channels, alpha {alpha}: kernel median {k_ms:.3f} ms (min {k_lo:.3f}, max {k_hi:.3f}), {(read + wrote) / k_ms / 1e6:.1f} GB/s of "
              f"{(read + wrote) / 1e6:.1f} MB; prepare_target per level {c_ms:.3f} ms (min {c_lo:.3f}, max {c_hi:.3f}); ratio {c_ms / k_ms:.1f}; "
              f"max |difference| {diff:.3e}", flush=True)


if __name__ == "__main__":
    main()
