"""Time the one-launch Adam kernel (sixdgs_gaussian_adam) alone.

    python tools/time_adam.py [--gaussians 500000] [--n_coef 16] [--iters 20] [--rounds 3]

Three arms on the same six tensors, alternating `rounds` times after a warm-up, each timed by HIP events over `iters` back-to-back
steps: ops.gaussian_adam (one launch for all groups), torch.optim.Adam (default arguments, so foreach) over six groups with six
rates, and a device-to-device copy of the bytes the kernel moves -- seven 4-byte streams per entry (p, m, v read and written, g read):
a copy of 3.5 floats per entry reads and writes that much.  Prints microseconds per step and the bandwidth each implies; asserts
nothing."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--n_coef", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_adam needs a GPU")
    ops = importlib.import_module("6dgs_amd.ops")
    n, nc = args.gaussians, args.n_coef
    gen = torch.Generator(device="cuda").manual_seed(0)
    widths = dict(zip(ops.FIT_GROUPS, (3, 3, 3 * (nc - 1), 1, 3, 4)))
    params = {k: torch.randn(n * w, device="cuda", generator=gen) for k, w in widths.items()}
    shapes = {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, nc - 1, 3), "opacity": (n,), "scale": (n, 3), "rot": (n, 4)}
    params = {k: v.reshape(shapes[k]) for k, v in params.items()}
    grads = {k: 1e-3 * torch.randn(v.shape, device="cuda", generator=gen) for k, v in params.items()}
    entries = n * (11 + 3 * nc)
    traffic = 7 * 4 * entries
    state = ops.gaussian_adam_state(params)
    tparams = [v.clone().requires_grad_(True) for v in params.values()]
    for p, g in zip(tparams, grads.values()):
        p.grad = g.clone()
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(tparams, LRS)], lr=0.0, eps=1e-15)
    src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    step = [0]

    def hip():
        ops.gaussian_adam(params, grads, state, step[0], LRS)
        step[0] += 1

    arms = {"gaussian_adam": hip, "torch.optim.Adam": opt.step, "copy": lambda: dst.copy_(src)}
    us = {k: [] for k in arms}
    for rnd in range(args.rounds + 1):                    # round 0 warms every arm up
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if rnd:
                us[name].append(1e3 * a.elapsed_time(b) / args.iters)
    print(f"{n} Gaussians, n_coef {nc}: {entries} entries, {traffic / 1e6:.1f} MB of traffic per step; {args.iters} steps per timing, {args.rounds} rounds")
    for name, v in us.items():
        med = float(np.median(v))
        print(f"{name:18s}: us per step, each round: {', '.join(f'{x:.1f}' for x in v)}; median {med:.1f} = {traffic / med / 1e6:.2f} TB/s of the kernel's traffic")
    print(f"gaussian_adam / copy {np.median(us['gaussian_adam']) / np.median(us['copy']):.3f}; torch.optim.Adam / gaussian_adam "
          f"{np.median(us['torch.optim.Adam']) / np.median(us['gaussian_adam']):.3f}; status {int(state['status'])}")


if __name__ == "__main__":
    main()
