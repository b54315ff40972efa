"""Time sixdgs_knn_mean_dist2 alone; writes the tables of profiles/knn.md.

    python tools/time_knn.py [--sizes 100000 500000] [--brute 100000] [--rounds 5] [--out profiles/knn.md]

HIP events around ops.knn_mean_dist2 with a kept workspace (bounding box, Morton codes, sort, gather and search: the whole call),
one warm-up call and `rounds` timed calls per cloud, in one process:
  uniform      a unit cube
  clustered    the centres of a stand-in scene (synthetic.make_scene: a standard normal cloud)
  identical    every point the same
Beside it, at --brute points, the chunked brute force of tests/knn_reference.py (separate elementwise torch kernels and topk) on the
same GPU, whose result is compared with the kernel's bit for bit.  Prints the figures as markdown and writes them to --out; asserts
nothing but that comparison."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 500000])
    ap.add_argument("--brute", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_knn needs a GPU")
    import knn_reference as K
    syn, ops = importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops")

    def clouds(n):
        return {"uniform": K.uniform(n, args.seed), "clustered": syn.make_scene(n, args.seed)["xyz"], "identical": K.identical(n)}

    lines = [f"`tools/time_knn.py`: the whole `ops.knn_mean_dist2` call with a kept workspace, HIP events, {args.rounds} calls after a warm-up.", "",
             "| n | cloud | ms per call, each call | median |", "|---|---|---|---|"]
    med = {}
    for n in args.sizes:
        ws = torch.empty(ops.knn_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        for name, p in clouds(n).items():
            x = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
            ops.knn_mean_dist2(x, workspace=ws)
            t = [timed(lambda: ops.knn_mean_dist2(x, workspace=ws))[0] for _ in range(args.rounds)]
            med[n, name] = float(np.median(t))
            lines.append(f"| {n} | {name} | {', '.join(f'{v:.3f}' for v in t)} | **{med[n, name]:.3f}** |")
    lines.append("")
    for n in args.sizes:
        lines.append(f"n = {n}: identical / uniform = {med[n, 'identical'] / med[n, 'uniform']:.2f}, clustered / uniform = "
                     f"{med[n, 'clustered'] / med[n, 'uniform']:.2f}.")
    n = args.brute
    lines += ["", f"Chunked torch brute force (`tests/knn_reference.py: brute_torch`, chunks of 512 queries) at n = {n} on the same GPU:", "",
              "| cloud | brute force ms | kernel ms | brute force / kernel | same bits |", "|---|---|---|---|---|"]
    ws = torch.empty(ops.knn_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for name, p in clouds(n).items():
        if name == "identical":
            continue
        x = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
        K.brute_torch(x[:2048].contiguous())                                          # warm the allocator and the kernels up
        tb, want = timed(lambda: K.brute_torch(x))
        ops.knn_mean_dist2(x, workspace=ws)
        tk, got = timed(lambda: ops.knn_mean_dist2(x, workspace=ws))
        same = np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
        lines.append(f"| {name} | {tb:.1f} | {tk:.3f} | {tb / tk:.0f} | {same} |")
        assert same, f"{name}: the kernel and the brute force differ"
    lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
