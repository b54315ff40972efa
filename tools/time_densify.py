"""Time the densification kernels and what the statistics add to a fused fitting step; writes profiles/densify.md's tables.

    python tools/time_densify.py [--gaussians 500000] [--n_coef 16] [--size 200] [--steps 20] [--rounds 3] [--out profiles/densify.md]

A stand-in scene (synthetic.make_scene) is rendered once at size x size; HIP events in one process:
  1. sixdgs_densify_stats behind a forward and a backward of that view, 20 back-to-back calls;
  2. one round at thresholds taken from the scene's own statistics (the median positive average gradient, the median largest scale), so that
     all three classes occur: ops.densify_raw (sixdgs_densify into kept buffers, no host read) against fit.densify_torch, the two
     arms alternating `rounds` times after a warm-up call each;
  3. `steps` steps of sixdgs_fit_scene_steps with the statistics on every step against the same call without them, alternating.
Prints the figures as markdown and writes them to --out; asserts nothing."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")

ORDER = ("xyz", "scale", "rot", "opacity", "f_dc", "f_rest")
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scale": "_scaling", "rot": "_rotation"}


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def row(name, v, unit=1.0, digits=1):
    return f"| {name} | {', '.join(f'{x * unit:.{digits}f}' for x in v)} | **{np.median(v) * unit:.{digits}f}** |"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_densify needs a GPU")
    pkg, syn, ops = (importlib.import_module(m) for m in ("6dgs_amd", "6dgs_amd.synthetic", "6dgs_amd.ops"))
    fit, render = importlib.import_module("6dgs_amd.fit"), importlib.import_module("6dgs_amd.render")
    n, size = args.gaussians, args.size
    scene = pkg.GaussianScene.from_dict(syn.make_scene(n, args.seed), device="cuda")
    views = render.render_views(scene, syn.make_cameras(1, args.seed + 200, width=size, height=size), renderer="raster")
    rows = torch.from_numpy(render.camera_rows(views)).cuda()
    target = torch.from_numpy(np.ascontiguousarray(views[0].image[..., :3]))[None].cuda().contiguous()
    p = {k: getattr(scene, a).detach().float().contiguous().clone() for k, a in ATTR.items()}
    p["f_dc"] += 0.05 * torch.randn(p["f_dc"].shape, generator=torch.Generator().manual_seed(1)).cuda()       # something to fit
    n_coef = 1 + p["f_rest"].shape[1]
    arrays = [p[k] for k in ORDER]
    lines = [f"`tools/time_densify.py`: {n} Gaussians, `n_coef = {n_coef}`, one {size} x {size} view, {args.rounds} rounds.", ""]
    # 1. the statistics kernel
    image, radii, needed, fwd = ops.raster_views(*arrays, 3, rows, size, size, want_float=True, want_u8=False, want_radii=True, want_instances=True,
                                                 want_state=True)
    _, grad = ops.photometric_loss(image, target, want_grad=True)
    bwd_ws = torch.empty(ops.raster_views_backward_workspace_bytes(n, 1, size, size, fwd[1]), dtype=torch.uint8, device="cuda")
    ops.raster_views_backward(*arrays, 3, rows, size, size, grad, fwd, workspace=bwd_ws, want=ORDER)
    stats = ops.densify_stats_state(n, "cuda")
    ops.densify_stats(fwd, bwd_ws, radii, stats, size, size)
    t_stats = [timed(lambda: ops.densify_stats(fwd, bwd_ws, radii, stats, size, size), 20) for _ in range(args.rounds)]
    visible = int((radii > 0).sum())
    lines += [f"{visible} of the Gaussians are visible and hold {needed} tile instances.", "", "| call | us per call, each round | median |", "|---|---|---|",
              row("`ops.densify_stats` (`k_densify_stats`)", t_stats, 1e3), ""]
    # 2. one round
    stats = ops.densify_stats_state(n, "cuda")
    ops.densify_stats(fwd, bwd_ws, radii, stats, size, size)
    avg = stats["grad_accum"][stats["grad_accum"] > 0]         # one pass: the sum is the average; many visible Gaussians blend into no pixel
    sigma = torch.exp(p["scale"].max(dim=1).values)
    extent = 1.0
    kw = dict(grad_threshold=float(avg.median()), percent_dense=float(sigma.median()) / extent, extent=extent, min_opacity=0.005, prune_big=True)
    state = ops.gaussian_adam_state(p)
    noise = fit.round_noise(n, 0, 0, "cuda")
    out = ops.densify_buffers(p, 2 * n)
    sl = ops.gaussian_adam_slices(n, n_coef)
    tstate = {k: (state["m"][sl[k]].reshape(p[k].shape), state["v"][sl[k]].reshape(p[k].shape)) for k in ops.FIT_GROUPS}
    arms = {"`ops.densify_raw` (`sixdgs_densify`: classify, scan, scatter)": lambda: ops.densify_raw(p, state, stats, noise, out, **kw),
            "`fit.densify_torch` (masks, cat, indexing; its counts are host reads)": lambda: fit.densify_torch(p, tstate, stats, noise, **kw)}
    ms = {k: [] for k in arms}
    for rnd in range(args.rounds + 1):
        for k, fn in arms.items():
            t = timed(fn)
            if rnd:
                ms[k].append(t)
    counts = ops.densify_raw(p, state, stats, noise, out, **kw).cpu().tolist()
    lines += [f"One round at `grad_threshold` = the median positive average gradient and `percent_dense * extent` = the median largest scale: n {n} -> "
              f"{counts[0]} ({counts[1]} clones, {counts[2]} split sources, {counts[3]} candidates pruned).", "",
              "| arm | ms per round, each round | median |", "|---|---|---|", *[row(k, v, 1.0, 3) for k, v in ms.items()], ""]
    # 3. a fused step with the statistics against one without
    steps = args.steps
    vs, lrs = np.zeros((steps, 1), np.int32), np.array([[fit.position_lr(s + 1), 2.5e-3, 2.5e-3 / 20.0, 0.05, 5e-3, 1e-3] for s in range(steps)])
    ws = torch.empty(ops.fit_scene_steps_workspace_bytes(n, n_coef, 1, size, size, fwd[1]), dtype=torch.uint8, device="cuda")

    def segment(with_stats):
        q = {k: v.clone() for k, v in p.items()}
        st = ops.gaussian_adam_state(q)
        st["instances_needed"] = torch.zeros(1, dtype=torch.int64, device="cuda")
        acc = ops.densify_stats_state(n, "cuda")
        call = lambda: ops.fit_scene_steps_raw(q, rows, size, size, target, st, views=vs, lrs=lrs, sh_degrees=[3] * steps,       # noqa: E731
                                               stats_steps=[int(with_stats)] * steps, stats=acc, max_instances=fwd[1], workspace=ws)
        t = timed(call) / steps
        assert int(st["status"]) == 0
        return t
    per = {"with the statistics on every step": [], "without": []}
    for rnd in range(args.rounds + 1):
        for k, flag in (("with the statistics on every step", True), ("without", False)):
            t = segment(flag)
            if rnd:
                per[k].append(t)
    a, b = np.median(per["with the statistics on every step"]), np.median(per["without"])
    lines += [f"`sixdgs_fit_scene_steps`, {steps} steps of the one view per call, the two arms alternating:", "",
              "| arm | ms per step, each round | median |", "|---|---|---|", *[row(k, v, 1.0, 3) for k, v in per.items()],
              "", f"The statistics add {1e3 * (a - b):.1f} us to a step of {b:.3f} ms ({100 * (a / b - 1):.2f} %).", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
