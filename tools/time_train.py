"""Iterations per second of train_id_module at the reference's training size, per-image loop against the batched window:

    python tools/time_train.py [--mode both|loop|window|none] [--warmup 2] [--iters 5] [--cameras 50] [--kernels] [--images 32] [--ray-groups 1]

1000 ellipsoids (the reference's max_ellipsoids; ~28.7 k quadricell rays), 32 images per iteration, 800 x 800 synthetic RGB cameras
(6dgs_amd/synthetic.py), rays renewed every 10 iterations as in training, evaluation switched off.  Each mode runs warm-up iterations
and then N timed ones; an iteration ends where train_id_module logs its loss (both modes read their scalars on the host there, so the
host clock sees finished work).  --kernels also times the scorer alone at the same size on the device clock: the forward
(ops.ray_attention_scores) and its backward (sixdgs_score_backward) for 32 images of 256 tokens, with the algorithmic TFLOP/s
(2 T R 384 per logit or product pass: 1 pass forward, 3 + 2 backward).
--images B: the images per iteration of the window mode and the --kernels timing (the per-image loop keeps 32); --ray-groups G: the split
of the scorer's backward over the rays (train_id_module(backward_ray_groups=G); 1 = unsplit, 0 = auto).  Both take comma-separated
lists: the window mode and the backward are then timed for every pair, each entry keyed "B<b>_G<g>" (g as given) with the G that auto
resolved to.  Prints one JSON line."""
import argparse
import functools
import importlib
import json
import os
import sys
import time
import types

os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("6dgs_amd")
syn = importlib.import_module("6dgs_amd.synthetic")
ops = importlib.import_module("6dgs_amd.ops")


def module():
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(0, with_cnn=True).items()}, strict=False)
    return idm.cuda()


def time_mode(batched, scene, info, warmup, iters, images=32, ray_groups=1):
    torch.manual_seed(0)
    idm = module()
    stamps = []

    def log_fn(tag, value, it):
        if tag == "train/loss":
            stamps.append(time.perf_counter())

    t0 = time.perf_counter()
    pkg.train_id_module("/tmp/time_train_id_module.th", "cuda", idm, functools.partial(pkg.generate_all_possible_rays, scene), info, "seq", "cat",
                        n_iterations=warmup + iters, display_every_n_iterations=10 ** 9, val_every_n_iterations=10 ** 9, log_fn=log_fn,
                        batched_window=batched, gradient_accumulation_steps=images if batched else 32, backward_ray_groups=ray_groups)
    torch.cuda.synchronize()
    per_it = (stamps[-1] - stamps[warmup - 1]) / iters if warmup > 0 else (stamps[-1] - t0) / iters
    return 1.0 / per_it


def resolved_ray_groups(b, r, ray_groups):
    """The G sixdgs_score_backward_split runs for (b, r, ray_groups): from its workspace size, which is the unsplit workspace plus
    G x B x 256 x (2 + 384) floats when G > 1 (both parts are multiples of the 256-byte alignment)."""
    lib = importlib.import_module("6dgs_amd._lib").load()
    extra = lib.sixdgs_score_backward_split_workspace_bytes(b, r, ray_groups) - lib.sixdgs_score_backward_workspace_bytes(b)
    return 1 if extra == 0 else extra // (b * 256 * 386 * 4)


def time_kernels(r, reps=5, b=32, ray_groups=1):
    gen = torch.Generator().manual_seed(0)
    q = (torch.randn(b, 256, 384, generator=gen) * 0.05).cuda().requires_grad_(True)
    k = torch.randn(r, 384, generator=gen).cuda().requires_grad_(True)
    n_tok = torch.full((b,), 256, dtype=torch.int32, device="cuda")
    g = torch.randn(b, r, device="cuda")
    out = {}
    for name in ("forward", "backward"):
        ts = []
        for _ in range(reps):
            s = ops.ray_attention_scores(q, n_tok, k, ray_groups) if name == "backward" else None
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "forward":
                ops.ray_attention_scores(q, n_tok, k)
            else:
                torch.autograd.grad(s, (q, k), g)
            e.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(e))
        ms = min(ts[1:])
        flop = 2.0 * b * 256 * r * 384 * (1 if name == "forward" else 5)
        out[name] = {"ms": round(ms, 3), "tflops": round(flop / ms / 1e9, 1)}
    out["ray_groups"] = resolved_ray_groups(b, r, ray_groups)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("both", "loop", "window", "none"), default="both", help="none: --kernels only")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cameras", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--images", default="32", help="images per window iteration and per --kernels timing (comma-separated list)")
    ap.add_argument("--ray-groups", default="1", help="backward ray groups, 0 = auto (comma-separated list)")
    a = ap.parse_args()
    images = [int(x) for x in a.images.split(",")]
    groups = [int(x) for x in a.ray_groups.split(",")]
    single = len(images) == 1 and len(groups) == 1
    scene = pkg.GaussianScene.from_dict(syn.make_scene(1000, 0), device="cuda")
    cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(a.cameras, 1, width=800, height=800)]
    info = types.SimpleNamespace(train_cameras=cams, test_cameras=cams[:1])
    r = int(pkg.generate_all_possible_rays(scene)[0].shape[0])
    res = {"rays": r, "images_per_iteration": images[0] if single else images, "ray_groups": groups[0] if single else groups,
           "warmup": a.warmup, "iters": a.iters}
    if a.mode in ("both", "loop"):
        res["loop_it_per_s"] = round(time_mode(False, scene, info, a.warmup, a.iters), 3)
    if a.mode in ("both", "window"):
        if single:
            res["window_it_per_s"] = round(time_mode(True, scene, info, a.warmup, a.iters, images[0], groups[0]), 3)
        else:
            res["window_it_per_s"] = {f"B{b}_G{g}": round(time_mode(True, scene, info, a.warmup, a.iters, b, g), 3) for b in images for g in groups}
    if a.mode == "both" and single:
        res["speedup"] = round(res["window_it_per_s"] / res["loop_it_per_s"], 2)
    if a.kernels:
        if single and images[0] == 32 and groups[0] == 1:
            res["scorer_32_images"] = time_kernels(r)
        else:
            res["scorer"] = {f"B{b}_G{g}": time_kernels(r, b=b, ray_groups=g) for b in images for g in groups}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
