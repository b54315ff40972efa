"""Iterations per second of train_id_module at the reference's training size, per-image loop against the batched window:

    python tools/time_train.py [--mode both|loop|window] [--warmup 2] [--iters 5] [--cameras 50] [--kernels]

1000 ellipsoids (the reference's max_ellipsoids; ~28.7 k quadricell rays), 32 images per iteration, 800 x 800 synthetic RGB cameras
(6dgs_amd/synthetic.py), rays renewed every 10 iterations as in training, evaluation switched off.  Each mode runs warm-up iterations
and then N timed ones; an iteration ends where train_id_module logs its loss (both modes read their scalars on the host there, so the
host clock sees finished work).  --kernels also times the scorer alone at the same size on the device clock: the forward
(ops.ray_attention_scores) and its backward (sixdgs_score_backward) for 32 images of 256 tokens, with the algorithmic TFLOP/s
(2 T R 384 per logit or product pass: 1 pass forward, 3 + 2 backward).  Prints one JSON line."""
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


def time_mode(batched, scene, info, warmup, iters):
    torch.manual_seed(0)
    idm = module()
    stamps = []

    def log_fn(tag, value, it):
        if tag == "train/loss":
            stamps.append(time.perf_counter())

    t0 = time.perf_counter()
    pkg.train_id_module("/tmp/time_train_id_module.th", "cuda", idm, functools.partial(pkg.generate_all_possible_rays, scene), info, "seq", "cat",
                        n_iterations=warmup + iters, display_every_n_iterations=10 ** 9, val_every_n_iterations=10 ** 9, log_fn=log_fn,
                        batched_window=batched)
    torch.cuda.synchronize()
    per_it = (stamps[-1] - stamps[warmup - 1]) / iters if warmup > 0 else (stamps[-1] - t0) / iters
    return 1.0 / per_it


def time_kernels(r, reps=5):
    gen = torch.Generator().manual_seed(0)
    b = 32
    q = (torch.randn(b, 256, 384, generator=gen) * 0.05).cuda().requires_grad_(True)
    k = torch.randn(r, 384, generator=gen).cuda().requires_grad_(True)
    n_tok = torch.full((b,), 256, dtype=torch.int32, device="cuda")
    g = torch.randn(b, r, device="cuda")
    out = {}
    for name in ("forward", "backward"):
        ts = []
        for _ in range(reps):
            s = ops.ray_attention_scores(q, n_tok, k) if name == "backward" else None
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("both", "loop", "window"), default="both")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cameras", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    scene = pkg.GaussianScene.from_dict(syn.make_scene(1000, 0), device="cuda")
    cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(a.cameras, 1, width=800, height=800)]
    info = types.SimpleNamespace(train_cameras=cams, test_cameras=cams[:1])
    r = int(pkg.generate_all_possible_rays(scene)[0].shape[0])
    res = {"rays": r, "images_per_iteration": 32, "warmup": a.warmup, "iters": a.iters}
    if a.mode in ("both", "loop"):
        res["loop_it_per_s"] = round(time_mode(False, scene, info, a.warmup, a.iters), 3)
    if a.mode in ("both", "window"):
        res["window_it_per_s"] = round(time_mode(True, scene, info, a.warmup, a.iters), 3)
    if a.mode == "both":
        res["speedup"] = round(res["window_it_per_s"] / res["loop_it_per_s"], 2)
    if a.kernels:
        res["scorer_32_images"] = time_kernels(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
