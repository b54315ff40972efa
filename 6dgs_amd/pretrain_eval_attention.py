"""The evaluation sweep -- drop-in for the reference's entry point pretrain_eval_attention.py:

    python -m sixdgs_amd.pretrain_eval_attention --exp_path <3DGS output dir> --out_path results.json --data_type mip360

for every trained scene under --exp_path (`<prefix>..._<id>/point_cloud/iteration_N/point_cloud.ply` + `cfg_args`):
PLY -> device arrays, cameras of the scene's dataset, train-or-load `id_module.th`, ray emission, the ground-truth-ray pass and the
true inference pass of test_pose_estimation, one results list for all scenes written as JSON (schema test.py:290-302).  Same
function names, arguments and per-scene RuntimeError handling as the reference (pretrain_eval_attention.py:20-248); behind them the
MI355X path of this package.

Multi-GPU (north_star: queries shard over independent test images): started under `torch.distributed.run`, every rank loads the
scene (rank 0 reads the PLY and the checkpoint and broadcasts them over RCCL; ray emission and the key cache are rebuilt locally,
deterministically), takes a contiguous block of the scene's test views, and rank 0 gathers the per-view result dicts in view order
before writing the file.  Training, when no checkpoint exists, runs on rank 0 only and is broadcast.

Beyond the reference (keyword-only / extra flags, defaults reproduce it): --emitter / --max_ellipsoids / --rays_per_ellipsoid select
full-scene emission (every Gaussian) instead of the reference's 1000-ellipsoid subsample; --skip_train evaluates random-init
weights when no checkpoint exists (smoke runs); --n_iterations shortens training; --pose_solver consensus (with --inlier_scale and
--rays_to_output, up to 1024) solves the pose with the consensus solver (ops.solve_pose_consensus) instead of least squares;
--refine_steps N (with --refine_downscale, --refine_lr, --refine_lambda, --refine_backend) refines every estimated pose by render-and-compare
(refine.refine_results) on each rank's block and adds the refined_* and photometric_loss_* keys to its result dicts; the mean and
median errors before and after go to <out_path>.refine_summary.json.  0, the default: no refinement, results.json as without the flag.
--refine_levels "8:30:4e-3,4:30:2e-3,2:40:1e-3" (downscale:steps:lr per level, coarse to fine) refines with that level schedule instead
(refine.refine_poses(levels=...): --refine_steps, --refine_lr and --refine_downscale are not used, and giving --refine_downscale beside
it is an error); off by default.
"""
from __future__ import annotations

import argparse
import json
import os
import traceback
from functools import partial
from typing import Any, List, Optional

import numpy as np
import torch

from . import distributed as dd
from .datasets import dotdict, get_checkpoint_arguments, load_data, parse_exp_dir
from .distance_based_loss import DistanceBasedScoreLoss
from .identification_module import IdentificationModule
from .sampling import generate_all_possible_rays
from .refine import level_plan, parse_levels, refine_results
from .scene import GaussianScene
from .test import test_pose_estimation
from .train import train_id_module

EMISSION = dict(max_ellipsoids=1000, emitter="quadricell", rays_per_ellipsoid=64)      # the reference's emission (sampling.py:145-149,175-196)


def parse_args(argv=None):
    """pose_estimation/opt.py:4-29 (plain argparse: configargparse is not a dependency) + this build's extras."""
    ap = argparse.ArgumentParser(add_help=True)
    ap.add_argument("--exp_path", type=str, required=True, help="experiment directory")
    ap.add_argument("--out_path", type=str, required=True, help="results file (json)")
    ap.add_argument("--data_type", type=str, choices=["blender", "mip360", "tankstemple", "cambridge_landmark", "all"], default="all",
                    help="the type of data to validate")
    ap.add_argument("--emitter", choices=["quadricell", "isocell"], default="quadricell")
    ap.add_argument("--max_ellipsoids", type=int, default=1000, help="ellipsoids that emit rays (1000 = the reference; -1 = every valid Gaussian)")
    ap.add_argument("--rays_per_ellipsoid", type=int, default=64, help="iso-cell emitter only")
    ap.add_argument("--n_iterations", type=int, default=1500, help="training iterations when no id_module.th exists")
    ap.add_argument("--batched_window", action="store_true",
                    help="train each iteration's 32 images as one window (one ray-MLP pass; train_id_module(batched_window=True)) instead of one by one")
    ap.add_argument("--data_parallel_train", action="store_true",
                    help="with --batched_window: every rank trains its block of each window, gradients summed by one all-reduce per iteration "
                         "(train_id_module(data_parallel=True)) instead of rank 0 training alone")
    ap.add_argument("--backward_ray_groups", type=int, default=1,
                    help="split of the scorer's backward over the rays in the window (1 = unsplit, 0 = auto from the CU count)")
    ap.add_argument("--skip_train", action="store_true", help="never train: evaluate the checkpoint, or random-init weights when there is none")
    ap.add_argument("--batch_size", type=int, default=16, help="query images per scorer launch")
    ap.add_argument("--pose_solver", choices=["ls", "consensus"], default="ls",
                    help="ls = the reference's least-squares line intersection; consensus = hypothesise-and-verify over the top-k (tolerates outlier rays)")
    ap.add_argument("--inlier_scale", type=float, default=None,
                    help="consensus solver: inlier scale in scene units (default: 0.01 x the diagonal of the ray origins' bounding box)")
    ap.add_argument("--rays_to_output", type=int, default=100,
                    help="size of the top-k handed to the pose solver (100 = the reference; values above 1024 are capped at 1024; ls takes at most 256)")
    ap.add_argument("--arena_gb", type=float, default=0.0,
                    help="carve the big per-scene buffers (key planes, select workspace, chain workspace) from ONE device buffer of this many GB allocated once "
                         "(ops.Arena) instead of asking the allocator scene by scene: a sweep over scenes of growing size otherwise pays a 100-200 GB hipMalloc "
                         "per scene.  -1: everything free but 56 GB; 0 (default): off")
    ap.add_argument("--refine_steps", type=int, default=0,
                    help="refine each estimated pose by render-and-compare for this many Adam steps (refine.refine_poses); 0 = off")
    downscale_given = []

    class NoteGiven(argparse.Action):                  # the default stays 4 in the namespace; --refine_levels needs to know it was typed
        def __call__(self, parser, namespace, values, option_string=None):
            downscale_given.append(option_string)
            setattr(namespace, self.dest, values)

    ap.add_argument("--refine_downscale", type=int, default=4, action=NoteGiven, help="refinement compares at 1 / this of the query's resolution")
    ap.add_argument("--refine_lr", type=float, default=2e-3, help="Adam step of the refinement")
    ap.add_argument("--refine_lambda", type=float, default=0.2, help="weight of D-SSIM in the refinement's loss (the reference's lambda_dssim)")
    # (absent from the namespace unless given: a command line without it parses to exactly what it did before the flag existed)
    ap.add_argument("--refine_backend", choices=("torch", "fused"), default=argparse.SUPPRESS,
                    help="the refinement's loop: torch (default; autograd and Adam around the kernels) or fused (one library call, sixdgs_refine_poses)")
    ap.add_argument("--refine_levels", type=str, default=argparse.SUPPRESS,
                    help='refine with a coarse-to-fine level schedule, downscale:steps:lr per level, e.g. "8:30:4e-3,4:30:2e-3,2:40:1e-3" '
                         "(refine.refine_poses(levels=...)); excludes --refine_downscale")
    args, rest = ap.parse_known_args(argv)
    if hasattr(args, "refine_levels"):
        if downscale_given:
            ap.error("--refine_levels and --refine_downscale exclude each other")
        try:
            args.refine_levels = parse_levels(args.refine_levels)
            level_plan(args.refine_levels, 1 << 15, 1 << 15)      # everything but the image's size, which each scene brings
        except ValueError as e:
            ap.error(f"--refine_levels: {e}")
    if args.refine_steps < 0:
        ap.error("--refine_steps must be >= 0 (0 = no refinement)")
    if args.refine_downscale < 1:
        ap.error("--refine_downscale must be >= 1")
    if not args.refine_lr > 0:
        ap.error("--refine_lr must be > 0")
    if not 0.0 <= args.refine_lambda <= 1.0:
        ap.error("--refine_lambda must be in [0, 1]")
    if args.data_parallel_train and not args.batched_window:
        ap.error("--data_parallel_train needs --batched_window")
    if args.backward_ray_groups < 0:
        ap.error("--backward_ray_groups must be >= 0 (0 = auto)")
    if args.rays_to_output < 1:
        ap.error("--rays_to_output must be >= 1")
    args.rays_to_output = min(args.rays_to_output, 1024)
    if args.inlier_scale is not None and not args.inlier_scale > 0:
        ap.error("--inlier_scale must be > 0")
    if args.pose_solver == "ls" and args.rays_to_output > 256:
        ap.error("--pose_solver ls takes --rays_to_output <= 256; use --pose_solver consensus beyond")
    if args.pose_solver == "consensus" and args.rays_to_output < 2:
        ap.error("--pose_solver consensus needs --rays_to_output >= 2")
    return args, rest


def load_model(checkpoint_path, device, sh_degrees=3):
    """pretrain_eval_attention.py:20-28: the 3DGS checkpoint as device arrays (no autograd state to switch off here)."""
    return GaussianScene.load_ply(checkpoint_path, sh_degree=sh_degrees, device=device)


def explore_model(model, **emission):
    """pretrain_eval_attention.py:163-169."""
    kw = dict(EMISSION)
    kw.update(emission)
    return generate_all_possible_rays(model, sample_quadricell_targets=50, **kw)


def pretrain_single_object(checkpoint_filepath: str, checkpoint_args: "dotdict[str, Any]", exp_dir_filepath: str, object_id: str, category_name: str,
                           starting_seed: int, lock_backbone: bool = True, device: str = "cuda", *, emission: Optional[dict] = None,
                           n_iterations: int = 1500, skip_train: bool = False, batch_size: int = 16, backbone: Optional[torch.nn.Module] = None,
                           batched_window: bool = False, data_parallel_train: bool = False, backward_ray_groups: int = 1,
                           pose_solver: str = "ls", inlier_scale: Optional[float] = None, rays_to_output: int = 100,
                           refine: Optional[dict] = None):
    """pretrain_eval_attention.py:31-160 for one scene; returns the result dicts of the inference pass for ALL test views (rank 0;
    other ranks return their own block).

    Multi-rank: the scene is walked in STAGES.  A stage is rank-local work that may fail (`dd.agree`: the ranks all-reduce a
    failure flag behind it and leave the scene TOGETHER on a RuntimeError of any of them); the collectives (scene / weight
    broadcast, seed, result gather) sit between the stages, where every rank is known to arrive.  Rank 0 trains a missing
    checkpoint inside a stage while the others wait in that stage's all-reduce (on the group with the long timeout: agree(long_wait=True),
    distributed.init_from_env).  data_parallel_train: every rank takes part in the training (train_id_module(data_parallel=True)), inside
    the same stage; the ranks of a failing iteration leave it together.

    pose_solver / inlier_scale / rays_to_output: handed to both passes of test_pose_estimation.  refine: the keyword arguments of
    refine.refine_poses (steps, lr, lambda_dssim, downscale, backend); when given, each rank refines the poses of its block after the inference
    pass (refine.refine_results).  None: no refinement."""
    solver = dict(pose_solver=pose_solver, inlier_scale=inlier_scale, rays_to_output=rays_to_output)
    torch.manual_seed(starting_seed)
    print("data_path: ", checkpoint_args.source_path)
    emission = dict(EMISSION, **(emission or {}))
    ckpt_path = os.path.join(exp_dir_filepath, "id_module.th")

    def stage_load():
        scene = load_model(checkpoint_filepath, device, sh_degrees=checkpoint_args.sh_degree if checkpoint_args.sh_degree is not None else 3) \
            if dd.rank() == 0 else None
        if checkpoint_args.fps_sampling is None:
            checkpoint_args.fps_sampling = -1
        info = load_data(checkpoint_args)
        module = IdentificationModule(backbone_type="dino", backbone=backbone).to(device).train()
        start = 0
        if os.path.exists(ckpt_path):
            print("Checkpoint already exist, skip training phase")
            ckpt = torch.load(ckpt_path, map_location=device)
            module.load_state_dict(ckpt["model_state_dict"])
            start = ckpt["epoch"]
        return scene, info, module, start

    scene, scene_info, id_module, start_iterations = dd.agree(stage_load, "load scene, cameras and checkpoint", device)
    gs_model = dd.broadcast_scene(scene, 0, device=device)

    def stage_train():
        if not skip_train and start_iterations < n_iterations and (dd.rank() == 0 or data_parallel_train):
            train_id_module(ckpt_path, device, id_module, partial(explore_model, gs_model, **emission), scene_info, object_id, category_name,
                            start_iterations=start_iterations, lock_backbone=lock_backbone, n_iterations=n_iterations,
                            batched_window=batched_window, data_parallel=data_parallel_train, backward_ray_groups=backward_ray_groups)

    dd.agree(stage_train, "train the scorer (every rank)" if data_parallel_train else "train the scorer (rank 0)", device, long_wait=True)
    dd.broadcast_module(id_module, 0)
    id_module.eval()
    id_module.invalidate_caches()
    print("Training complete starting testing phase...")
    if dd.is_dist():         # every rank must emit the SAME rays (the subsample is a torch.randperm): one seed from rank 0's generator
        torch.manual_seed(dd.broadcast_int(int(torch.randint(0, 2**31 - 1, (1,)).item()), 0, device))
    lo, hi = dd.shard_range(len(scene_info.test_cameras), dd.rank(), dd.world())

    def stage_evaluate():
        rays_ori, rays_dirs, rays_rgb = explore_model(gs_model, **emission)
        model_up = torch.from_numpy(np.mean(np.asarray([c.R[:3, 1] for c in scene_info.train_cameras], dtype=np.float32), axis=0)).to(device)
        mine = scene_info.test_cameras[lo:hi]
        print("Testing overfit performances...")
        _, o_t, o_a, o_s, o_r = test_pose_estimation(mine, id_module, rays_ori, rays_dirs, rays_rgb, model_up, sequence_id=object_id,
                                                     category_id=category_name, loss_fn=DistanceBasedScoreLoss(), batch_size=batch_size, **solver)
        print("Overfit AVG translation error: ", o_t)
        print("Overfit AVG angular error: ", o_a)
        print("Overfit AVG score error: ", o_s)
        print("Overfit recall: ", o_r)
        print("Testing performances on same points...")
        results, t_t, t_a, t_s, t_r = test_pose_estimation(mine, id_module, rays_ori, rays_dirs, rays_rgb, model_up, sequence_id=object_id,
                                                           category_id=category_name, save=False, save_all=False, batch_size=batch_size, **solver)
        if refine:
            print("Refining the estimated poses...")
            try:
                refine_results(gs_model, mine, results, **refine)
            except RuntimeError:        # an optional post-pass: the unrefined rows stay (entries refined before the error keep their new keys)
                traceback.print_exc()
        for r in results:
            r["frame_id"] += lo                  # frame ids count the scene's test views, not the rank's block
        print("Test AVG translation error: ", t_t)
        print("Test AVG angular error: ", t_a)
        print("Test AVG score error: ", t_s)
        print("Test recall: ", t_r)
        return results

    results = dd.agree(stage_evaluate, "emit rays and evaluate the test views", device)
    return dd.gather_results(results, 0)


def evaluate_single_object_in_blender(checkpoint_filepath: str, checkpoint_args, exp_dir_filepath: str, object_id: str, category_name: str,
                                      starting_seed: int = 55176280, device: str = "cuda", lock_backbone: bool = True, **extras):
    """pretrain_eval_attention.py:172-197."""
    return pretrain_single_object(checkpoint_filepath, checkpoint_args, exp_dir_filepath, object_id, category_name, starting_seed,
                                  device=device, lock_backbone=lock_backbone, **extras)


def refine_summary(results: List[dict]) -> dict:
    """Mean and median of the errors before and after refinement over the refined views, the unrefined ones from the same poses
    (refine.pose_errors on pred_c2w), under key names of their own."""
    from .refine import pose_errors

    done = [r for r in results if "refined_c2w" in r]
    out = {"refined_views": len(done), "views": len(results)}
    if done:
        t0, a0 = pose_errors(torch.tensor([r["gt_c2w"] for r in done]), torch.tensor([r["pred_c2w"] for r in done]))
        cols = {"translation_error": t0.numpy(), "angular_error": a0.numpy(),
                "refined_translation_error": np.array([r["refined_translation_error"] for r in done]),
                "refined_angular_error": np.array([r["refined_angular_error"] for r in done]),
                "photometric_loss_before": np.array([r["photometric_loss_before"] for r in done]),
                "photometric_loss_after": np.array([r["photometric_loss_after"] for r in done])}
        for k, v in cols.items():
            out["mean_" + k], out["median_" + k] = float(np.nanmean(v)), float(np.nanmedian(v))
    return out


PREFIXES = {"blender": "synthetic_", "mip360": "mip_360_", "tankstemple": "tt_", "cambridge_landmark": "cl_"}


def main(argv=None, backbone: Optional[torch.nn.Module] = None) -> List[dict]:
    args, _ = parse_args(argv)
    forced = os.environ.get("SIXDGS_FORCE_DEVICE")            # test hook: several ranks on one GPU (gloo)
    rank, world, local = dd.init_from_env(set_device=forced is None)
    if forced is not None:
        local = int(forced)
    out_path_abs = os.path.abspath(args.out_path)
    if rank == 0:
        os.makedirs(os.path.dirname(out_path_abs), exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("6dgs_amd: the evaluation sweep needs an MI355X (no CPU fallback on the product path)")
    device = f"cuda:{local}"
    torch.cuda.set_device(local)
    dd.warm_long_wait_group(torch.device(device))          # (exists already unless init_from_env left it to us: nccl with a forced device)
    if dd.is_dist():
        seen = dd.ranks_seen(torch.device(device))          # a collective: every rank takes part, rank 0 reports
        if rank == 0:
            print(f"[6dgs_amd] evaluation sweep over {seen} rank(s), backend {dd.backend_name()}")
    results: List[dict] = []
    arena = None
    if args.arena_gb:
        from . import ops
        free_b = torch.cuda.mem_get_info(torch.device(device))[0]
        want = int(free_b - (56 << 30)) if args.arena_gb < 0 else int(args.arena_gb * (1 << 30))
        arena = ops.Arena(max(1 << 28, min(want, int(0.95 * free_b))), torch.device(device))
        ops.set_arena(arena)
        if rank == 0:
            print(f"[6dgs_amd] arena of {arena.capacity / 2**30:.1f} GiB for the per-scene buffers")
    for exp in parse_exp_dir(args.exp_path, PREFIXES.get(args.data_type, "")).values():
        ckpt_args = get_checkpoint_arguments(exp["exp_dir_filepath"])
        try:
            obj = evaluate_single_object_in_blender(
                exp["checkpoint_filepath"], ckpt_args, exp["exp_dir_filepath"], exp["sequence_id"], exp["category_name"], starting_seed=55176280,
                device=device, lock_backbone=True,
                emission=dict(emitter=args.emitter, max_ellipsoids=args.max_ellipsoids, rays_per_ellipsoid=args.rays_per_ellipsoid),
                n_iterations=args.n_iterations, skip_train=args.skip_train, batch_size=args.batch_size, backbone=backbone,
                batched_window=args.batched_window, data_parallel_train=args.data_parallel_train,
                backward_ray_groups=args.backward_ray_groups, pose_solver=args.pose_solver, inlier_scale=args.inlier_scale,
                rays_to_output=args.rays_to_output,
                refine=dict(levels=args.refine_levels, lambda_dssim=args.refine_lambda, backend=getattr(args, "refine_backend", "torch"))
                if hasattr(args, "refine_levels") else
                dict(steps=args.refine_steps, lr=args.refine_lr, lambda_dssim=args.refine_lambda, downscale=args.refine_downscale,
                     backend=getattr(args, "refine_backend", "torch"))
                if args.refine_steps > 0 else None)
            if rank == 0:
                results.extend(obj)
        except RuntimeError:            # the only exception the reference survives per scene (pretrain_eval_attention.py:243-244)
            traceback.print_exc()
    if arena is not None:
        from . import ops
        ops.set_arena(None)
    if rank == 0:
        print("Saving results")
        with open(out_path_abs, "w") as fh:
            json.dump(results, fh)
        if args.refine_steps > 0 or hasattr(args, "refine_levels"):
            with open(out_path_abs + ".refine_summary.json", "w") as fh:
                json.dump(refine_summary(results), fh)
    dd.barrier()
    return results


if __name__ == "__main__":
    torch.manual_seed(71170)
    main()
