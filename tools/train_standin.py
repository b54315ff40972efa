"""Train the scorer on rendered views of a stand-in scene and look at the inference path on the trained weights.

    python tools/train_standin.py [--gaussians 5000] [--iterations 1500] [--size 224] [--renderer disc|raster] [--out profiles/trained_standin.md]

Builds synthetic.make_scene, renders training and held-out views with render_views (6dgs_amd/render.py), records the per-view pose
errors of test_pose_estimation with the initial weights, trains with train_id_module(batched_window=True) on the reference's schedule
(1500 iterations x 32 images, rays renewed every 10), records the errors again, and on the trained weights: the select path's statuses
and candidate counts, select / two-pass / CPU checker agreement (top-100 under the tie policy of tests/test_gpu_configs.py, scores,
pose), how peaked the softmax became, and the time of render_views at 500 k Gaussians / 800 x 800.  Everything goes to the output
file together with the command line; a number that was not measured is not written.  tests/test_gpu_trained_scorer.py uses the
functions below for a shorter run.

--pose-solver both: on the trained weights, additionally, least squares (k = 100) against the consensus solver (k = 100, 256, 1024) on the
training and the held-out views -- median errors, the distribution of `support` and `n_inliers`, and both solvers' GPU time per batch of 8
images from HIP events -- written to --consensus-out (profiles/pose_consensus.md)."""
import argparse
import functools
import importlib
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")       # no DINOv2 weights offline: a random-init ViT-S/14, as in the tests

SCORE_TOL = 1e-5          # max |score - checker| / max checker score
POSE_TOL = 1e-4
MARGIN = 8e-6             # top-100 membership margin, relative to the largest score (tests/test_gpu_configs.py)


def modules():
    return (importlib.import_module("6dgs_amd"), importlib.import_module("6dgs_amd.synthetic"), importlib.import_module("6dgs_amd.ops"),
            importlib.import_module("6dgs_amd.test"))


def fresh_scorer(seed: int = 0):
    pkg, syn, _, _ = modules()
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(seed, with_cnn=True).items()}, strict=False)
    return idm.cuda()


def build_standin(n_gauss: int, seed: int, n_train: int, n_held: int, size: int, extent: float = 1.0, renderer: str = "disc"):
    """-> (GaussianScene, rendered training views, rendered held-out views): cameras of make_cameras with different seeds."""
    pkg, syn, _, _ = modules()
    scene = pkg.GaussianScene.from_dict(syn.make_scene(n_gauss, seed), device="cuda")
    train = pkg.render_views(scene, syn.make_cameras(n_train, seed + 100, width=size, height=size), extent=extent, renderer=renderer)
    held = pkg.render_views(scene, syn.make_cameras(n_held, seed + 200, width=size, height=size), extent=extent, renderer=renderer)
    return scene, train, held


def model_up_of(cams, device="cuda"):
    return torch.from_numpy(np.mean(np.asarray([c.R[:3, 1] for c in cams], dtype=np.float32), axis=0)).to(device)


def pose_errors(idm, cams, rays, model_up):
    """Per view: translation error (camera centre), rotation error in degrees, and whether the pose is unusable (NaN or the identity
    test_pose_estimation returns after a singular solve)."""
    pkg, _, _, _ = modules()
    results, *_ = pkg.test_pose_estimation(cams, idm, *rays, model_up, verbose=False)
    t_err, r_err, bad = [], [], []
    for res in results:
        pred, gt = np.asarray(res["pred_c2w"], np.float64), np.asarray(res["gt_c2w"], np.float64)
        unusable = (not np.isfinite(pred).all()) or np.array_equal(pred, np.eye(4))
        bad.append(bool(unusable))
        t_err.append(float(np.linalg.norm(pred[:3, 3] - gt[:3, 3])) if np.isfinite(pred).all() else float("nan"))
        cos = (np.trace(pred[:3, :3].T @ gt[:3, :3]) - 1) / 2 if np.isfinite(pred).all() else float("nan")
        r_err.append(float(np.degrees(np.arccos(np.clip(cos, -1, 1)))))
    return np.array(t_err), np.array(r_err), np.array(bad)


def train(idm, scene, train_cams, held_cams, ckpt, iterations: int, accumulation: int = 32, renewal: int = 10):
    """train_id_module(batched_window=True) without the periodic evaluation -> the logged train/loss_score per iteration."""
    pkg, _, _, _ = modules()
    info = types.SimpleNamespace(train_cameras=list(train_cams), test_cameras=list(held_cams))
    logged = []
    pkg.train_id_module(ckpt, "cuda", idm, functools.partial(pkg.generate_all_possible_rays, scene), info, "standin", "synthetic",
                        n_iterations=iterations, gradient_accumulation_steps=accumulation, renewal_every_n_iterations=renewal,
                        display_every_n_iterations=max(iterations, 1) + 1, val_every_n_iterations=max(iterations, 1) + 1,
                        log_fn=lambda tag, v, it: logged.append(v) if tag == "train/loss_score" else None, batched_window=True)
    idm.eval()
    return logged


def improved_views(before, after, bad_after):
    """Views whose translation error fell; an unusable pose after training is not an improvement."""
    return int(np.sum((after < before) & ~bad_after & np.isfinite(after)))


@torch.no_grad()
def image_side(idm, cams):
    """-> (tokens as a list of [T,398] tensors, camera-up [B,3]) for rendered views."""
    _, _, _, T = modules()
    imgs = [torch.from_numpy(np.ascontiguousarray(c.image)).cuda() for c in cams]
    tokens, fmaps = T.image_side_tokens(idm, imgs)
    return [tokens[i] for i in range(len(cams))], idm.camera_up(fmaps)


@torch.no_grad()
def peakedness(idm, toks, rays):
    """Per image: the range of the logits q.k / sqrt(384) and the largest softmax mass one token puts on one ray."""
    key = idm.ray_keys(*rays)
    q, _, n_host = idm._tokens_to_q(toks, rays[0].device)
    out = []
    for b, n in enumerate(n_host):
        logits = (q[b, :n] @ key.t()) / math.sqrt(key.shape[1])
        out.append((float(logits.max() - logits.min()), float(torch.softmax(logits, dim=-1).max())))
    return out


@torch.no_grad()
def trained_parity(idm, cams, rays, checker, k: int = 100):
    """Select path, two-pass scorer and the CPU checker on the module's current weights, per view.  The rays may be fewer than
    ops.SELECT_MIN_RAYS (a 1000-ellipsoid emission): the threshold is lowered for the call, as tests/test_gpu_select_contract.py does.
    -> list of per-view dicts (status, ok flags, errors) -- nothing is asserted here."""
    _, _, ops, _ = modules()
    o, d, c = rays
    toks, up = image_side(idm, cams)
    old = ops.SELECT_MIN_RAYS
    try:
        ops.SELECT_MIN_RAYS = min(old, 4096)
        idm.invalidate_caches()
        i_s, v_s, none = idm.score_tokens(toks, o, d, c, k, want_scores=False)
        path = idm.last_scoring_path
        assert none is None and path.startswith("select"), path
        status = list(idm.last_select_candidates)
    finally:
        ops.SELECT_MIN_RAYS = old
    i_t, v_t, sc = idm.score_tokens(toks, o, d, c, k, want_scores=True)
    assert idm.last_scoring_path == "two-pass"
    p_s = ops.solve_pose(o, d, i_s, v_s, up)["c2w"].cpu().numpy()
    p_t = ops.solve_pose(o, d, i_t, v_t, up)["c2w"].cpu().numpy()
    sd = {name: v.detach().cpu().numpy() for name, v in idm.state_dict().items()}
    on, dn, cn = o.cpu().numpy(), d.cpu().numpy(), c.cpu().numpy()
    _, key = checker.ray_features(on, dn, cn, sd)
    peaks = peakedness(idm, toks, rays)
    rows = []
    for b in range(len(cams)):
        s_ref = checker.attention_scores(checker.q_proj(toks[b].cpu().numpy(), sd), key)
        smax = float(s_ref.max())
        order = np.argsort(-s_ref, kind="stable")
        s_k, s_next = float(s_ref[order[k - 1]]), float(s_ref[order[k]])
        must = set(order[:k][s_ref[order[:k]] - s_next > MARGIN * smax].tolist())
        row = dict(status=int(status[b]), gap_at_cut=(s_k - s_next) / smax, logit_range=peaks[b][0], softmax_peak=peaks[b][1],
                   score_err=float(np.abs(sc[b].cpu().numpy().astype(np.float64) - s_ref).max() / smax))
        up_b = up[b].cpu().numpy()
        for name, idx, val, pose in (("select", i_s[b], v_s[b], p_s[b]), ("two_pass", i_t[b], v_t[b], p_t[b])):
            got = idx.cpu().numpy().astype(np.int64)
            members = set(got.tolist())
            row[name + "_top_ok"] = bool(len(members) == k and must <= members and float(s_ref[got].min()) >= s_k - MARGIN * smax)
            row[name + "_identical"] = members == set(order[:k].tolist())
            row[name + "_value_err"] = float(np.abs(val.cpu().numpy().astype(np.float64) - s_ref[got]).max() / smax)
            # the checker's pose from ITS top-k where the lists agree, else from its scores of the returned rays (a swap inside the margin)
            ref_idx = order[:k] if row[name + "_identical"] else got
            p_ref = checker.pose_from_topk(on, dn, ref_idx, s_ref[ref_idx].astype(np.float32), up_b)["c2w"]
            same_nan = np.array_equal(np.isnan(pose), np.isnan(p_ref))
            row[name + "_pose_err"] = float(np.nanmax(np.abs(pose - p_ref))) if same_nan and np.isfinite(pose).any() else (0.0 if same_nan else float("inf"))
        row["select_equals_two_pass"] = set(i_s[b].tolist()) == set(i_t[b].tolist())
        rows.append(row)
    return rows


@torch.no_grad()
def time_render(n_gauss: int = 500_000, size: int = 800, views: int = 4, repeats: int = 5):
    """HIP-event time of ops.splat_views per view at full size (device work only: no host copy of the images)."""
    pkg, syn, ops, _ = modules()
    render = importlib.import_module("6dgs_amd.render")
    scene = pkg.GaussianScene.from_dict(syn.make_scene(n_gauss, 0), device="cuda")
    cams = torch.from_numpy(render.camera_rows(syn.make_cameras(views, 21, width=size, height=size))).cuda()
    args = (scene._xyz, scene._scaling, scene._features_dc, scene._features_rest, scene.active_sh_degree, cams, size, size)
    ws = torch.empty(ops.splat_views_workspace_bytes(n_gauss, views, size, size), dtype=torch.uint8, device="cuda")
    ops.splat_views(*args, workspace=ws)
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.splat_views(*args, workspace=ws)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / views)
    return float(np.median(times)), float(min(times)), float(max(times))


CONSENSUS_KS = (100, 256, 1024)


@torch.no_grad()
def solver_comparison(idm, cams, rays, batch: int = 8):
    """Per view of `cams`: least squares at k = 100 and consensus at CONSENSUS_KS on the module's current weights, one scorer pass per k.
    -> {(solver, k): dict(t=[..], r=[..], bad=[..], support=[..], n_inliers=[..])}, errors as the solvers report them against the view's pose."""
    _, _, ops, T = modules()
    o, d, c = rays
    tau = T.default_inlier_scale(idm, o)
    out = {}
    for b0 in range(0, len(cams), batch):
        part = cams[b0:b0 + batch]
        toks, up = image_side(idm, part)
        gt = torch.stack([T.gt_pose_and_intrinsics(cam, "cpu")[0] for cam in part]).cuda()
        for k in CONSENSUS_KS:
            idx, val, _ = idm.score_tokens(toks, o, d, c, k, want_scores=False)
            sols = [("consensus", ops.solve_pose_consensus(o, d, idx, val, up, gt, inlier_scale=tau))]
            if k == 100:
                sols.append(("ls", ops.solve_pose(o, d, idx, val, up, gt)))
            for name, sol in sols:
                row = out.setdefault((name, k), dict(t=[], r=[], bad=[], support=[], n_inliers=[]))
                st = sol["status"].cpu().numpy()
                err = sol["errors"].cpu().numpy().astype(np.float64)
                row["bad"] += ((st & 6) != 0).tolist()
                row["t"] += np.where((st & 6) != 0, np.nan, err[:, 0]).tolist()
                row["r"] += np.where((st & 6) != 0, np.nan, err[:, 1]).tolist()
                if name == "consensus":
                    row["support"] += sol["support"].cpu().tolist()
                    row["n_inliers"] += sol["n_inliers"].cpu().tolist()
    return out, tau


@torch.no_grad()
def time_solvers(idm, cams, rays, repeats: int = 20):
    """GPU time of one solver call on a batch of 8 images (HIP events around the call: both kernels of the consensus solver, the one of least
    squares), median / min / max over `repeats` calls after a warm-up.  -> {(solver, k): (median, min, max) in microseconds}."""
    _, _, ops, T = modules()
    o, d, c = rays
    tau = T.default_inlier_scale(idm, o)
    toks, up = image_side(idm, cams[:8])
    out = {}
    for k in CONSENSUS_KS:
        idx, val, _ = idm.score_tokens(toks, o, d, c, k, want_scores=False)
        calls = [("consensus", lambda: ops.solve_pose_consensus(o, d, idx, val, up, inlier_scale=tau))]
        if k <= ops.SOLVE_POSE_MAX_K:
            calls.append(("ls", lambda: ops.solve_pose(o, d, idx, val, up)))
        for name, fn in calls:
            fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            out[(name, k)] = (float(np.median(times)), float(min(times)), float(max(times)))
    return out


def _quantiles(a):
    a = np.asarray(a, np.float64)
    return "min {:.3g}, quartiles {:.3g} / {:.3g} / {:.3g}, max {:.3g}".format(a.min(), *np.percentile(a, [25, 50, 75]), a.max())


def consensus_report(args, cmd, comparison, tau, timing, rays_n, extra=None):
    L = ["# Consensus pose solver: measurements", "",
         f"Command: `{cmd}`", "",
         f"Scene, views, training and emission as in `profiles/trained_standin.md` (`make_scene({args.gaussians}, {args.seed})`, {args.train_views} training and "
         f"{args.held_views} held-out rendered views, {args.iterations} iterations; {rays_n} rays).  Inlier scale: the default, 0.01 x the diagonal of the ray "
         f"origins' bounding box = {tau:.4g} scene units; uniform prior.", "",
         "## Least squares against consensus on the trained stand-in weights", "",
         "Errors as the solvers report them against each view's pose (translation = camera centre, scene units; rotation in degrees); median over the views; "
         "a view whose pose came back NaN / identity counts as unusable and is left out of the medians.", "",
         "| views | solver | k | translation | rotation | unusable |", "|---|---|---|---|---|---|"]
    for split in ("train", "held"):
        for key in [("ls", 100)] + [("consensus", k) for k in CONSENSUS_KS]:
            row = comparison[split][key]
            L.append(f"| {split} ({len(row['t'])}) | {'least squares' if key[0] == 'ls' else 'consensus'} | {key[1]} | {_med(row['t']):.4f} | {_med(row['r']):.2f} | {int(np.sum(row['bad']))} |")
    L += ["", "Distribution of the consensus solver's confidence outputs over the views:", ""]
    for split in ("train", "held"):
        for k in CONSENSUS_KS:
            row = comparison[split][("consensus", k)]
            L.append(f"* {split}, k = {k}: `support` {_quantiles(row['support'])}; `n_inliers` {_quantiles(row['n_inliers'])}")
    L += ["", "## Solver time per batch of 8 images", "",
          "HIP events around one call (`k_consensus_sweep` + `k_consensus_finish`; `k_solve_pose` for least squares), same process, same box, median (min - max) of 20 calls:", "",
          "| solver | k | microseconds |", "|---|---|---|"]
    for key in sorted(timing, key=lambda x: (x[1], x[0])):
        med, lo, hi = timing[key]
        L.append(f"| {'least squares' if key[0] == 'ls' else 'consensus'} | {key[1]} | {med:.0f} ({lo:.0f} - {hi:.0f}) |")
    if extra:
        L += ["", extra.rstrip()]
    L.append("")
    return "\n".join(L)


def _med(a):
    a = np.asarray(a, np.float64)
    return float(np.nanmedian(a)) if np.isfinite(a).any() else float("nan")


def report(args, cmd, loss, errs, parity, render_ms, seconds, test_seconds=None):
    L = ["# Scorer trained on rendered views of a stand-in scene", "",
         f"Command: `{cmd}`", "",
         f"Inputs: `make_scene({args.gaussians}, {args.seed})`, {args.train_views} training and {args.held_views} held-out views of "
         f"`make_cameras` (seeds {args.seed + 100} / {args.seed + 200}, {args.size} x {args.size}, FoV 0.8) rendered by `render_views` "
         f"(renderer {args.renderer!r}, extent {args.extent}); random-init ViT-S/14 (`SIXDGS_RANDOM_BACKBONE=1`), scorer initialised from `make_scorer_state_dict(0, with_cnn=True)`; "
         f"`train_id_module(batched_window=True)`, {args.iterations} iterations x {args.accumulation} images, rays renewed every {args.renewal} "
         f"(1000-ellipsoid emission).  Pose errors: `test_pose_estimation` on one fixed emission ({errs['rays']} rays), the same before and after.", "",
         "## Training", "",
         f"* `train/loss_score`, mean of the first 20 iterations: {np.mean(loss[:20]):.6g}; of the last 20: {np.mean(loss[-20:]):.6g}",
         f"* training took {seconds['train']:.1f} s ({args.iterations / max(seconds['train'], 1e-9):.1f} iterations/s)", "",
         "## Pose errors per view (median over the views; translation = camera centre, scene units; rotation in degrees)", "",
         "| views | weights | translation | rotation | unusable poses (NaN / identity) |", "|---|---|---|---|---|"]
    for split in ("train", "held"):
        for when in ("before", "after"):
            t, r, bad = errs[split][when]
            L.append(f"| {split} ({len(t)}) | {'initial' if when == 'before' else 'trained'} | {_med(t):.4f} | {_med(r):.2f} | {int(bad.sum())} |")
    for split in ("train", "held"):
        n_imp = improved_views(errs[split]["before"][0], errs[split]["after"][0], errs[split]["after"][2])
        L.append("")
        L.append(f"Views whose translation error fell with training, {split}: **{n_imp} of {len(errs[split]['before'][0])}**")
    st = [r["status"] for r in parity]
    L += ["", f"## Inference path on the trained weights ({len(parity)} held-out views, {errs['rays']} rays, top-100, `SELECT_MIN_RAYS` lowered to 4096 for the call)", "",
          f"* select statuses (candidates examined per image; -1 = refused, re-done by the two-pass scorer): {st}",
          f"* -1 fallbacks: {sum(1 for s in st if s < 0)} of {len(st)}; candidate counts of the others: min {min([s for s in st if s >= 0] or [0])}, "
          f"median {int(np.median([s for s in st if s >= 0] or [0]))}, max {max([s for s in st if s >= 0] or [0])}",
          f"* top-100 against the CPU checker under the tie policy (MARGIN = {MARGIN:g}): select {sum(r['select_top_ok'] for r in parity)} / {len(parity)} ok "
          f"({sum(r['select_identical'] for r in parity)} lists identical), two-pass {sum(r['two_pass_top_ok'] for r in parity)} / {len(parity)} ok "
          f"({sum(r['two_pass_identical'] for r in parity)} identical); select and two-pass return the same set on {sum(r['select_equals_two_pass'] for r in parity)} / {len(parity)}",
          f"* smallest relative gap between the checker's 100th and 101st score: {min(r['gap_at_cut'] for r in parity):.3g}",
          f"* largest score difference to the checker (two-pass score vector, relative to the largest score): {max(r['score_err'] for r in parity):.3g} (bar {SCORE_TOL:g}); "
          f"top-100 values: select {max(r['select_value_err'] for r in parity):.3g}, two-pass {max(r['two_pass_value_err'] for r in parity):.3g}",
          f"* largest pose difference to the checker: select {max(r['select_pose_err'] for r in parity):.3g}, two-pass {max(r['two_pass_pose_err'] for r in parity):.3g} (bar {POSE_TOL:g})",
          f"* logit range per image: min {min(r['logit_range'] for r in parity):.3g}, max {max(r['logit_range'] for r in parity):.3g}; largest softmax mass of one token on one ray: "
          f"{max(r['softmax_peak'] for r in parity):.3g} (uniform would be {1.0 / errs['rays']:.3g})"]
    if "parity_initial" in errs:
        pi = errs["parity_initial"]
        L.append(f"* the same with the INITIAL weights, for comparison: statuses {[r['status'] for r in pi]}, logit range max {max(r['logit_range'] for r in pi):.3g}, "
                 f"largest softmax mass {max(r['softmax_peak'] for r in pi):.3g}")
    if render_ms is not None:
        L += ["", "## render_views at full size", "",
              f"`ops.splat_views`, 500 000 Gaussians (`make_scene(500000, 0)`), 800 x 800, 4 views per launch, HIP events, device work only: "
              f"median {render_ms[0]:.2f} ms per view (min {render_ms[1]:.2f}, max {render_ms[2]:.2f} over 5 launches)"]
    if test_seconds:
        L += ["", "## Duration of the new GPU tests", "", test_seconds]
    L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--train-views", type=int, default=50)
    ap.add_argument("--held-views", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--extent", type=float, default=1.0)
    ap.add_argument("--renderer", choices=["disc", "raster"], default="disc",
                    help="disc: z-buffered flat discs (ops.splat_views); raster: the alpha-blended 3DGS rasteriser (ops.raster_views)")
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--accumulation", type=int, default=32)
    ap.add_argument("--renewal", type=int, default=10)
    ap.add_argument("--no-render-timing", action="store_true")
    ap.add_argument("--test-durations", default=None, help="a line on the measured duration of the new GPU tests, copied into the report")
    ap.add_argument("--ckpt", default="id_module.th", help="where the trained checkpoint is written (default: the current directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trained_standin.md"))
    ap.add_argument("--pose-solver", choices=["ls", "both"], default="ls",
                    help="both: also compare least squares with the consensus solver on the trained weights and time them (see --consensus-out)")
    ap.add_argument("--consensus-out", default=os.path.join(ROOT, "profiles", "pose_consensus.md"))
    ap.add_argument("--consensus-extra", default=None, help="a markdown file appended to the consensus report (figures collected elsewhere)")
    args = ap.parse_args()
    from oracle import oracle as checker
    checker.build()
    pkg, _, _, _ = modules()
    torch.manual_seed(0)
    scene, train_cams, held_cams = build_standin(args.gaussians, args.seed, args.train_views, args.held_views, args.size, args.extent, args.renderer)
    idm = fresh_scorer().eval()
    rays = pkg.generate_all_possible_rays(scene)
    up = model_up_of(train_cams)
    errs = {"rays": int(rays[0].shape[0]), "train": {}, "held": {}}
    errs["train"]["before"], errs["held"]["before"] = pose_errors(idm, train_cams, rays, up), pose_errors(idm, held_cams, rays, up)
    errs["parity_initial"] = trained_parity(idm, held_cams, rays, checker)
    os.makedirs(os.path.dirname(os.path.abspath(args.ckpt)), exist_ok=True)
    t0 = time.time()
    loss = train(idm, scene, train_cams, held_cams, args.ckpt, args.iterations, args.accumulation, args.renewal)
    torch.cuda.synchronize()
    seconds = {"train": time.time() - t0}
    errs["train"]["after"], errs["held"]["after"] = pose_errors(idm, train_cams, rays, up), pose_errors(idm, held_cams, rays, up)
    parity = trained_parity(idm, held_cams, rays, checker)
    if args.pose_solver == "both":
        comparison = {}
        comparison["train"], tau = solver_comparison(idm, list(train_cams), rays)
        comparison["held"], _ = solver_comparison(idm, list(held_cams), rays)
        timing = time_solvers(idm, list(held_cams), rays)
        extra = open(args.consensus_extra).read() if args.consensus_extra else None
        ctext = consensus_report(args, "python tools/train_standin.py " + " ".join(sys.argv[1:]), comparison, tau, timing, errs["rays"], extra)
        os.makedirs(os.path.dirname(os.path.abspath(args.consensus_out)), exist_ok=True)
        with open(args.consensus_out, "w") as f:
            f.write(ctext)
        print(ctext)
    render_ms = None if args.no_render_timing else time_render()
    text = report(args, "python tools/train_standin.py " + " ".join(sys.argv[1:]), loss, errs, parity, render_ms, seconds, args.test_durations)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
