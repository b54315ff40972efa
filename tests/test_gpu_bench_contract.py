"""bench.py contract on the GPU box: one JSON line with the required keys (small scene so it runs in seconds), and the
N > 1 code path (scene broadcast, weight broadcast, image sharding, pose gather, max-over-ranks timing) with two ranks
sharing the one GPU over gloo -- the driver runs the same path over RCCL at 2/4/8 GPUs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline"}


def _run_eight(cmd, env, timeout):
    """Eight processes sharing ONE GPU (gloo between them).  Round 5 saw one such run in ~8 abort and repeated it once; round 6 found the abort to be the HSA
    runtime's queue-error callback -- HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION raised by the GPU inside a stock PyTorch copy kernel of a WORKING rank, 1 run in
    40 -- under eight processes x four hardware queues on one device (profiles/r06_eight_ranks_sigabrt.md).  The launchers now give every rank ONE hardware
    queue when ranks are forced onto one device (GPU_MAX_HW_QUEUES=1: 40 of 40 runs clean), and the retry is gone: a run that dies fails the test."""
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _run(cmd, env=None, timeout=400):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-1000:]
    return json.loads(lines[0])


@pytest.mark.timeout(500)
def test_bench_single_gpu_json_contract():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _run([sys.executable, "-W", "ignore", "bench.py", "--gaussians", "8000", "--steps", "2", "--warmup", "1", "--cpu-sample-rays", "100000", "--full"])
    assert REQUIRED <= set(d) and "cpu_baseline" in d
    assert d["metric"] == "poses/sec" and d["unit"] == "poses/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["value"] > 0 and abs(d["value"] - 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-2 * d["value"]      # 8 images per GPU and step since round 6
    assert d["config"]["images_per_gpu_per_step"] == 8
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["launches"] >= 2 and r["avg_launch_ms"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["ranks_seen"] == 1 and d["median_step"]["n"] == 2 and d["config"]["preset"] == "headline"
    # the second half of BASELINE.json's metric ("mean rot/trans err") and the parity of the run, from the line alone
    p = d["parity_vs_oracle"]
    assert "error" not in p, p
    assert p["sample_rays"] == 100000 and p["top100_identical"] is True and p["score_rel_err"] < 1e-5
    assert p["two_pass"]["value_rel_err"] < 1e-5 and p["select"]["value_rel_err"] < 1e-5 and p["select"]["top100_identical"] is True
    assert p["ray_mlp_keys"]["max_row_rel_err"] < 5e-6 and p["ray_mlp_keys"]["rays"] > 0 and "every 5-th ray" in p["sample"]      # round 4: strided sample, the oracle's own keys
    assert p["rot_err_deg"] < 1e-2 and p["trans_err"] < 1e-4 * max(1.0, abs(p["pose"]["vs_synthetic_gt"]["oracle"]["trans_err"]))
    g = p["pose"]["vs_synthetic_gt"]
    assert abs(g["hip"]["rot_err_deg"] - g["oracle"]["rot_err_deg"]) < 1e-2 and abs(g["hip"]["trans_err"] - g["oracle"]["trans_err"]) < 1e-3
    assert d["metric_errors"]["mean_rot_err_deg_vs_reference_outputs"] == p["rot_err_deg"] and "errors_vs_synthetic_gt" not in d
    assert d["reference_mode"]["value"] > 0 and 20000 < d["reference_mode"]["rays"] < 40000


@pytest.mark.timeout(500)
def test_bench_two_ranks_code_path():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _run([sys.executable, "-W", "ignore", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
              "127.0.0.1", "--master-port", "29541", "bench.py", "--gpus", "2", "--gaussians", "8000", "--steps", "2", "--warmup", "1"],
             env={"SIXDGS_BENCH_BACKEND": "gloo", "SIXDGS_BENCH_FORCE_DEVICE": "0"})
    assert d["n_gpus"] == 2 and "cpu_baseline" not in d       # baseline only on rank 0 at N = 1
    assert abs(d["value"] - 2 * 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-2 * d["value"]   # whole-job aggregate over both ranks
    assert d["ranks_seen"] == 2 and d["backend"] == "gloo"


@pytest.mark.timeout(500)
def test_bench_plain_start_self_launches_the_ranks():
    """`python bench.py --gpus 2` with no rank environment (how the driver may start the scaling runs): bench.py becomes the
    launcher itself.  One GPU here, so the two ranks share it over gloo (test hooks); on the 8-GPU node the same path runs
    one rank per GPU over RCCL."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SIXDGS_BENCH_BACKEND="gloo", SIXDGS_BENCH_FORCE_DEVICE="0")
    p = subprocess.run([sys.executable, "-W", "ignore", "bench.py", "--gpus", "2", "--gaussians", "8000", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2


@pytest.mark.timeout(900)
def test_bench_pipelined_steps_give_the_poses_of_one_batch_at_a_time(tmp_path):
    """Round 5: two batches in flight (6dgs_amd.test.PoseStream: batch N + 1 submitted before batch N is collected, its image side on a second stream)
    against --no-pipeline: the same poses BIT FOR BIT, the pipelining named in the line.  --dump-outputs of both runs: the same arrays bit for bit,
    the poses those of the line; the plain run (no --full) prints none of the secondary figures."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    args = ["bench.py", "--gaussians", "40000", "--steps", "4", "--warmup", "1", "--skip-cpu-baseline", "--skip-reference-mode", "--l32-steps", "0"]
    da, db = str(tmp_path / "a"), str(tmp_path / "b")
    a = _run([sys.executable, "-W", "ignore", *args, "--full", "--dump-outputs", da], env={"SIXDGS_BENCH_DUMP_POSES": "1"})
    b = _run([sys.executable, "-W", "ignore", *args, "--no-pipeline", "--dump-outputs", db], env={"SIXDGS_BENCH_DUMP_POSES": "1"})
    assert a["config"]["pipeline"].startswith("2 batches in flight") and b["config"]["pipeline"].startswith("none")
    assert a["config"]["scoring_path"] == b["config"]["scoring_path"] == "select"
    assert a["poses_last_step"] == b["poses_last_step"] and len(a["poses_last_step"]) == 8
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db)) and {"c2w.npy", "topk_indices.npy", "topk_weights.npy", "up.npy"} <= set(names), names
    for n in names:
        xa, xb = np.load(os.path.join(da, n)), np.load(os.path.join(db, n))
        assert xa.dtype in (np.float32, np.float64) and xa.dtype == xb.dtype and np.array_equal(xa, xb), n
    assert np.array_equal(np.load(os.path.join(da, "c2w.npy")), np.asarray(a["poses_last_step"], np.float32))
    assert np.load(os.path.join(da, "topk_indices.npy")).shape == (8, 100)
    assert not {"roofline", "headline_b4", "reference_mode", "cpu_baseline", "fp32_logits_mode"} & set(b) and "roofline" in a
    assert a["median_step"]["n"] == b["median_step"]["n"] == 4 and "completions" in a["median_step"]["note"]
    assert a["headline_b4"]["images_per_gpu_per_step"] == 4 and a["headline_b4"]["value"] > 0 and "headline_b8" not in a      # the 4-image figure of rounds 1-5 beside it
    assert a["config"]["select_sweep_launches"] == [[8, 8]]                 # eight 256-token views: eight tiles, one launch


@pytest.mark.timeout(900)
def test_bench_eight_ranks_on_one_gpu_over_gloo():
    """the driver's first 8-GPU run is unattended, and nothing beyond two ranks had ever executed.  Eight ranks share the one GPU
    here (gloo, SIXDGS_BENCH_FORCE_DEVICE=0): scene + weight broadcast to seven peers, image sharding, the pipelined steps, ONE final fixed-size
    pose gather, max-over-ranks timing -- bench.py started plainly, so it also self-launches the ranks as the driver may."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SIXDGS_BENCH_BACKEND="gloo", SIXDGS_BENCH_FORCE_DEVICE="0", SIXDGS_RANDOM_BACKBONE="1", OMP_NUM_THREADS="2")
    p = _run_eight([sys.executable, "-W", "ignore", "bench.py", "--gpus", "8", "--gaussians", "8000", "--batch", "2", "--steps", "2", "--warmup", "1",
                    "--skip-reference-mode", "--l32-steps", "0"], env, 400)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_seen"] == 8 and d["backend"] == "gloo" and d["scaling"] == "weak" and "cpu_baseline" not in d
    assert abs(d["value"] - 8 * 2 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-2 * d["value"]          # whole-job aggregate over the eight ranks
    assert "image-sharded x8" in d["config"]["parallelism"]


@pytest.mark.timeout(600)
def test_bench_presets_cfg1_cfg2_and_streamed_scorer():
    """BASELINE.json configs as bench presets: cfg1 (10 k Gaussians, one 400x400 query), cfg2's code path (scene through a 3DGS
    PLY file, one query; size reduced here, the full 300 k run is tests/test_gpu_configs.py) and cfg4's streamed scorer at a
    small size."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _run([sys.executable, "-W", "ignore", "bench.py", "--config", "cfg1", "--steps", "5", "--skip-cpu-baseline", "--full"])
    assert d["config"]["preset"] == "cfg1" and d["config"]["gaussians"] == 10_000 and d["config"]["images_per_gpu_per_step"] == 1
    assert d["median_step"]["n"] == 5 and d["median_step"]["min_ms"] <= d["median_step"]["ms"] <= d["median_step"]["max_ms"]
    assert d["fp32_logits_mode"]["mma"] == "f16x3l32" and d["fp32_logits_mode"]["value"] > 0
    assert "traffic_source" in d["roofline"]
    d = _run([sys.executable, "-W", "ignore", "bench.py", "--config", "cfg2", "--gaussians", "20000", "--steps", "2", "--skip-cpu-baseline", "--full"])
    assert d["config"]["preset"] == "cfg2" and "PLY" in d["config"]["workload"] and d["config"]["images_per_gpu_per_step"] == 1
    d = _run([sys.executable, "-W", "ignore", "bench.py", "--config", "cfg4", "--gaussians", "4000", "--batch", "3", "--chunk-rays", "300000",
              "--steps", "1", "--skip-cpu-baseline", "--full"])
    assert d["config"]["scoring"] == "streamed" and d["config"]["rays"] == 4000 * 256 and d["roofline"]["launches"] >= 8


@pytest.mark.timeout(600)
def test_bench_cfg5_standin_sweep_at_full_scale():
    """BASELINE.json configs[4] AT ITS WORKLOAD: the twelve scenes of the reference's evaluation sweep (pretrain_eval_attention.py:200-248,
    tools/launch_all_mip_training.sh:3-9, tools/launch_all_tanks_and_temple_training.sh:3-7) at their Gaussian counts (0.3-6.1 M), every valid Gaussian x 64
    iso-cell rays (19 M - 392 M rays per scene), ALL 384 test views, 800-pixel queries, masked RGBA views for the T&T scenes, one arena for the per-scene
    buffers.  Per scene one view is checked against the CPU oracle on the first 2^20 rays of the scene (the oracle's OWN ray MLP + k_proj, scorer, top-100, pose
    solve): top-100 identical through both scorers, scores <= 1e-5, pose <= 1e-4 (north_star).  bicycle / garden / stump do not fit the GPU and are streamed,
    the other Mip-360 scenes are resident, the T&T scenes resident and masked.  Replaces the 1/50-scale and the 1/4-scale runs of rounds 4-5."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if torch.cuda.get_device_properties(0).total_memory < 200 * 2**30:
        pytest.skip("the full-scale sweep is sized for one MI355X (288 GB)")
    import time
    t0 = time.time()
    d = _run([sys.executable, "-W", "ignore", "bench.py", "--config", "cfg5-standin", "--oracle-rays", "1048576"], timeout=560)
    wall = time.time() - t0
    assert d["config"]["preset"] == "cfg5-standin" and len(d["scenes"]) == 12 and d["config"]["test_views"] == 384 and d["value"] > 0
    rows = {r["scene"]: r for r in d["scenes"]}
    assert list(rows)[0] == "mip_360_bicycle" and list(rows)[-1] == "tt_Truck"
    streamed = {"mip_360_bicycle", "mip_360_garden", "mip_360_stump"}
    gauss = {"mip_360_bicycle": 6_130_000, "mip_360_bonsai": 1_240_000, "mip_360_counter": 1_220_000, "mip_360_garden": 5_830_000, "mip_360_kitchen": 1_850_000,
             "mip_360_room": 1_590_000, "mip_360_stump": 4_960_000, "tt_Barn": 600_000, "tt_Caterpillar": 500_000, "tt_Family": 350_000, "tt_Ignatius": 300_000,
             "tt_Truck": 450_000}
    views = {"mip_360_bicycle": 25, "mip_360_bonsai": 37, "mip_360_counter": 30, "mip_360_garden": 24, "mip_360_kitchen": 35, "mip_360_room": 39,
             "mip_360_stump": 16, "tt_Barn": 48, "tt_Caterpillar": 46, "tt_Family": 19, "tt_Ignatius": 33, "tt_Truck": 32}
    for name, r in rows.items():
        assert r["gaussians"] == gauss[name] and r["test_views"] == views[name], name
        assert 0.8 * 64 * r["gaussians"] < r["rays"] <= 64 * r["gaussians"] and r["poses_per_s"] > 0
        lo, hi = r["tokens_per_image_min_max"]
        assert r["masked"] == name.startswith("tt_") and ((hi < 256 and lo >= 1) if r["masked"] else (lo == hi == 256)), (name, lo, hi)
        if name in streamed:
            assert r["scoring"] == "streamed" and r["rays"] > 300_000_000 and r["scoring_path"].startswith("streamed select"), (name, r["scoring_path"])
        else:
            assert r["scoring"] == "resident" and r["scoring_path"] == "select", (name, r["scoring_path"])
        p = r["parity_vs_oracle"]
        assert p["sample_rays"] == 1 << 20
        assert p["top100_identical_two_pass"] and p["top100_identical_select"] and p["score_rel_err"] < 1e-5 and p["pose_rel_err"] < 1e-4, (name, p)
        assert p["rot_err_deg_vs_oracle"] < 1e-2 and p["trans_err_vs_oracle"] < 4e-4, (name, p)
        items = r["setup_breakdown_s"]
        assert abs(sum(items.values()) - r["setup_s"]) <= 0.05 * r["setup_s"] + 0.02, (name, items, r["setup_s"])
        assert r["setup_standin_s"] == pytest.approx(sum(v for k, v in items.items() if k.startswith("standin_")), abs=2e-3)
    ps = d["parity_summary"]
    assert ps["scenes_checked"] == 12 and ps["all_top100_identical"]
    assert abs(d["scene_setup_s_total"] - sum(r["setup_s"] for r in d["scenes"])) < 0.1
    assert d["value"] > 0 and d["value_including_product_scene_setup"] >= d["value_including_scene_setup"]
    assert d["roofline"]["frac"] is not None and d["cpu_baseline"]["kind"] == "port" and d["process_setup_s"]["arena_gib"] > 150
    print(f"cfg5-standin at full scale: {d['value']:.2f} poses/s over {d['config']['test_views']} views ({d['eval_s_total']:.1f} s of evaluation, "
          f"{d['scene_setup_s_total']:.1f} s of scene set-up, {wall:.0f} s wall incl. the oracle checks); mean rotation error vs the oracle "
          f"{ps['mean_rot_err_deg_vs_oracle']:.2e} deg, mean translation error vs the oracle {ps['mean_trans_err_vs_oracle']:.2e} over {ps['scenes_checked']} checked views; "
          f"sweep {d['roofline']['achieved']} TFLOP/s")


@pytest.mark.timeout(900)
def test_evaluation_sweep_with_eight_ranks_on_one_gpu(tmp_path):
    """pretrain_eval_attention.py at EIGHT ranks (gloo, all on the one GPU) over three scenes whose 5 / 4 / 5 test views leave ranks with one
    view and ranks with NONE: scene + weight broadcast to seven peers, the emission seed, agree() behind every stage, test_pose_estimation over an
    empty block, gather_results -- and the same results.json as the single-process run."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    pkg = importlib.import_module("6dgs_amd")
    syn = importlib.import_module("6dgs_amd.synthetic")
    from test_gpu_e2e import _write_experiment
    root = str(tmp_path)
    srcs = syn.write_dataset_fixtures(os.path.join(root, "data"), 1, n_views=34, width=64, height=48)
    _write_experiment(root, syn, pkg, "mip_360_room_aa11", srcs["colmap_txt"], 3000, 4)
    _write_experiment(root, syn, pkg, "mip_360_garden_bb22", srcs["colmap_bin"], 2500, 5)
    _write_experiment(root, syn, pkg, "mip_360_stump_cc33", srcs["colmap_txt"], 2000, 6)
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base.update(SIXDGS_RANDOM_BACKBONE="1", OMP_NUM_THREADS="2")
    outs = []
    for name, launcher, extra in (("plain", [], {}),
                                  ("gloo8", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", "29571"],
                                   {"SIXDGS_DIST_BACKEND": "gloo", "SIXDGS_FORCE_DEVICE": "0"})):
        out = os.path.join(root, f"res_{name}.json")
        p = _run_eight([sys.executable, "-W", "ignore", *launcher, os.path.join(ROOT, "pretrain_eval_attention.py"), "--exp_path", os.path.join(root, "output"),
                        "--out_path", out, "--data_type", "mip360", "--skip_train", "--batch_size", "3", "--max_ellipsoids", "-1"], dict(base, **extra), 400)
        assert p.returncode == 0, p.stderr[-3000:]
        if name == "gloo8":
            assert "evaluation sweep over 8 rank(s), backend gloo" in (p.stdout + p.stderr)
        outs.append(json.load(open(out)))
    assert len(outs[0]) == len(outs[1]) >= 12
    for a, b in zip(*outs):
        assert (a["sequence_id"], a["frame_id"]) == (b["sequence_id"], b["frame_id"])
        assert a["gt_c2w"] == b["gt_c2w"]
        # (the backbone's GEMMs see batches of 3 views in one run and of 1 in the other: library kernels are not bit-stable across batch sizes)
        assert np.abs(np.asarray(a["pred_c2w"]) - np.asarray(b["pred_c2w"])).max() < 1e-5
