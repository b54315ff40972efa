"""Data-parallel window training (train_id_module(data_parallel=True)) with two ranks that share the one GPU of the test box and talk
over gloo: tools/train_dp_check.py runs under torch.distributed.run once for the module and prints one JSON line; the tests read it.
On a multi-GPU node the tool runs unchanged over RCCL (--backend nccl)."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-W", "ignore", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29581", "tools/train_dp_check.py", "--backend", "gloo", "--device", "0"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=540)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_summed_gradients_meet_the_fp64_per_image_loop(report):
    """One iteration of 32 draws split 16 / 16 over the ranks (auto-split scorer backward on each), gradients summed by dd.sum_gradients:
    every one of the 24 trainable parameters within 4 x the fp32 PyTorch per-image loop's error + u sqrt(R) of the fp64 per-image loop
    (the yardstick of test_gpu_train_window.test_window_equals_the_per_image_loop)."""
    g = report["gradients"]
    assert report["world"] == 2 and report["backend"] == "gloo"
    assert g["draws"] == [0, 16] and g["finite"]
    assert g["params"] == 24 and g["same_names"]
    assert not g["out_of_bound"], g
    print(f"summed gradients: largest error / bound {g['worst_ratio']:.2f}")


@pytest.mark.timeout(600)
def test_ranks_hold_the_same_parameters(report):
    """After 4 iterations of train_id_module(batched_window=True, data_parallel=True, backward_ray_groups=0) both ranks' state_dicts are the
    same bits (every rank steps Adafactor on the same all-reduced gradients), and both logged the same (all-reduced) scalars."""
    t = report["training"]
    assert t["state_dicts_identical"] and t["logs_identical_on_ranks"]
    assert t["iterations"] == 4 and t["finite"] and t["evaluated"]


@pytest.mark.timeout(600)
def test_losses_match_the_single_rank_window(report):
    """Rank 0's logged loss, camera-up and score terms against a single-rank batched_window=True run from the same seed (same rays, same
    draws: rank 0 consumes the random numbers of the single-rank run; 4 images per iteration, 2 per rank).

    Iteration 0 evaluates the same parameters on the same images; only the order of the sum over the images (2 + 2 across the ranks) and
    the batch sizes of the image-side products differ: bound 16 u relative.

    Iteration 1 starts from parameters one Adafactor step apart.  Adafactor's step is lr x max(1e-3, RMS(p)) x u with an update u normalised
    by the second moment (clipped to RMS 1), so to first order a relative error e of the gradient changes u, and with it the loss change of
    the step L1 - L0, by at most 2 e relative.  (Elements whose gradient is below the rounding noise may flip the sign of their update, but
    they enter the loss with that near-zero gradient.)  The summed gradients are within 4 x the fp32 PyTorch error of fp64 (the first test;
    the ray-group split only changes rounding): e <= 1e-4.  Bound on the loss: 2e-4 |L1 - L0| + 16 u |L1| (its two terms are not what the
    step descends along, so they get only the iteration-0 bound).

    From iteration 2 on the two runs are two rounding trajectories, not one: a 4-image window at Adafactor's relative step changes the loss
    by a factor of 3 per iteration, and the normalised update amplifies the iteration-1 difference by about 10^2 per step (one MI355X:
    3.5 % at iteration 2, 17 % at iteration 3).  There the check is that both runs are finite and keep decreasing the loss alike; the
    state_dicts of the ranks, the reduced logs and the gradients of one iteration are checked exactly or against fp64 above."""
    t = report["training"]
    dp, single = t["logs_dp"], t["logs_single"]
    ratios = []
    for name, a, b in zip(("loss", "cam_up", "loss_score"), dp, single):
        assert len(a) == len(b) == 4, name
        ratios.append(abs(a[0] - b[0]) / (16 * 2.0 ** -24 * abs(b[0])))
        if name == "loss":
            ratios.append(abs(a[1] - b[1]) / (2e-4 * abs(b[1] - b[0]) + 16 * 2.0 ** -24 * abs(b[1])))
        assert all(math.isfinite(v) and v >= 0 for v in a + b), name
    print(f"logged scalars, iterations 0 and 1: largest |dp - single| / bound = {max(ratios):.3g}; "
          f"losses dp {[f'{v:.6g}' for v in dp[0]]}, single {[f'{v:.6g}' for v in single[0]]}")
    assert max(ratios) <= 1.0, (dp, single)
    assert dp[0][3] < dp[0][0] and single[0][3] < single[0][0]


@pytest.mark.timeout(600)
def test_checkpoint_keys_are_those_of_the_single_rank_window(report):
    assert report["training"]["checkpoint_keys_match"]
