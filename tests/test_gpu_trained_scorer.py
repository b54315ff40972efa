"""A scorer TRAINED on rendered views of a stand-in scene (render_views + train_id_module(batched_window=True)), one training run
shared by the tests of this module: it trains on its own objective, it learns poses, the inference path -- select, two-pass, CPU
oracle -- agrees on the trained (peaked) weights under DESIGN §2's bars, and the checkpoint round-trips.

Scene and run: make_scene(5000, 11), 50 training and 16 held-out views of 224 x 224 (the backbone's crop size), random-init ViT,
600 iterations x 32 images on the reference's 1000-ellipsoid emission renewed every 10 iterations.

The 33-of-50 bar of test_training_improves_the_pose_of_most_training_views is not tuned: if training did nothing for the pose each
view would improve with probability 1/2, and 33 or more of 50 then has probability below 2 % (binomial)."""
import importlib
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_GAUSS, SEED, TRAIN_VIEWS, HELD_VIEWS, SIZE, ITERATIONS = 5000, 11, 50, 16, 224, 600
MUST_IMPROVE = 33


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ts = importlib.import_module("train_standin")
    pkg = importlib.import_module("6dgs_amd")
    ops = importlib.import_module("6dgs_amd.ops")
    ops.set_mma_mode(ops.MMA_DEFAULT)
    t0 = time.time()
    torch.manual_seed(0)
    scene, train_cams, held_cams = ts.build_standin(N_GAUSS, SEED, TRAIN_VIEWS, HELD_VIEWS, SIZE)
    idm = ts.fresh_scorer().eval()
    rays = pkg.generate_all_possible_rays(scene)          # one fixed emission for every pose error, before and after
    up = ts.model_up_of(train_cams)
    before = {"train": ts.pose_errors(idm, train_cams, rays, up), "held": ts.pose_errors(idm, held_cams, rays, up)}
    ckpt = str(tmp_path_factory.mktemp("standin") / "id_module.th")
    t1 = time.time()
    loss = ts.train(idm, scene, train_cams, held_cams, ckpt, ITERATIONS)
    torch.cuda.synchronize()
    t2 = time.time()
    after = {"train": ts.pose_errors(idm, train_cams, rays, up), "held": ts.pose_errors(idm, held_cams, rays, up)}
    print(f"\n[trained scorer] {rays[0].shape[0]} rays; set-up {t1 - t0:.1f} s, {ITERATIONS} iterations in {t2 - t1:.1f} s "
          f"({ITERATIONS / (t2 - t1):.1f} /s), evaluation {time.time() - t2:.1f} s")
    yield dict(ts=ts, pkg=pkg, ops=ops, scene=scene, train_cams=train_cams, held_cams=held_cams, idm=idm, rays=rays, up=up, before=before,
               after=after, loss=loss, ckpt=ckpt)
    idm.invalidate_caches()
    torch.cuda.empty_cache()


def test_rendered_views_of_one_scene_differ(run):
    """What the random-byte views could not give: image content, and backbone tokens, that follow the camera."""
    cams = run["train_cams"]
    assert cams[0].image.shape == (SIZE, SIZE, 3) and cams[0].image.dtype == np.uint8
    covered = np.mean([(c.image != 255).any(axis=-1).mean() for c in cams])
    assert covered > 0.5, covered
    toks, _ = run["ts"].image_side(run["idm"], cams[:2])
    diff = float((toks[0] - toks[1]).abs().max())
    print(f"coverage of the training views {covered:.3f}; largest token difference between two views {diff:.3g}")
    assert diff > 0


def test_training_reduces_its_own_objective(run):
    loss = run["loss"]
    assert len(loss) == ITERATIONS and np.isfinite(loss).all()
    first, last = float(np.mean(loss[:20])), float(np.mean(loss[-20:]))
    print(f"train/loss_score: first 20 iterations {first:.6g}, last 20 {last:.6g}")
    assert last < first, (first, last)


def test_training_improves_the_pose_of_most_training_views(run):
    """Per training view, the translation error (camera centre) with the trained weights against the same view with the initial weights:
    at least 33 of 50 improve.  A pose that is NaN or identity after training counts as not improved.  The medians are printed, no bar
    is set on them nor on the held-out views."""
    ts = run["ts"]
    for split in ("train", "held"):
        (tb, rb, bb), (ta, ra, ba) = run["before"][split], run["after"][split]
        print(f"{split}: median translation error {np.nanmedian(tb):.4f} -> {np.nanmedian(ta):.4f}, median rotation error "
              f"{np.nanmedian(rb):.2f} -> {np.nanmedian(ra):.2f} deg, unusable poses {int(bb.sum())} -> {int(ba.sum())}, "
              f"improved {ts.improved_views(tb, ta, ba)} of {len(tb)}")
    (tb, _, _), (ta, _, ba) = run["before"]["train"], run["after"]["train"]
    assert len(tb) == TRAIN_VIEWS == 50
    improved = ts.improved_views(tb, ta, ba)
    assert improved >= MUST_IMPROVE, f"{improved} of 50 training views improved"


def test_select_two_pass_and_oracle_agree_on_trained_weights(run, oracle):
    """16 rendered views on the trained weights: top-100 of the select path and of the two-pass scorer identical to the oracle's wherever
    its gap at the cut exceeds MARGIN = 8e-6, scores within 1e-5, pose within 1e-4.  A view the select path refuses (status -1) comes
    back through the two-pass fallback and is held to the same bars.  The number of refusals is printed, not bounded."""
    ts = run["ts"]
    rows = ts.trained_parity(run["idm"], run["held_cams"], run["rays"], oracle)
    assert len(rows) >= 16
    st = [r["status"] for r in rows]
    print(f"select statuses on trained weights: {st} ({sum(1 for s in st if s < 0)} refused)")
    print(f"logit range max {max(r['logit_range'] for r in rows):.3g}, largest softmax mass {max(r['softmax_peak'] for r in rows):.3g}, "
          f"smallest gap at the cut {min(r['gap_at_cut'] for r in rows):.3g}")
    print(f"score err {max(r['score_err'] for r in rows):.3g}; value err select {max(r['select_value_err'] for r in rows):.3g} two-pass "
          f"{max(r['two_pass_value_err'] for r in rows):.3g}; pose err select {max(r['select_pose_err'] for r in rows):.3g} two-pass "
          f"{max(r['two_pass_pose_err'] for r in rows):.3g}; identical lists select {sum(r['select_identical'] for r in rows)} two-pass "
          f"{sum(r['two_pass_identical'] for r in rows)} of {len(rows)}")
    for b, r in enumerate(rows):
        assert r["select_top_ok"] and r["two_pass_top_ok"], (b, r)
        assert r["score_err"] <= ts.SCORE_TOL and r["select_value_err"] <= ts.SCORE_TOL and r["two_pass_value_err"] <= ts.SCORE_TOL, (b, r)
        assert r["select_pose_err"] <= ts.POSE_TOL and r["two_pass_pose_err"] <= ts.POSE_TOL, (b, r)
    assert ts.SCORE_TOL == 1e-5 and ts.POSE_TOL == 1e-4 and ts.MARGIN == 8e-6


def test_checkpoint_round_trips(run):
    """id_module.th loads into a fresh IdentificationModule and reproduces the top-100."""
    ts, idm, rays = run["ts"], run["idm"], run["rays"]
    ck = torch.load(run["ckpt"], map_location="cpu")
    assert ck["epoch"] == ITERATIONS and "optimizer_state_dict" in ck
    fresh = run["pkg"].IdentificationModule("dino")
    missing, unexpected = fresh.load_state_dict(ck["model_state_dict"], strict=False)
    assert not unexpected and not [m for m in missing if not m.startswith("backbone_wrapper.")], (missing, unexpected)
    fresh = fresh.cuda().eval()
    toks, _ = ts.image_side(idm, run["held_cams"][:4])
    i_a, v_a, _ = idm.score_tokens(toks, *rays, 100, want_scores=True)
    i_b, v_b, _ = fresh.score_tokens(toks, *rays, 100, want_scores=True)
    assert torch.equal(i_a, i_b) and torch.equal(v_a, v_b)
    fresh.invalidate_caches()
