"""The select sweep's block-wise epilogue (the default of the 16x16x32 tile: the epilogue of a tile runs ray block by ray block under the MFMAs of
its last slab and of the next tile's first one, csrc/score.hip: SweepEpi) against the per-tile epilogue (SIXDGS_SWEEP_EPILOGUE=tile), BIT FOR BIT.

Both forms do the same floating-point operations in the same order per value, so nothing here has a tolerance: after begin() + sweep() on a
zeroed workspace the two runs must leave the same bytes in
  * the whole stage workspace -- it holds the quarter rows `ub` the sweep stores, the per-group token partials and the q planes;
  * U after the finish pass (the rays of the scene) and the per-tile maxima;
  * gsum (g_t after the merge).
Shapes are the smallest at which each path of the new order exists: one tile per group (prologue and drain only), two to seven tiles per group
(the carry-over into slab 0 with its zero C operand, a drain behind a ragged tile), several groups per persistent set (the drain at the group
loop's boundary), 1 / 3 / 8 slots, token counts that leave wave rows inactive, packed slots, the 32x32x16 shape (which the switch must not
touch) and, in one child process each because the library reads that mode once, the sibling modes 0 and 2."""
import importlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("SIXDGS_SWEEP_EPILOGUE", "SIXDGS_SWEEP_MFMA")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = importlib.import_module("6dgs_amd.ops")
    o.set_mma_mode(o.MMA_DEFAULT)
    return o


@pytest.fixture
def switches():
    """Sets the sweep's developer switches for one call and restores them (the library reads both at every launch)."""
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def use(epilogue=None, mfma=None):
        for k, v in zip(SWITCHES, (epilogue, mfma)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    yield use
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def make_case(ops, r, seed, n_tok, q_scale=6.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    key = (torch.randn(r, 384, generator=g) * 0.07).cuda()
    q = torch.randn(len(n_tok), 256, 384, generator=g) * q_scale
    for b, t in enumerate(n_tok):
        q[b, t:] = 0.0
    q = q.cuda()
    nt = torch.tensor(n_tok, dtype=torch.int32, device="cuda")
    planes, scale = ops.split_planes_f16(key)
    si = ops.select_sample_indices(r, "cuda") if r >= ops.SELECT_SAMPLE_STRIDE else torch.tensor([r // 2], device="cuda")
    s_planes, s_scale = ops.split_planes_f16(key[si].contiguous())
    return dict(r=r, q=q, nt=nt, n_tok=list(n_tok), planes=planes, scale=scale, s_planes=s_planes, s_scale=s_scale)


def sweep(ops, c):
    ss = ops.SelectStream(c["q"], c["nt"], c["r"], 100, 4096, c["n_tok"])
    ss.reserve(c["r"])
    ss.ws.zero_()
    ws_at = ss.ws.data_ptr()
    ss.begin(c["s_planes"], c["s_scale"])
    ss.sweep(c["planes"], c["scale"], 0)
    torch.cuda.synchronize()
    assert ss.ws.data_ptr() == ws_at, "the workspace grew: its unwritten bytes are not comparable"
    return {"workspace (ub rows, token partials)": ss.ws.clone(), "U": ss.u[:, :c["r"]].clone(), "tile maxima": ss.utm.clone(), "gsum": ss.gsum.clone()}


def same_bits(ops, c, use, tag, mfma=None):
    use(None, mfma)
    new = sweep(ops, c)
    use("tile", mfma)
    old = sweep(ops, c)
    use()
    for name in new:
        a, b = new[name], old[name]
        a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a, b)
        n = int((a != b).sum())
        print(f"[sweep epilogue] {tag}: {name}: {n} of {a.numel()} words differ")
        assert n == 0, f"{tag}: {name} differs from the per-tile epilogue in {n} words"
    for b, t in enumerate(c["n_tok"]):                       # and the answer is one: finite, positive where there is something to sum
        if t > 0:
            assert bool(torch.isfinite(new["U"][b]).all()) and bool((new["U"][b] > 0).all()), f"{tag} image {b}: U"
            assert bool((new["gsum"][b, :t] > 0).all()) and bool((new["gsum"][b, t:] == 0).all()), f"{tag} image {b}: g_t"


@pytest.mark.parametrize("r", [255, 256, 257])
def test_single_tile(ops, switches, r):
    """One tile per group: the prologue and the drain alone, the carry-over never runs.  One slot (one-shot grid) and three (persistent)."""
    same_bits(ops, make_case(ops, r, 3 + r, (256,)), switches, f"R={r} one slot")
    same_bits(ops, make_case(ops, r, 4 + r, (256, 200, 129)), switches, f"R={r} three slots")


def test_three_tiles_per_workgroup_last_one_ragged(ops, switches):
    """769 tiles in 256 groups: 3 tiles per workgroup (the first group 4), the scene's last tile holds one ray."""
    same_bits(ops, make_case(ops, 196_608 + 1, 21, (256,)), switches, "R=196609 one slot")


def test_several_groups_per_persistent_set(ops, switches):
    """3 slots: 85 sets walk 256 groups of 6-7 tiles -- carry-over inside a group, drain at the group loop's boundary, then a fresh prologue."""
    same_bits(ops, make_case(ops, 400_003, 22, (256, 256, 256)), switches, "R=400003 three slots")


@pytest.mark.parametrize("slots", [1, 3, 8])
def test_slot_counts(ops, switches, slots):
    """274 tiles in 256 groups: groups of one and of two tiles side by side."""
    same_bits(ops, make_case(ops, 70_001, 30 + slots, (256,) * slots), switches, f"{slots} slots")


@pytest.mark.parametrize("t", [256, 65, 64, 1])
def test_token_counts(ops, switches, t):
    """Wave rows beyond the token count run no epilogue pieces (65: two active rows, 64 and 1: one), alone and beside full images."""
    same_bits(ops, make_case(ops, 70_001, 50 + t, (t,)), switches, f"t={t} one image")
    same_bits(ops, make_case(ops, 70_001, 51 + t, (t, 256, t)), switches, f"t={t} beside 256")


def test_packed_slots(ops, switches):
    """Quarters and halves of several images share a slot (sweep_plan.h): per-quarter scales and offsets under the carried pieces."""
    same_bits(ops, make_case(ops, 70_001, 61, (64, 30, 128, 1, 64, 100, 200, 0, 17)), switches, "packed")


def test_32x32x16_shape_is_untouched(ops, switches):
    same_bits(ops, make_case(ops, 70_001, 71, (256, 137)), switches, "SIXDGS_SWEEP_MFMA=32", mfma=32)


CHILD = r"""
import importlib, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import test_gpu_sweep_epilogue as t
ops = importlib.import_module("6dgs_amd.ops")
ops.set_mma_mode(ops.MMA_DEFAULT)
def use(epilogue=None, mfma=None):
    for k, v in zip(t.SWITCHES, (epilogue, mfma)):
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))
t.same_bits(ops, t.make_case(ops, 400_003, 81, (256, 137, 256)), use, "sibling mode " + os.environ["SIXDGS_SIBLING_SYNC"])
"""


@pytest.mark.parametrize("mode", [0, 2])
def test_sibling_modes(ops, mode):
    """The library reads SIXDGS_SIBLING_SYNC once per process: one child each, one after the other (0: one-shot grid for every slot count,
    2: persistent sets without the per-tile meeting)."""
    env = dict(os.environ, SIXDGS_SIBLING_SYNC=str(mode))
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
