"""sixdgs_image_metrics on the GPU: SSIM -- and without quantise L1 and the squared errors -- against the fp64 restatement
(tests/metrics_reference.py) under a bound taken from the restatement's own fp32 rounding; with quantise the integer sums' outputs and
the render's bytes bit for bit, special values included; SSIM and L1 against sixdgs_photometric_loss bit for bit; determinism and
batching; guard bytes through the raw C call; the fourth channel; the refusals; and the reference's stored values.  Everything runs
inside this process.

Measured on MI355X (profiles/evaluate_views.md): parity worst |gpu - fp64| / bound 0.45 (a channel's squared error on the 289-tile
case, whose bound is the floor of 1e-6 of the scale; 0.19 below that case)."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as MR  # noqa: E402
import photometric_reference as PR  # noqa: E402
from test_metrics_host import GOLDEN_BOUND, MODES, refusals  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COLUMNS = {"l1": slice(0, 1), "ssim": slice(1, 2), "mse": slice(2, 3), "mse_c": slice(3, 6)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def forms(x, kind):
    return G(x["target_u8"]) if kind == "u8" else G(x["target_f"] if kind == "f4" else x["target_f"][..., :3])


@pytest.mark.parametrize("views,height,width", MR.CASES)
def test_parity_against_fp64(ops, views, height, width):
    worst = 0.0
    for quantise in (False, True):
        for kind in ("f3", "f4", "u8"):
            c = MR.case(views, height, width, quantise, kind == "u8")
            x, r64 = c["x"], c["r64"]
            target = forms(x, kind)
            for stride in (3, 4):
                what = f"{views}x{height}x{width} quantise={quantise} {kind} stride={stride}"
                metrics, render = ops.image_metrics(G(x["image"][..., :stride]), target, quantise=quantise, want_render=True)
                assert metrics.shape == (views, 6) and metrics.dtype == torch.float32 and render.shape == (views, height, width, 3)
                got = metrics.cpu().numpy()
                for k in (("ssim",) if quantise else MR.KEYS):
                    scale, y, limit = c["bounds"][k]
                    err = float(np.abs(got[:, COLUMNS[k]].astype(np.float64).reshape(r64[k].shape) - r64[k]).max())
                    assert limit <= PR.CEILING * scale, f"{what} {k}: the case is unfit"
                    print(f"{what} {k}: max |gpu - fp64| {err:.3e} (scale {scale:.3e}, y {y:.3e}, bound {limit:.3e}, ratio {err / limit:.3f})")
                    assert np.isfinite(got).all() and err <= limit, f"{what} {k}: {err:.3e} > {limit:.3e}"
                    worst = max(worst, err / limit)
                # the render's bytes are the 8-bit rule's whatever quantise is, the planted values included
                assert np.array_equal(render.cpu().numpy(), r64["render_u8"]), what
                if quantise:
                    for col in (0, 2, 3, 4, 5):
                        assert np.array_equal(got[:, col].view(np.int32), r64["exact"][:, col].view(np.int32)), (what, col)
    print(f"{views}x{height}x{width}: worst measured / bound {worst:.3f}")


def test_l1_and_ssim_are_the_photometric_losss_bits(ops):
    """Inputs already in [0, 1]: the clamp changes nothing, and the sums are sixdgs_photometric_loss's, tile for tile."""
    for views, height, width in ((3, 17, 33), (2, 272, 260)):
        x = PR.inputs(views, height, width)
        for target in (G(x["target_u8"]), G(x["target_f"]), G(x["target_f"][..., :3])):
            for stride in (3, 4):
                image = G(x["image"][..., :stride])
                _, parts = ops.photometric_loss(image, target, want_parts=True)
                metrics = ops.image_metrics(image, target, quantise=False)
                assert same(metrics[:, :2].contiguous(), parts) and bool((metrics[:, 2:] > 0).all())


def test_views_do_not_mix_and_calls_repeat(ops):
    x = MR.inputs(3, 17, 33)
    image, target = G(x["image"]), G(x["target_f"])
    for quantise in (False, True):
        batch = ops.image_metrics(image, target, quantise=quantise, want_render=True)
        again = ops.image_metrics(image, target, quantise=quantise, want_render=True)
        assert same(batch[0], again[0]) and torch.equal(batch[1], again[1])
        for v in range(3):
            one = ops.image_metrics(image[v:v + 1].contiguous(), target[v:v + 1].contiguous(), quantise=quantise, want_render=True)
            assert same(one[0][0], batch[0][v]) and torch.equal(one[1][0], batch[1][v]), v
        # the fourth channel, NaN on both sides, is never read
        dirty_i, dirty_t = image.clone(), target.clone()
        dirty_i[..., 3] = float("nan")
        dirty_t[..., 3] = float("nan")
        dirty = ops.image_metrics(dirty_i, dirty_t, quantise=quantise, want_render=True)
        assert same(dirty[0], batch[0]) and torch.equal(dirty[1], batch[1]) and bool(torch.isfinite(dirty[0]).all())
        # NaN all over one view: it counts as 0 there, and the other views' rows stay
        ruined = image.clone()
        ruined[1, ..., :3] = float("nan")
        got = ops.image_metrics(ruined, target, quantise=quantise)
        assert same(got[0], batch[0][0]) and same(got[2], batch[0][2]) and not same(got[1], batch[0][1]) and bool(torch.isfinite(got).all())
        zero = image.clone()
        zero[1, ..., :3] = 0.0
        assert same(ops.image_metrics(zero, target, quantise=quantise), got)
    assert ops.image_metrics(image[:0], target[:0], quantise=True).shape == (0, 6)          # no views


def test_guard_bytes_through_the_c_call(ops):
    lib = importlib.import_module("6dgs_amd._lib").load()
    views, height, width = 2, 40, 24
    x = MR.inputs(views, height, width)
    image, target = G(x["image"]), G(x["target_u8"])
    guard = 256
    p = lambda t, off=0: t.data_ptr() + off      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    need = ops.image_metrics_workspace_bytes(views, width, height)
    assert need == (views * 3 * 2 * 20 + 255) // 256 * 256
    for quantise in (0, 1):
        want = ops.image_metrics(image, target, quantise=bool(quantise), want_render=True)
        for with_render in (1, 0):
            ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")       # exactly workspace_bytes between the guards
            outs = [torch.full((s + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda") for s in (4 * 6 * views, views * height * width * 3)]
            st = lib.sixdgs_image_metrics(p(image), 4, p(target), 1, 3, views, width, height, quantise, p(outs[0], guard),
                                          p(outs[1], guard) if with_render else None, p(ws, guard), need, stream, None)
            torch.cuda.synchronize()
            assert st == 0
            assert bool((ws[:guard] == 0xA5).all()) and bool((ws[-guard:] == 0xA5).all()), "the workspace's guard bytes were written"
            for o, k in zip(outs, ("metrics", "render_u8")):
                assert bool((o[:guard] == 0x5A).all()) and bool((o[-guard:] == 0x5A).all()), f"the guard bytes of {k} were written"
            assert torch.equal(outs[0][guard:-guard].view(torch.float32), want[0].reshape(-1))
            if with_render:
                assert torch.equal(outs[1][guard:-guard], want[1].reshape(-1))
            else:
                assert bool((outs[1] == 0x5A).all()), "a render was written without being asked for"
    assert lib.sixdgs_image_metrics(p(image), 4, p(target), 1, 3, views, width, height, 0, p(outs[0], guard), None, p(ws, guard), need - 1, stream,
                                    None) == -2


def test_entry_points_refuse_before_any_device_work(ops):
    refusals()
    image, target = torch.zeros(2, 16, 16, 4), torch.zeros(2, 16, 16, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.image_metrics(image, target, quantise=True)
    for bad in (dict(quantise=2), dict(quantise=None)):
        with pytest.raises(ValueError):
            ops.image_metrics(image, target, **bad)
    for bad_target in (torch.zeros(2, 16, 16, 4, dtype=torch.uint8), torch.zeros(2, 16, 16, 2), torch.zeros(3, 16, 16, 3)):
        with pytest.raises(ValueError):
            ops.image_metrics(image, bad_target, quantise=False)


def test_golden_against_the_reference(ops, golden):
    """|gpu - reference| within the golden bound (8 x the measured |fp64 restatement - reference|) plus the pair's parity bound; the
    PSNRs are derived as evaluate.py derives them, and their parity bound is the mse's carried through 10 log10(1 / mse)."""
    ev = importlib.import_module("6dgs_amd.evaluate")
    g = golden("g17_metrics")
    for name in g["names"]:
        image, target = g[f"{name}_image"][None], g[f"{name}_target"][None]
        for mode in MODES:
            quantise = mode == "u8"
            r64, r32 = MR.evaluate(image, target, quantise, np.float64), MR.evaluate(image, target, quantise, np.float32)
            b = MR.bounds(r64, r32)
            row = ops.image_metrics(G(image), G(target), quantise=quantise)[0].cpu().numpy()
            db = 10.0 / np.log(10.0)
            got = {"l1": (row[0], b["l1"][2]), "ssim": (row[1], b["ssim"][2]), "ssim4": (row[1], b["ssim"][2]),
                   "psnr": (ev.psnr_of_mse(row[2:3])[0], db * b["mse"][2] / r64["mse"][0]),
                   "psnr_channels": (ev.psnr_of_channels(row[None, 3:6])[0], db * b["mse_c"][2] / r64["mse_c"].min())}
            for k, (v, own) in got.items():
                ref = float(g[f"{name}_{mode}_{k}"])
                if k.startswith("psnr"):        # the derived value is rounded to float32 once more
                    own += float(np.spacing(np.float32(abs(ref)))) / 2
                print(f"{name} {mode} {k}: |gpu - reference| {abs(v - ref) / abs(ref):.2e} of the scale (bound {GOLDEN_BOUND[k] + own / abs(ref):.2e})")
                assert abs(float(v) - ref) <= GOLDEN_BOUND[k] * abs(ref) + own, (name, mode, k)
