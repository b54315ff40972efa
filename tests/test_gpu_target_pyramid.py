"""sixdgs_target_pyramid on the GPU against the fp32 restatement of tests/pyramid_reference.py, bit for bit: one and three views, RGB
and RGBA with and without compositing, crops on one axis, both and neither, several levels in one call, a 1 x 1 level, d = 3, d = 256,
strips wider than one workgroup, rows whose 16-byte phase changes from row to row and a base that is not pixel aligned; guard bytes
around every output; each view alone; two calls; what is refused without a launch."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 256
BG = (0.25, 1.0, 0.6)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    importlib.import_module("6dgs_amd")
    return importlib.import_module("6dgs_amd.ops")


def guarded(shape):
    n = int(np.prod(shape)) * 4
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32).reshape(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == 0x5A).all()) and bool((buf[-GUARD:] == 0x5A).all())


def on_gpu(images, offset=0):
    """The images on the GPU as a contiguous tensor whose first byte lies `offset` bytes behind a 256-byte boundary."""
    flat = torch.zeros(images.size + 256, dtype=torch.uint8, device="cuda")
    flat[offset:offset + images.size] = torch.from_numpy(images.reshape(-1)).cuda()
    t = flat[offset:offset + images.size].view(images.shape)
    assert t.is_contiguous() and t.data_ptr() % 256 == offset
    return t


def run(ops, images, ds, composite, offset=0):
    """One call into guarded outputs -> the levels as numpy arrays."""
    V, H, W, _ = images.shape
    bufs, outs = zip(*[guarded((V,) + R.geometry(W, H, d)[1::-1] + (3,)) for d in ds])
    for o in outs:
        o.fill_(float("nan"))
    got = ops.target_pyramid(on_gpu(images, offset), ds, composite=composite, background=BG, out=list(outs))
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in bufs), "guard bytes were written"
    return [g.cpu().numpy() for g in got]


# (W, H, downscales): crops on one axis, both, neither; a 1 x 1 level; d = 3; the wide-load tail; more than one workgroup per row
SIZES = ((37, 29, (8, 4, 2, 1)), (64, 64, (8, 4, 2, 1)), (17, 16, (8, 4, 2, 1)), (37, 29, (29, 3)), (263, 5, (1, 2, 3, 5)), (1100, 3, (1, 2, 3)))
KINDS = ((3, False), (4, False), (4, True))


@pytest.mark.parametrize("views", (1, 3))
@pytest.mark.parametrize("channels,composite", KINDS)
@pytest.mark.parametrize("W,H,ds", SIZES)
def test_levels_are_the_fp32_restatement_bit_for_bit(ops, views, channels, composite, W, H, ds):
    images = np.random.default_rng(W * H + channels + views).integers(0, 256, (views, H, W, channels), dtype=np.uint8)
    got = run(ops, images, ds, composite)
    for d, g in zip(ds, got):
        want = R.target_f32(images, d, composite, BG)
        assert g.shape == want.shape and g.dtype == np.float32
        assert np.array_equal(R.bits(g), R.bits(want)), f"d {d}: {int((R.bits(g) != R.bits(want)).sum())} of {want.size} entries differ"
    if (W, H) == (37, 29) and 29 in ds:
        assert got[0].shape == (views, 1, 1, 3)
    again = run(ops, images, ds, composite)
    assert all(np.array_equal(R.bits(a), R.bits(b)) for a, b in zip(got, again)), "two calls, different bytes"
    if views > 1:
        for v in range(views):
            alone = run(ops, images[v:v + 1], ds, composite)
            assert all(np.array_equal(R.bits(a[0]), R.bits(b[v])) for a, b in zip(alone, got)), f"view {v} alone differs"


@pytest.mark.parametrize("channels,composite", KINDS)
def test_largest_downscale_and_strips_of_several_workgroups(ops, channels, composite):
    """d = 256 on 1300 x 300: five output columns where a workgroup takes four; with full bytes S1 is at its largest."""
    rng = np.random.default_rng(channels)
    images = rng.integers(0, 256, (1, 300, 1300, channels), dtype=np.uint8)
    images[:, :, 650:] = 255
    got = run(ops, images, (256, 100), composite)
    for d, g in zip((256, 100), got):
        assert np.array_equal(R.bits(g), R.bits(R.target_f32(images, d, composite, BG))), d
    assert got[0].shape == (1, 1, 5, 3)


@pytest.mark.parametrize("offset", (1, 2, 7, 16))
@pytest.mark.parametrize("channels,composite", KINDS)
def test_a_base_that_is_not_aligned(ops, channels, composite, offset):
    images = np.random.default_rng(offset).integers(0, 256, (2, 9, 45, channels), dtype=np.uint8)
    got = run(ops, images, (1, 2, 4), composite, offset)
    for d, g in zip((1, 2, 4), got):
        assert np.array_equal(R.bits(g), R.bits(R.target_f32(images, d, composite, BG))), d


def test_extreme_bytes_and_alpha(ops):
    for value, alpha in ((0, 0), (255, 255), (255, 0), (0, 255)):
        images = np.full((1, 16, 16, 4), value, np.uint8)
        images[..., 3] = alpha
        for composite in (False, True):
            got = run(ops, images, (16, 4, 1), composite)
            for d, g in zip((16, 4, 1), got):
                assert np.array_equal(R.bits(g), R.bits(R.target_f32(images, d, composite, BG))), (value, alpha, composite, d)
    # the fourth channel does not enter without compositing
    a = np.random.default_rng(0).integers(0, 256, (1, 8, 8, 4), dtype=np.uint8)
    b = a.copy()
    b[..., 3] = 255 - b[..., 3]
    assert all(np.array_equal(R.bits(x), R.bits(y)) for x, y in zip(run(ops, a, (2, 1), False), run(ops, b, (2, 1), False)))


def test_refusals_make_no_launch(ops):
    lib = importlib.import_module("6dgs_amd._lib").load()
    images = on_gpu(np.zeros((1, 16, 16, 3), np.uint8))
    with pytest.raises(ValueError):
        ops.target_pyramid(images, [17])                      # larger than the image
    with pytest.raises(ValueError):
        ops.target_pyramid(images, [2] * 9)
    with pytest.raises(ValueError):
        ops.target_pyramid(images, [257])
    with pytest.raises(ValueError):
        ops.target_pyramid(images, [2], composite=True)       # three channels
    # the entry point itself, on real buffers: refused, and nothing written
    bufs, outs = zip(*[guarded((1, 16, 16, 3)) for _ in range(9)])
    for o in outs:
        o.fill_(-1.0)
    h_out = (C.c_void_p * 9)(*[o.data_ptr() for o in outs])
    stream = torch.cuda.current_stream().cuda_stream
    for ds in ([17], [2] * 9, [257], [1, 17], [1, 0]):
        h_d = (C.c_int32 * len(ds))(*ds)
        st = lib.sixdgs_target_pyramid(images.data_ptr(), 1, 16, 16, 3, 0, None, len(ds), C.cast(h_d, C.c_void_p), C.cast(h_out, C.c_void_p), stream)
        assert st == -1, ds
    torch.cuda.synchronize()
    assert all(bool((o == -1.0).all()) for o in outs) and all(guards_intact(b) for b in bufs)
