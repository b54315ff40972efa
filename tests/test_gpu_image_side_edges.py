"""GPU tests of the image side's entry kernels (6dgs_amd/csrc/vit.hip: sixdgs_image_prep, sixdgs_u8_to_planar, sixdgs_im2col) at the
shapes where they change path.  Run with `-m gpu` on an MI355X; everything runs in this process.

sixdgs_image_prep is held to tests/image_prep_reference.py in fp64 -- written from the operation's definition, vetted against PyTorch's
CPU op and against csrc/image_prep_rules.h by tests/test_image_prep_host.py -- under the bound that module forms from its own fp32
evaluation.  The case table lives there; every case names its branch:
  band heights rb = 8 / 4 / 2 / 1 ............ band_* (batch and the LDS budget decide; the plan's rb is asserted on the CPU)
  spans clipped at the image's edge .......... border_*, corner_*
  one axis up, one down; an identity axis .... mixed_up_down, identity_rows
  ragged last band, S % 4 != 0, S > 256 ...... out_1, out_37, out_221, out_448, out_518
  images that start off a dword .............. bytes_mod1, bytes_mod2 (last row and column in the crop: taps at the buffer's end)
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import image_prep_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64                      # floats = 256 bytes on either side of out
SENTINEL = -12345.5
BADARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd.ops")


@pytest.fixture(scope="module")
def lib(ops):
    return importlib.import_module("6dgs_amd._lib").load()


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_prep(lib, u8, tab, resized_h, resized_w, top, left, out_size, images_ptr=None, batch=None, mean=R.MEAN, std=R.STD):
    """sixdgs_image_prep through the C call on a guarded output -> (status, out [B][3][S][S] or the untouched body, guards intact)."""
    b, h, w, _ = u8.shape
    n = b * 3 * out_size * out_size
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device="cuda")
    body = buf[GUARD:GUARD + n]
    st = lib.sixdgs_image_prep(C.c_void_p(u8.data_ptr() if images_ptr is None else images_ptr), b if batch is None else batch, h, w, C.c_void_p(tab.data_ptr()),
                               resized_h, resized_w, top, left, out_size, f3(mean), f3(std), C.c_void_p(body.data_ptr()), _stream())
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return st, body.view(b, 3, out_size, out_size), intact


def run_case(lib, d, images=None):
    c = d["case"]
    u8 = G(d["u8"]) if images is None else images
    return raw_prep(lib, u8, G(d["table"]), c.resized_h, c.resized_w, c.crop_top, c.crop_left, c.out_size)


# =====================================================================================================
# sixdgs_image_prep
# =====================================================================================================
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_image_prep_case_against_fp64(ops, lib, name):
    """Every case of the table: status 0, the 256 guard bytes on both sides of out intact, |gpu - r64| within the case's bound; where the
    geometry is one ops.image_prep produces, also within 5e-6 of PyTorch's GPU op (resize of the table's values to (resized_h, resized_w),
    slice, normalise) -- the yardstick of test_image_prep_against_the_transform_pipeline_it_replaces on these shapes."""
    d = R.case_data(name)
    c = d["case"]
    assert d["fit"]
    st, out, intact = run_case(lib, d)
    assert st == 0 and intact
    assert not bool((out == SENTINEL).any()) and bool(torch.isfinite(out).all())
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - d["r64"]).max())
    line = f"[image_prep] gpu case {name}: err={err:.3g} bound={d['bound']:.3g} err/bound={err / d['bound']:.3g} y={d['y']:.3g} scale={d['scale']:.4g}"
    e_op = None
    if R.op_geometry(c, ops.image_prep_geometry):
        values = G(d["table"])[G(d["u8"]).long()].permute(0, 3, 1, 2)
        resized = torch.nn.functional.interpolate(values, size=(c.resized_h, c.resized_w), mode="bicubic", antialias=True, align_corners=False)
        crop = resized[:, :, c.crop_top:c.crop_top + c.out_size, c.crop_left:c.crop_left + c.out_size]
        ref_op = (crop - G(R.MEAN).view(1, 3, 1, 1)) / G(R.STD).view(1, 3, 1, 1)
        e_op = float((out - ref_op).abs().max())
        line += f" vs the GPU op={e_op:.3g}"
    print(line)
    assert err <= d["bound"], line
    assert e_op is None or e_op <= 5e-6, line


def test_the_op_geometry_anchor_is_used():
    """The second anchor is no empty set: the whole-resize downscale and every output-size case have the geometry ops.image_prep produces."""
    geometry = importlib.import_module("6dgs_amd.ops").image_prep_geometry
    anchored = {c.name for c in R.CASES if R.op_geometry(c, geometry)}
    assert {"border_down", "out_1", "out_37", "out_221", "out_448", "out_518"} <= anchored


@pytest.mark.parametrize("name", ("band_b10_h300", "band_b10_h1002", "band_b10_h1003", "bytes_mod1", "bytes_mod2"))
def test_images_do_not_mix_and_the_band_height_is_invisible(lib, name):
    """Nothing in an item's arithmetic depends on the band height or on the image's place in the batch: every image run alone (batch 1:
    4-row bands where the batch of 10 takes 8-row ones; a dword-aligned buffer of its own where the odd-sized batch's images start off a
    dword) gives the bits of its slice of the batch, and a second call on the batch gives the same bytes."""
    d = R.case_data(name)
    u8 = G(d["u8"])
    st, out, intact = run_case(lib, d)
    assert st == 0 and intact
    st2, again, intact2 = run_case(lib, d)
    assert st2 == 0 and intact2 and torch.equal(out, again)
    for i in range(d["case"].batch):
        one = u8[i:i + 1].clone()
        assert one.data_ptr() % 4 == 0
        st1, alone, intact1 = run_case(lib, d, images=one)
        assert st1 == 0 and intact1
        assert torch.equal(alone[0], out[i]), (name, i, float((alone[0] - out[i]).abs().max()))


def test_image_prep_refusals_touch_nothing(ops, lib):
    """SIXDGS_E_UNSUPPORTED for 2151 x 260 to 256 x 256 (no band fits the LDS budget) and 260 x 4000 to 256 x 256 (more than 64 taps), out
    and its guards untouched; ops.image_prep answers None for a 2151 x 2151 image at the default geometry (the shape the default Resize(256)
    turns into that very plan; a 2151 x 260 image would be resized to 2117 x 256 there, which the kernel takes); batch 0 is 0; every
    argument the entry point checks is SIXDGS_E_BADARG."""
    tab = G(R.table("div255"))
    for b, h, w, nh, nw, top, left, s in R.UNSUPPORTED:
        u8 = torch.zeros(b, h, w, 3, dtype=torch.uint8, device="cuda")
        st, out, intact = raw_prep(lib, u8, tab, nh, nw, top, left, s)
        assert st == UNSUPPORTED and intact and bool((out == SENTINEL).all()), (h, w, st)
    square = torch.zeros(1, 2151, 2151, 3, dtype=torch.uint8, device="cuda")
    assert ops.image_prep(square, tab, R.MEAN, R.STD) is None
    assert ops.image_prep(square[:, :2150, :2150], tab, R.MEAN, R.STD) is not None
    u8 = torch.zeros(2, 40, 40, 3, dtype=torch.uint8, device="cuda")

    def status(**kw):
        args = dict(resized_h=32, resized_w=32, top=4, left=4, out_size=24)
        args.update(kw)
        st, out, intact = raw_prep(lib, u8, tab, **args)
        assert intact and bool((out == SENTINEL).all())
        return st

    assert status(batch=0) == 0
    assert status(batch=0, images_ptr=0) == 0
    assert status(top=9) == BADARG and status(left=9) == BADARG and status(top=-1) == BADARG and status(out_size=33, top=0, left=0) == BADARG
    assert status(images_ptr=0) == BADARG
    assert status(images_ptr=u8.data_ptr() + 1) == BADARG and status(images_ptr=u8.data_ptr() + 2) == BADARG
    assert status(batch=65536) == BADARG
    n = 2 * 3 * 24 * 24
    out = torch.full((n,), SENTINEL, device="cuda")
    P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                      # noqa: E731
    call = lambda images, table, mean, std, o: lib.sixdgs_image_prep(P(images), 2, 40, 40, P(table), 32, 32, 4, 4, 24, mean, std, P(o), _stream())   # noqa: E731
    assert call(u8, None, f3(R.MEAN), f3(R.STD), out) == BADARG
    assert call(u8, tab, None, f3(R.STD), out) == BADARG and call(u8, tab, f3(R.MEAN), None, out) == BADARG
    assert call(u8, tab, f3(R.MEAN), f3(R.STD), None) == BADARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(u8, tab, f3(R.MEAN), f3(R.STD), out) == 0                            # and the same call with everything in place runs
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# =====================================================================================================
# sixdgs_u8_to_planar
# =====================================================================================================
@pytest.mark.parametrize("shape", ((3, 2, 2, 3), (1, 2048, 4096, 3), (1, 2049, 4096, 3), (14, 800, 800, 3)))
def test_u8_to_planar_at_its_grid_cap(ops, shape):
    """The smallest shape (one group of four pixels per image); exactly 8192 x 256 groups (the capped grid, each thread one group); one
    image row more (the grid-stride loop comes round a second time); 14 images of 800 x 800 (a little over one trip, several images): each
    equal to table[byte] exactly, with the random table."""
    g = torch.Generator(device="cuda").manual_seed(shape[0] * 31 + shape[1])
    u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8, device="cuda")
    tab = G(R.table("random"))
    planar = ops.u8_to_planar(u8, tab)
    assert planar.shape == (shape[0], 3, shape[1], shape[2])
    assert torch.equal(planar.permute(0, 2, 3, 1), tab[u8.long()])


# =====================================================================================================
# sixdgs_im2col
# =====================================================================================================
def test_im2col_scalar_fallback_off_a_16_byte_boundary(ops):
    """A taps-major map with channel-contiguous input and C a multiple of 4 takes 16-byte copies -- unless its base pointer is off a
    16-byte boundary (here by one float: a storage offset of 1), which sends it through the scalar kernel: same result as the vector
    path on an aligned copy, and as unfold."""
    b, c, h, w, k = 2, 8, 6, 7, 3
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(b, c, h, w, generator=g).cuda()
    ref = torch.nn.functional.unfold(x, k).transpose(1, 2).reshape(b * (h - k + 1) * (w - k + 1), c * k * k)
    tm = ref.view(-1, c, k * k).transpose(1, 2).reshape(ref.shape[0], -1)              # columns (ky, kx, c)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    aligned = nhwc.permute(0, 3, 1, 2)
    store = torch.zeros(b * h * w * c + 4, device="cuda")
    assert store.data_ptr() % 16 == 0
    store[1:1 + b * h * w * c] = nhwc.reshape(-1)
    shifted = store[1:1 + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.stride(1) == 1 and torch.equal(shifted, aligned)
    vec, scalar = ops.im2col(aligned, k, taps_major=True), ops.im2col(shifted, k, taps_major=True)
    assert torch.equal(vec, tm) and torch.equal(scalar, tm) and torch.equal(scalar, vec)
    assert bool((store[0] == 0).all()) and bool((store[1 + b * h * w * c:] == 0).all())
