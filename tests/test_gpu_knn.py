"""sixdgs_knn_mean_dist2 on the GPU against the fp32 brute force of tests/knn_reference.py, BIT FOR BIT: every size at which the
search takes another path (around a wave, a box, several boxes, the sort's block sizes), clouds that stress the box bound (clusters
with far outliers, flat and degenerate clouds, a lattice, duplicates, identical points, a large offset, anisotropy), permutation,
repeatability across calls and streams, one large cloud against the same brute force run by torch on the GPU, and the argument and
workspace errors.  Every output buffer carries guard elements behind n that must survive.  Everything runs inside this process."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as K  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD, SENTINEL = 64, -12345.0
BADARG, WORKSPACE = -1, -2
with open(os.path.join(ROOT, "6dgs_amd", "csrc", "knn_rules.h")) as _f:
    BOX = int(re.search(r"constexpr int kBox = (\d+);", _f.read()).group(1))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("6dgs_amd._lib").load()


@pytest.fixture(scope="module")
def ops(lib):
    return importlib.import_module("6dgs_amd.ops")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def run(lib, p, stream=None):
    """The raw call on a cloud (numpy or a GPU tensor) into a guarded buffer -> numpy float32 [n]."""
    x = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p, F)).cuda()
    n = x.shape[0]
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        out = torch.full((n + GUARD,), SENTINEL, device="cuda")
        need = lib.sixdgs_knn_workspace_bytes(n)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        status = lib.sixdgs_knn_mean_dist2(n, x.data_ptr(), out.data_ptr(), ws.data_ptr(), need, C.c_void_p(s.cuda_stream))
        assert status == 0, status
        got = out.cpu().numpy()
    assert np.all(got[n:] == F(SENTINEL)), "the guard behind n was written"
    return got[:n]


@pytest.mark.parametrize("name", sorted(K.cases(BOX)))
def test_every_case_of_the_table_is_bit_equal_to_brute_force(lib, name):
    p, want = K.case(name, BOX)
    got = run(lib, p)
    wrong = bits(got) != bits(want)
    assert not wrong.any(), (int(wrong.sum()), got[wrong][:4], want[wrong][:4])
    if name == "lattice":
        assert np.all(got == F(1.0))
    if name in ("duplicated", "identical600", "identical8193"):
        assert np.all(got == F(0.0))


def test_permuting_the_input_permutes_the_output(lib):
    p, want = K.case("clustered", BOX)
    perm = np.random.default_rng(9).permutation(p.shape[0])
    assert np.array_equal(bits(run(lib, p[perm])), bits(want[perm]))


def test_same_bytes_on_a_second_call_and_a_second_stream(lib, ops):
    p, want = K.case("uniform8193", BOX)
    x = torch.from_numpy(np.array(p)).cuda()
    first = run(lib, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert np.array_equal(bits(first), bits(want)) and np.array_equal(bits(run(lib, x)), bits(first))
    assert np.array_equal(bits(run(lib, x, side)), bits(first))
    # the wrapper: its own workspace, and a caller's that is larger than needed
    assert np.array_equal(bits(ops.knn_mean_dist2(x).cpu().numpy()), bits(first))
    ws = torch.empty(ops.knn_workspace_bytes(8193) + 4096, dtype=torch.uint8, device="cuda")
    assert np.array_equal(bits(ops.knn_mean_dist2(x, workspace=ws).cpu().numpy()), bits(first))
    assert ops.knn_mean_dist2(torch.zeros(0, 3, device="cuda")).shape == (0,)


def test_large_cloud_against_the_brute_force_on_the_gpu(lib):
    """n = 100 001 (391 boxes, well above 4 sort blocks of rocPRIM) on the clustered cloud with its outliers, against brute_torch run on
    the same GPU: separate elementwise kernels, so unfused by construction."""
    x = torch.from_numpy(K.clustered(100001, seed=1)).cuda()
    want = K.brute_torch(x, chunk=512)
    got = run(lib, x)
    wrong = bits(got) != bits(want)
    assert not wrong.any(), (int(wrong.sum()), got[wrong][:4], want[wrong][:4])


def test_argument_and_workspace_errors(lib):
    n = 1000
    x = torch.zeros(n + 1, 3, device="cuda")
    out = torch.full((n + GUARD,), SENTINEL, device="cuda")
    need = lib.sixdgs_knn_workspace_bytes(n)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    call, s = lib.sixdgs_knn_mean_dist2, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, op, wp = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert wp % 256 == 0
    for m in (1, 2, 3, -1, 2 ** 31):
        assert call(m, xp, op, wp, need + 256, s) == BADARG
    assert [lib.sixdgs_knn_workspace_bytes(m) for m in (0, 1, 2, 3, 2 ** 31)] == [0] * 5
    assert call(0, None, None, None, 0, s) == 0
    assert call(n, None, op, wp, need, s) == BADARG and call(n, xp, None, wp, need, s) == BADARG and call(n, xp, op, None, need, s) == BADARG
    assert call(n, xp + 2, op, wp, need, s) == BADARG and call(n, xp, op + 2, wp, need, s) == BADARG and call(n, xp, op, wp + 64, need, s) == BADARG
    assert call(n, xp, xp, wp, need, s) == BADARG and call(n, xp, xp + 12 * n - 4, wp, need, s) == BADARG
    assert call(n, xp + 4 * n - 4, xp, wp, need, s) == BADARG
    assert call(n, xp, op, wp, need - 1, s) == WORKSPACE and call(n, xp, op, wp, 0, s) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote its output"
    assert call(n, xp, op, wp, need, s) == 0                                  # and the exact size is enough
    torch.cuda.synchronize()
    assert bool((out[:n] == 0).all()) and bool((out[n:] == SENTINEL).all())
