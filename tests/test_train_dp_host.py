"""Data-parallel window training without a GPU: the ray-split scorer-backward ABI entries (header, binding, library), the one
collective of an iteration (distributed.sum_gradients) over two gloo ranks on CPU tensors, and the refusals of
train_id_module(data_parallel=True)."""
import ctypes
import importlib
import os
import re
import socket
import sys

import pytest

torch = pytest.importorskip("torch")
mp = pytest.importorskip("torch.multiprocessing")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sixdgs_score_backward_split", "sixdgs_score_backward_split_workspace_bytes")


def test_split_backward_symbols_are_declared_bound_and_exported():
    lib = importlib.import_module("6dgs_amd._lib")
    with open(os.path.join(ROOT, "include", "sixdgs.h")) as f:
        header = f.read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(so, name), f"{name} is not exported by {lib.LIB_PATH}"
    assert lib.ABI_VERSION >= 9


def test_split_workspace_sizes():
    """G = 1, and every G that clamps to 1 (R <= 128 rays), needs only the unsplit workspace; G > 1 adds G x B x 256 x (2 + 384) floats;
    G beyond the 128-ray tiles clamps; a negative G asks for nothing (the call refuses it).  Explicit G: no device query."""
    L = importlib.import_module("6dgs_amd._lib").load()
    base = L.sixdgs_score_backward_workspace_bytes(3)
    assert L.sixdgs_score_backward_split_workspace_bytes(3, 28691, 1) == base
    assert L.sixdgs_score_backward_split_workspace_bytes(3, 17, 8) == base
    assert L.sixdgs_score_backward_split_workspace_bytes(3, 300, 3) == base + 3 * 3 * 256 * 386 * 4
    assert L.sixdgs_score_backward_split_workspace_bytes(3, 300, 8) == base + 3 * 3 * 256 * 386 * 4      # 300 rays = 3 tiles
    assert L.sixdgs_score_backward_split_workspace_bytes(3, 300, -1) == 0


def test_split_backward_refuses_negative_groups_without_touching_memory():
    L = importlib.import_module("6dgs_amd._lib").load()
    assert L.sixdgs_score_backward_split(None, None, 1, None, 300, None, None, None, None, -1, None, 0, None) != 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params(rank):
    gen = torch.Generator().manual_seed(100 + rank)
    ps = [torch.nn.Parameter(torch.zeros(7, 5)), torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2, 2))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen)
    return ps


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dd = importlib.import_module("6dgs_amd.distributed")
        train = importlib.import_module("6dgs_amd.train")
        dd.init_from_env("gloo")
        out = {}
        # 1. the sums of the gradients and of the logs
        ps = _params(rank)
        logs = torch.tensor([1.5, 0.25, -3.0]) * (rank + 1)
        got = dd.sum_gradients(ps, logs)
        out["grads"] = [p.grad.numpy().copy() for p in ps]       # numpy: pickled by value through the queue
        out["logs"] = got.numpy().copy()
        # 2. a flag raised on rank 1 only: both ranks raise, in the same call
        ps = _params(rank)
        try:
            dd.sum_gradients(ps, torch.zeros(3), failed=rank == 1)
            out["flag"] = "no error"
        except RuntimeError as e:
            out["flag"] = str(e)
        # 3. a parameter without a gradient on rank 0: refused on both ranks
        ps = _params(rank)
        if rank == 0:
            ps[1].grad = None
        try:
            dd.sum_gradients(ps, torch.zeros(3))
            out["missing"] = "no error"
        except RuntimeError as e:
            out["missing"] = str(e)
        # 4. the collectives still pair up after the refusals
        ps = _params(rank)
        out["after"] = dd.sum_gradients(ps, torch.ones(3)).numpy().copy()
        # 5. more ranks than images per iteration
        try:
            train.train_id_module("unused.th", "cpu", None, None, None, "seq", "cat", gradient_accumulation_steps=1, batched_window=True,
                                  data_parallel=True)
            out["world"] = "no error"
        except ValueError as e:
            out["world"] = "ValueError: " + str(e)
        q.put((rank, out))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc()))


@pytest.mark.timeout(300)
def test_sum_gradients_two_gloo_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert not isinstance(res[r], str), res[r]
    a, b = res[0], res[1]
    want = [g0 + g1 for g0, g1 in zip((p.grad for p in _params(0)), (p.grad for p in _params(1)))]
    for ga, gb, w in zip(a["grads"], b["grads"], want):
        assert torch.equal(torch.from_numpy(ga), w) and torch.equal(torch.from_numpy(gb), w)
        assert ga.tobytes() == gb.tobytes()
    assert a["logs"].tolist() == [4.5, 0.75, -9.0] and a["logs"].tobytes() == b["logs"].tobytes()
    assert "failed" in a["flag"] and "failed" in b["flag"]
    assert "no gradient" in a["missing"] and "1 rank" in b["missing"]
    assert a["after"].tolist() == [2.0, 2.0, 2.0] and b["after"].tolist() == [2.0, 2.0, 2.0]
    assert a["world"].startswith("ValueError") and b["world"].startswith("ValueError")


def test_sum_gradients_without_a_process_group():
    dd = importlib.import_module("6dgs_amd.distributed")
    ps = _params(0)
    ref = [p.grad.clone() for p in ps]
    logs = torch.tensor([1.0, 2.0, 3.0])
    assert torch.equal(dd.sum_gradients(ps, logs), logs)
    assert all(torch.equal(p.grad, r) for p, r in zip(ps, ref))
    ps[2].grad = None
    with pytest.raises(RuntimeError, match="no gradient"):
        dd.sum_gradients(ps, logs)
    with pytest.raises(RuntimeError):
        dd.sum_gradients(_params(0), logs, failed=True)


def test_data_parallel_needs_the_batched_window():
    train = importlib.import_module("6dgs_amd.train")
    with pytest.raises(ValueError, match="batched_window"):
        train.train_id_module("unused.th", "cpu", None, None, None, "seq", "cat", data_parallel=True)
    with pytest.raises(ValueError, match="backward_ray_groups"):
        train.train_id_module("unused.th", "cpu", None, None, None, "seq", "cat", batched_window=True, backward_ray_groups=-1)
