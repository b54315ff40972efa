"""Multi-GPU layer: one process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).

The pose loop has no cross-image state (pose_estimation/test.py:46-302), so query images shard
across ranks with NO collective on the data path:
  1. rank 0 broadcasts the Gaussian arrays (236 B per Gaussian: 118 MB at N = 500 k -- far cheaper
     than the 36 B x R rays or 1536 B x R keys derived from them) and the scorer weights;
  2. every rank re-emits the rays and rebuilds its key cache locally (deterministic kernels);
  3. images are split into contiguous blocks, one per rank;
  4. rank 0 gathers c2w[B,4,4] (+ status) once per batch -- a few hundred bytes per image.
The helpers are plain tensor plumbing and also run on CPU tensors with the gloo backend (CI tests).

Ray sharding (SURVEY 8(e) fallback, `score_topk_ray_sharded`): when the key cache of a scene does not fit one GPU
(2 M Gaussians x 256 rays = 512 M rays = 786 GB of key planes) or a single image must be scored by several GPUs, every
rank keeps a contiguous slice of the rays.  The softmax runs over all rays, so the scorer is cut at the row statistics:
two all-reduces of [B,256] floats (max, then the rescaled sum of exponentials) between the two passes and one all-gather
of the per-rank top-k candidates -- a few KB per image, latency-bound, the only collectives on a data path in this build.
"""
from __future__ import annotations

import datetime
import os
from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

_SCENE_FIELDS = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")


_single_rank_group = False     # a process group of ONE rank is in use (SIXDGS_DIST_SINGLE=1): every collective still runs through the backend
_long_group = None             # the group with the long timeout (stages one rank may spend hours in: training); created AND warmed by init_from_env
_long_group_timeout_s = None


def init_from_env(backend: Optional[str] = None, set_device: bool = True) -> Tuple[int, int, int]:
    """(rank, world, local_rank) from RANK / WORLD_SIZE / LOCAL_RANK; initialises the process group when
    WORLD_SIZE > 1 (rendezvous through MASTER_ADDR / MASTER_PORT, 127.0.0.1 on one node).

    SIXDGS_DIST_SINGLE=1: initialise the group at WORLD_SIZE = 1 as well, so that every collective of this module
    (broadcast_scene, broadcast_module, gather_poses, gather_results, merge_row_stats, merge_topk, kth_largest_of_union, agree, ...)
    runs through the backend -- RCCL on device tensors with `nccl` -- on the one GPU of a test box (round 4: the only way to
    execute the RCCL path without a multi-GPU node; tests/test_gpu_rccl_single.py)."""
    global _single_rank_group
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    single = world == 1 and os.environ.get("SIXDGS_DIST_SINGLE") == "1"
    if (world > 1 or single) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend is None:
            backend = os.environ.get("SIXDGS_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        kw = {}
        if backend == "nccl" and set_device:
            torch.cuda.set_device(local)
            # device_id: the default group's communicator is created EAGERLY, bound to this rank's GPU -- a rank whose device is wrong
            # or busy fails here, at init, with every peer at the same point, instead of inside the first collective of an unattended evaluation;
            # later groups (the long-wait one) are split off it
            kw["device_id"] = torch.device("cuda", local)
        # The backend's default timeout (10 min with nccl = RCCL, 30 min with gloo) stays on the default group: a rank that dies between
        # two stages takes its peers down within minutes, not hours.  Only the stage one rank may legitimately spend hours in -- the
        # evaluation sweep trains a missing id_module.th on rank 0 (1500 x 32 steps) while the others wait -- gets a long timeout, on
        # its own group (agree(..., long_wait=True)).  SIXDGS_DIST_TIMEOUT_S overrides the default group's timeout (seconds).
        if os.environ.get("SIXDGS_DIST_TIMEOUT_S"):
            kw["timeout"] = datetime.timedelta(seconds=int(os.environ["SIXDGS_DIST_TIMEOUT_S"]))
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
        # The long-wait group exists -- communicator included -- BEFORE any long stage: with nccl = RCCL a new group's
        # communicator is built lazily on its FIRST collective, where the peers wait for rank 0's unique id in the store under the
        # DEFAULT group's timeout (10 min).  Created inside agree() that first collective came after rank 0's hours of training: the
        # peers timed out in the store long before.  One tiny all-reduce here, while every rank is at the same point, builds it.
        # With nccl and set_device=False the caller pins the device AFTER this call: every rank is still on device 0 here and a collective
        # would put them all on one GPU -- such callers run warm_long_wait_group() themselves once the device is pinned.
        _single_rank_group = single
        if backend == "gloo" or set_device:
            warm_long_wait_group(None if backend == "gloo" else torch.device("cuda", local))
    if single and dist.is_initialized():
        _single_rank_group = True
    return rank, world, local


def is_dist() -> bool:
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _single_rank_group)


def long_wait_group(device=None):
    """The process group for collectives a rank may wait hours in (SIXDGS_DIST_LONG_TIMEOUT_S, default 12 h).  Creating it is COLLECTIVE and ends in
    one 4-byte all-reduce on it (`device`: where, for nccl; default the current device), so that its communicator exists on every rank from then on --
    also when it is re-created because the timeout variable changed (the re-created group used to stay cold, the original bug again).
    init_from_env does this at start-up; a process group initialised elsewhere, or with set_device=False, gets it through warm_long_wait_group()."""
    global _long_group, _long_group_timeout_s
    t = int(os.environ.get("SIXDGS_DIST_LONG_TIMEOUT_S", str(12 * 3600)))
    if _long_group is None or _long_group_timeout_s != t:
        _long_group = dist.new_group(timeout=datetime.timedelta(seconds=t))
        _long_group_timeout_s = t
        dev = "cpu" if dist.get_backend() == "gloo" else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        one = torch.ones(1, dtype=torch.int32, device=dev)
        dist.all_reduce(one, op=dist.ReduceOp.SUM, group=_long_group)
        if int(one.item()) != dist.get_world_size():
            raise RuntimeError(f"6dgs_amd: long-wait group saw {int(one.item())} of {dist.get_world_size()} ranks")
    return _long_group


def warm_long_wait_group(device=None) -> None:
    """Create the long-wait group (first collective included, see long_wait_group) if it does not exist yet.  Collective: every rank calls it at
    the same point -- init_from_env does; callers that pin their device themselves (set_device=False with nccl) call it right after."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    long_wait_group(device)


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block [lo, hi) of `n` items for `rank` (sizes differ by at most one)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def broadcast_scene(scene, src: int = 0, device=None):
    """Rank `src` holds the scene; everyone returns a scene with identical arrays.  One broadcast of the
    shapes, then one per attribute array (xGMI point-to-point: 118 MB at 500 k Gaussians)."""
    from .scene import GaussianScene

    if not is_dist():
        return scene
    rank = dist.get_rank()
    dev = device if device is not None else (scene.device if scene is not None else "cpu")
    meta = torch.zeros(2 + len(_SCENE_FIELDS) * 3, dtype=torch.int64, device=dev)
    if rank == src:
        vals = [scene.max_sh_degree, scene.active_sh_degree]
        for f in _SCENE_FIELDS:
            t = getattr(scene, f)
            shp = list(t.shape) + [1] * (3 - t.dim())
            vals += shp[:3]
        meta = torch.tensor(vals, dtype=torch.int64, device=dev)
    dist.broadcast(meta, src)
    m = meta.tolist()
    out = scene if rank == src else GaussianScene(int(m[0]))
    out.active_sh_degree = int(m[1])
    for i, f in enumerate(_SCENE_FIELDS):
        shp = m[2 + 3 * i: 5 + 3 * i]
        if rank == src:
            t = getattr(scene, f).to(dev).contiguous()
        else:
            nd = {"_xyz": 2, "_scaling": 2, "_rotation": 2, "_opacity": 2}.get(f, 3)
            t = torch.empty(shp[:nd], dtype=torch.float32, device=dev)
        dist.broadcast(t, src)
        setattr(out, f, t)
    return out


def broadcast_module(module: torch.nn.Module, src: int = 0):
    """Same weights on every rank (the reference loads one id_module.th; here rank `src` owns it)."""
    if not is_dist():
        return module
    for t in list(module.parameters()) + list(module.buffers()):
        dist.broadcast(t.data, src)
    return module


def gather_poses(c2w: torch.Tensor, status: Optional[torch.Tensor] = None, dst: int = 0, counts: Optional[list] = None):
    """Per-rank c2w [b_i,4,4] (b_i may differ, 0 included) -> on `dst`: concatenation in rank order; None elsewhere.

    counts: the b_i of ALL ranks when the caller knows them -- it does whenever the images were cut with shard_range, or every rank
    scores the same batch size (bench.py) -- then the call is ONE fixed-size gather to `dst` (north_star: "a final gather") with no
    host synchronisation on the other ranks.  Without counts the sizes are exchanged first (one all_gather of an integer + a host
    read per rank: round 4 paid that on every step)."""
    if not is_dist():
        return c2w, status
    world, rank = dist.get_world_size(), dist.get_rank()
    if counts is None:
        counts = all_counts(int(c2w.shape[0]), c2w.device)
    else:
        counts = [int(c) for c in counts]
        if len(counts) != world or counts[rank] != int(c2w.shape[0]):
            raise RuntimeError(f"6dgs_amd: gather_poses: counts {counts} do not describe rank {rank}'s block of {int(c2w.shape[0])} poses")
    mx = max(counts) if counts else 0
    if mx == 0:
        return (c2w, status) if rank == dst else (None, None)
    payload = torch.zeros(mx, 17, dtype=torch.float32, device=c2w.device)
    payload[: c2w.shape[0], :16] = c2w.reshape(-1, 16)
    if status is not None:
        payload[: c2w.shape[0], 16] = status.float()
    payload = _collective_device(payload)          # gloo moves host memory (a few hundred bytes per image); nccl = RCCL gathers device tensors
    bufs = [torch.empty_like(payload) for _ in range(world)] if rank == dst else None
    dist.gather(payload, bufs, dst=dst)
    if rank != dst:
        return None, None
    allp = torch.cat([b[:c] for b, c in zip(bufs, counts)], dim=0)
    return allp[:, :16].reshape(-1, 4, 4), (allp[:, 16].to(torch.int32) if status is not None else None)


def shard_counts(n: int, world: int) -> list:
    """Block sizes of shard_range(n, r, world) for r = 0 .. world-1 (the `counts` of gather_poses)."""
    return [shard_range(n, r, world)[1] - shard_range(n, r, world)[0] for r in range(world)]


def rank() -> int:
    return dist.get_rank() if is_dist() else 0


def world() -> int:
    return dist.get_world_size() if is_dist() else 1


def all_counts(n: int, device) -> list:
    """One integer per rank -> the list of all of them, in rank order, on every rank."""
    if not is_dist():
        return [int(n)]
    t = torch.tensor([int(n)], dtype=torch.int64, device="cpu" if dist.get_backend() == "gloo" else device)
    bufs = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(bufs, t)
    return [int(b.item()) for b in bufs]


def broadcast_int(value: int, src: int, device) -> int:
    """One integer from rank `src` to every rank."""
    if not is_dist():
        return int(value)
    t = torch.tensor([int(value)], dtype=torch.int64, device="cpu" if dist.get_backend() == "gloo" else device)
    dist.broadcast(t, src)
    return int(t.item())


def gather_results(results: list, dst: int = 0) -> list:
    """Per-rank lists of picklable result records (the dicts of test_pose_estimation) -> on `dst` their concatenation in rank order
    (ranks hold contiguous blocks of the test views, so this is view order); the other ranks keep their own block."""
    if not is_dist():
        return results
    bufs = [None] * dist.get_world_size() if dist.get_rank() == dst else None
    dist.gather_object(results, bufs, dst=dst)
    if dist.get_rank() != dst:
        return results
    return [r for block in bufs for r in block]


def barrier():
    if is_dist():
        dist.barrier()


def agree(fn: Callable, what: str = "", device=None, long_wait: bool = False):
    """Runs the rank-local stage `fn()` (NO collectives inside) and then lets the ranks agree on whether it worked: an all-reduce
    (MAX) of a failure flag.  ANY exception on ANY rank reaches the all-reduce (a FileNotFoundError or KeyError out of a
    loader used to skip it and leave the peers waiting in it): the failing rank re-raises its own exception afterwards, the others
    raise a RuntimeError naming the stage, so that all ranks leave the stage together and the next collectives pair up again.  What
    a sweep SURVIVES stays the caller's decision -- the reference's per-scene `except RuntimeError`
    (pretrain_eval_attention.py:243-244) catches the peers' RuntimeError and the failing rank's own only if it is one.
    long_wait: the stage may take hours on one rank (training on rank 0): its all-reduce runs on the group with the long timeout,
    everything else keeps the backend's default.  Without a process group: plain fn()."""
    err, out = None, None
    try:
        out = fn()
    except Exception as e:              # noqa: BLE001 -- re-raised below, after the ranks have met
        err = e
    if is_dist():
        dev = "cpu" if dist.get_backend() == "gloo" else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        flag = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=long_wait_group() if long_wait else None)
        if int(flag.item()) and err is None:
            raise RuntimeError(f"6dgs_amd: another rank failed during '{what}'; rank {dist.get_rank()} leaves the scene with it")
    if err is not None:
        raise err
    return out


# ---------------------------------------------------------------------------------------------
# data-parallel training (train_id_module(data_parallel=True))
# ---------------------------------------------------------------------------------------------
def sum_gradients(params, logs: torch.Tensor, failed: bool = False, group=None) -> torch.Tensor:
    """The one collective of a data-parallel training iteration: the gradients of `params` (the optimiser's parameters, in its order),
    the logged sums `logs` [n] and a failure flag go into ONE fp32 bucket, which is all-reduced (SUM) on `group` (default: the long-wait
    group -- rank 0 evaluates and checkpoints between two iterations while the others wait here); the summed gradients are written back
    into p.grad.  Returns the summed logs, identical on every rank.

    failed: this rank's window step raised; it contributes zero gradients and zero logs.  A parameter without a gradient (on a rank that
    did not fail) is an error, not a silent zero: it raises the flag too.  When any rank raised the flag, EVERY rank raises RuntimeError
    after the reduce -- the ranks leave the scene together (as agree() makes them do) instead of one waiting in the next collective.
    Without a process group: the gradients stay as they are, and a flag or a missing gradient raises at once."""
    params = list(params)
    missing = [i for i, p in enumerate(params) if p.grad is None]
    logs = logs.detach().reshape(-1)
    dev = logs.device
    bad = bool(failed) or bool(missing)
    if not is_dist():
        if failed:
            raise RuntimeError("6dgs_amd: the window step failed")
        if missing:
            raise RuntimeError(f"6dgs_amd: sum_gradients: parameters {missing} of the optimiser have no gradient")
        return logs
    parts = [torch.zeros(p.numel(), dtype=torch.float32, device=dev) if bad else p.grad.detach().reshape(-1).to(device=dev, dtype=torch.float32)
             for p in params]
    parts.append(torch.zeros_like(logs, dtype=torch.float32) if bad else logs.to(torch.float32))
    parts.append(torch.full((1,), 1.0 if bad else 0.0, dtype=torch.float32, device=dev))
    bucket = _collective_device(torch.cat(parts))
    dist.all_reduce(bucket, op=dist.ReduceOp.SUM, group=long_wait_group() if group is None else group)
    if float(bucket[-1]) > 0:
        if missing and not failed:
            raise RuntimeError(f"6dgs_amd: sum_gradients: parameters {missing} of the optimiser have no gradient on rank {dist.get_rank()}")
        raise RuntimeError(f"6dgs_amd: a training window step failed on {int(float(bucket[-1]))} rank(s); rank {dist.get_rank()} leaves the scene with it")
    off = 0
    for p in params:
        n = p.numel()
        p.grad.copy_(bucket[off: off + n].view_as(p.grad))
        off += n
    return bucket[off: off + logs.numel()].to(dev)


def broadcast_tensor(t: Optional[torch.Tensor], src: int, device, dtype=torch.float32, shape=None, group=None) -> torch.Tensor:
    """A tensor of rank `src` (1-D or 2-D; `t` is ignored elsewhere) on every rank, on `device`.  shape None: the shape is broadcast first,
    so the other ranks need not know it; otherwise every rank passes the same `shape`.  Default group: the long-wait one (data-parallel
    training: rank 0 may be evaluating while the others wait here)."""
    if not is_dist():
        return t
    g = long_wait_group() if group is None else group
    host = dist.get_backend() == "gloo"
    if shape is None:
        meta = torch.zeros(3, dtype=torch.int64, device="cpu" if host else device)
        if dist.get_rank() == src:
            shp = list(t.shape)
            if len(shp) not in (1, 2):
                raise RuntimeError(f"6dgs_amd: broadcast_tensor takes 1-D or 2-D tensors (got {tuple(t.shape)})")
            meta = torch.tensor([len(shp)] + shp + [0] * (2 - len(shp)), dtype=torch.int64, device=meta.device)
        dist.broadcast(meta, src, group=g)
        nd, shp = int(meta[0]), [int(x) for x in meta[1:]]
        shape = shp[:nd]
    if dist.get_rank() == src:
        buf = t.detach().to(dtype).contiguous()
        buf = buf.cpu() if host else buf.to(device)
    else:
        buf = torch.empty(shape, dtype=dtype, device="cpu" if host else device)
    dist.broadcast(buf, src, group=g)
    return buf.to(device)


def backend_name() -> str:
    """"nccl" (= RCCL on ROCm) / "gloo" when a process group is up, "none" for a single process."""
    return dist.get_backend() if is_dist() else "none"


def ranks_seen(device) -> int:
    """How many ranks take part in the collectives: an all-reduce (sum) of ones over the process group -- over RCCL on
    device memory when the backend is nccl.  1 without a process group."""
    if not is_dist():
        return 1
    one = torch.ones(1, dtype=torch.float32, device=device if dist.get_backend() != "gloo" else "cpu")
    dist.all_reduce(one, op=dist.ReduceOp.SUM)
    return int(round(float(one.item())))


def max_over_ranks(x: float, device) -> float:
    if not is_dist():
        return x
    t = torch.tensor([x], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def all_floats(x: float, device) -> list:
    """One float of every rank, in rank order, on every rank (bench.py: each rank's own time next to the max -- which GPU of an 8-GPU node is the slow one)."""
    if not is_dist():
        return [float(x)]
    t = torch.tensor([x], dtype=torch.float64, device=device if dist.get_backend() != "gloo" else "cpu")
    bufs = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(bufs, t)
    return [float(b.item()) for b in bufs]


# ---------------------------------------------------------------------------------------------
# ray-sharded scoring
# ---------------------------------------------------------------------------------------------
def _collective_device(t: torch.Tensor) -> torch.Tensor:
    """gloo moves host memory: tiny tensors take the detour through the CPU; nccl (RCCL) reduces device tensors in place."""
    return t.cpu() if (t.is_cuda and dist.get_backend() == "gloo") else t


def merge_row_stats(stats: torch.Tensor, group=None) -> torch.Tensor:
    """Local (max, sumexp) [B,T,2] of every rank's ray slice -> the statistics over all rays, identical on every rank:
    M = max_g m_g;  S = sum_g s_g * exp(m_g - M).  Rows without rays anywhere stay (-inf, 0)."""
    if not is_dist():
        return stats
    dev = stats.device
    m = _collective_device(stats[..., 0].contiguous())
    sl = _collective_device(stats[..., 1].contiguous())
    mg = m.clone()
    dist.all_reduce(mg, op=dist.ReduceOp.MAX, group=group)
    scale = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), torch.exp(m - mg))
    sg = sl * scale
    dist.all_reduce(sg, op=dist.ReduceOp.SUM, group=group)
    return torch.stack([mg, sg], dim=-1).to(dev)


def merge_topk(idx_local: torch.Tensor, val: torch.Tensor, ray_offset: int, k: int, group=None):
    """Per-rank top-k candidates (indices local to the rank's ray slice, -1 / NaN padded) -> the global top-k on every
    rank, ordered like the single-GPU kernel: value descending, ties by the lower global ray index."""
    gidx = torch.where(idx_local >= 0, idx_local + int(ray_offset), idx_local)
    if is_dist() and group is not False:           # group=False: merge the given candidates locally (streamed scoring)
        world = dist.get_world_size(group)
        dev = idx_local.device
        gi, gv = _collective_device(gidx.contiguous()), _collective_device(val.contiguous())
        bi = [torch.empty_like(gi) for _ in range(world)]
        bv = [torch.empty_like(gv) for _ in range(world)]
        dist.all_gather(bi, gi, group=group)
        dist.all_gather(bv, gv, group=group)
        gidx, val = torch.cat(bi, dim=1).to(dev), torch.cat(bv, dim=1).to(dev)
    pad = gidx < 0
    key = torch.where(pad, torch.full_like(val, -float("inf")), val)
    big = torch.iinfo(torch.int64).max
    order = torch.argsort(torch.where(pad, torch.full_like(gidx, big), gidx), dim=1, stable=True)      # index ascending ...
    key, gidx, val = key.gather(1, order), gidx.gather(1, order), val.gather(1, order)
    order = torch.argsort(key, dim=1, descending=True, stable=True)[:, :k]                            # ... then value descending, stable
    return gidx.gather(1, order), val.gather(1, order)


def score_topk_ray_sharded(q: torch.Tensor, n_tok: torch.Tensor, key: Optional[torch.Tensor], ray_offset: int, topk: int = 100,
                           key_planes: Optional[torch.Tensor] = None, key_scale: Optional[torch.Tensor] = None, want_scores: bool = False,
                           workspace: Optional[torch.Tensor] = None, group=None):
    """Exact scorer over a ray set that is split across the ranks of `group`; this rank holds rays
    [ray_offset, ray_offset + r_local).  Returns (global idx [B,k], val [B,k], local scores [B,r_local] | None), the first two
    identical on every rank and equal to the single-GPU result up to the rounding of the sum of exponentials."""
    from . import ops

    r_local = key.shape[0] if key is not None else key_planes.shape[0]
    b = q.shape[0]
    if workspace is None:
        workspace = torch.empty(ops.score_topk_workspace_bytes(r_local, b, topk), dtype=torch.uint8, device=q.device)
    local = ops.score_pass1(q, n_tok, key, workspace, topk, key_planes=key_planes, key_scale=key_scale)
    glob = merge_row_stats(local, group)
    idx, val, scores = ops.score_pass2(glob, n_tok, r_local, workspace, topk, used_planes=key_planes is not None, want_scores=want_scores)
    gidx, gval = merge_topk(idx, val, ray_offset, topk, group)
    return gidx, gval, scores


def kth_largest_of_union(val_local: torch.Tensor, k: int, group=None) -> torch.Tensor:
    """Per-rank descending top-k value lists [B,k] (NaN-padded) -> the k-th largest value of their union, per image [B] (the
    union of the shards' top-k lists contains the scene's top-k as a multiset).  -inf where the union holds fewer than k values."""
    v = val_local
    if is_dist() and group is not False:
        world = dist.get_world_size(group)
        c = _collective_device(v.contiguous())
        bufs = [torch.empty_like(c) for _ in range(world)]
        dist.all_gather(bufs, c, group=group)
        v = torch.cat(bufs, dim=1).to(val_local.device)
    v = torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v)
    return torch.sort(v, dim=1, descending=True).values[:, k - 1].contiguous()


def _all_reduce(t: torch.Tensor, op, group=None) -> torch.Tensor:
    if not is_dist():
        return t
    c = _collective_device(t.contiguous())
    dist.all_reduce(c, op=op, group=group)
    if c is not t:
        t.copy_(c.to(t.device))
    return t


def score_select_ray_sharded(q: torch.Tensor, n_tok: torch.Tensor, key_planes: torch.Tensor, key_scale: torch.Tensor, sample_planes: torch.Tensor,
                             sample_scale: torch.Tensor, ray_offset: int, r_total: int, r_sample_total: int, topk: int = 100,
                             max_candidates: Optional[int] = None, n_tok_host=None, profile=None, group=None, key_norm: Optional[torch.Tensor] = None):
    """The select path (top-k without materialised logits, include/sixdgs.h: sixdgs_score_select) over a scene whose key planes are
    split across the ranks of `group`; this rank holds the planes of rays [ray_offset, ray_offset + r_local) and of ITS share of the
    ray sample.  Per image and batch the ranks exchange: the sample's row statistics (2 all-reduces of 1 KB), the exact per-token
    sums g_t after the sweep (1 all-reduce of 1 KB), the largest key norm (4 B), their k largest U (all-gather of k floats), the
    statuses (4 B) and the per-rank exact top-k candidates (all-gather of k (index, value) pairs) -- a few KB, latency-bound; the
    matrix-core sweep itself runs on local planes only.

    Returns (global idx [B,k], val [B,k], status [B] host list): the first two identical on every rank and equal to the single-GPU
    select answer up to the rounding of the per-token sums (the same 100 rays, values <= 2e-6); status[b] = candidates examined over
    all ranks, or -1 when some rank could not decide image b (too many candidates / exponent overflow) -- the caller then scores
    those images with score_topk_ray_sharded (all ranks take that decision together: the status is all-reduced)."""
    from . import ops

    r_local = key_planes.shape[0]
    cmax = ops.SELECT_MAX_CANDIDATES if max_candidates is None else int(max_candidates)
    with ops.arena_scope():      # U and the stage workspace of this batch go back to the arena (if one is installed) when the batch is enqueued
        ss = ops.SelectStream(q, n_tok, r_local, topk, cmax, n_tok_host)
        stats = merge_row_stats(ss.sample_stats(sample_planes, sample_scale), group)             # identical ctok on every rank
        ss.prepare(stats, r_sample_total, r_total)
        if key_norm is not None:                    # max |k_r| of the local planes, kept beside them (otherwise: one more pass over the planes)
            ss.key_norm.copy_(key_norm)
        ss.sweep(key_planes, key_scale, 0, profile, update_norm=key_norm is None)
        _all_reduce(ss.gsum, dist.ReduceOp.SUM, group)                                            # exact g_t over ALL rays
        _all_reduce(ss.key_norm, dist.ReduceOp.MAX, group)
        # U_(k) of the scene from the ranks' exact k largest U.  (The single-GPU path takes a lower bound from the tile maxima of U and repairs the
        # rare image whose top rays sit in a few tiles on the device; here that repair would be a second round of collectives, and six passes over
        # the local U are 1 % of a rank's sweep.)
        uk = kth_largest_of_union(ss.topk_u(exact=True), min(topk, r_total), group)
        cand, count = ss.candidates(uk=uk)
        idx, val, status = ss.rescore(key_planes, key_scale, cand, count, compact=False, allow_fewer=True)
        st = status.to(torch.int64)
        bad = _all_reduce((st < 0).to(torch.int64), dist.ReduceOp.MAX, group) if is_dist() else (st < 0).to(torch.int64)
        tot = _all_reduce(st.clamp(min=0), dist.ReduceOp.SUM, group) if is_dist() else st.clamp(min=0)
    gidx, gval = merge_topk(idx, val, ray_offset, topk, group)
    out_status = torch.where(bad > 0, torch.full_like(tot, -1), tot).tolist()
    for b, v in enumerate(out_status):
        if v < 0:
            gidx[b], gval[b] = -1, float("nan")
    return gidx, gval, out_status


def gather_selected_rays(gidx: torch.Tensor, ori_local: torch.Tensor, dir_local: torch.Tensor, ray_offset: int, group=None):
    """Global ray indices [B,k] (-1 = none) of a ray-sharded scene -> (ori [B,k,3], dir [B,k,3]) on every rank: each rank fills in
    the rays it owns, one all-reduce (SUM) of 6 floats per selected ray puts them together (every index has exactly one owner)."""
    r_local = ori_local.shape[0]
    loc = gidx - int(ray_offset)
    mine = (gidx >= 0) & (loc >= 0) & (loc < r_local)
    safe = torch.where(mine, loc, torch.zeros_like(loc))
    if r_local == 0:       # a rank whose ray slice is empty owns no selected ray (found by the 8-rank rehearsal: indexing an empty slice raised)
        both = torch.zeros(*gidx.shape, 6, dtype=ori_local.dtype, device=ori_local.device)
    else:
        both = torch.cat([ori_local[safe], dir_local[safe]], dim=-1) * mine[..., None].to(ori_local.dtype)
    if is_dist() and group is not False:
        _all_reduce(both, dist.ReduceOp.SUM, group)
    return both[..., :3].contiguous(), both[..., 3:].contiguous()
