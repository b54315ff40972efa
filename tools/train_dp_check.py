"""Data-parallel window training check (run under torch.distributed.run, any world size <= 4; tests/test_gpu_train_dp.py launches it
with two gloo ranks on one GPU; on a multi-GPU node run it over RCCL: --backend nccl).

1. Gradients of one iteration: 32 draws from 6 views with a pinned image side and 3000 rays (the set-up of
   tests/test_gpu_train_window.py::test_window_equals_the_per_image_loop).  Rank r runs train.window_step_loss on its block
   dd.shard_range(32, r, world) of the draws with the global divisor 32 and the auto-split scorer backward, and dd.sum_gradients adds
   the ranks' gradients.  Rank 0 checks the sum against the per-image loop in fp64 with PyTorch's layers, the fp32 PyTorch loop being the
   yardstick: error <= 4 x its error + u sqrt(R) per parameter (relative to the largest fp64 entry; the two biases whose true gradient is
   0 against their layer's weight gradient).
2. Training: 4 iterations of train_id_module(batched_window=True, data_parallel=True, backward_ray_groups=0) on a 2 000-Gaussian scene,
   4 images per iteration, evaluation on rank 0 every 2 iterations.  Every rank hashes its state_dict; rank 0 then trains a fresh module
   from the same seed alone (batched_window=True, the single-rank defaults); both runs' logged scalars (loss, camera-up, score term per
   iteration) and the agreement of the checkpoint keys go into the report.

Prints one JSON line (rank 0)."""
import argparse
import functools
import hashlib
import importlib
import json
import math
import os
import sys
import tempfile
import types

os.environ.setdefault("SIXDGS_RANDOM_BACKBONE", "1")     # synthetic check: random-init ViT-S/14 (the image side is pinned anyway)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 2.0 ** -24
MARGIN = 2.0 ** -20
ZERO_GRADIENT = ("ray_preprocessor.mlp2.2.bias", "attention.k_proj.bias")

pkg = importlib.import_module("6dgs_amd")
syn = importlib.import_module("6dgs_amd.synthetic")
ops = importlib.import_module("6dgs_amd.ops")
train = importlib.import_module("6dgs_amd.train")
dd = importlib.import_module("6dgs_amd.distributed")


def _scorer():
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(0, with_cnn=True).items()}, strict=False)
    return idm.cuda().train()


def _ray_margin(idm64, ori, dr, rgb):
    """Per ray, the smallest |pre-activation| / (|a| |w|^T + |b|) over the ReLU layers of the ray MLP."""
    rp = idm64.ray_preprocessor
    with torch.no_grad():
        ori, dr, rgb = ori.double(), dr.double(), rgb.double()
        x = torch.cat((ori, dr, rgb, idm64._pe(ori, rp.pospe), idm64._pe(dr, rp.viewpe), idm64._pe(rgb, rp.rgbpe)), -1)
        margin = torch.full((x.shape[0],), math.inf, dtype=torch.float64, device=x.device)
        a = x
        for lin in (rp.mlp[0], rp.mlp[2], rp.mlp2[0]):
            if lin is rp.mlp2[0]:
                a = torch.cat((a, x), -1)
            z = torch.nn.functional.linear(a, lin.weight, lin.bias)
            margin = torch.minimum(margin, (z.abs() / (a.abs() @ lin.weight.abs().t() + lin.bias.abs())).min(dim=1).values)
            a = torch.relu(z)
    return margin


class _Window:
    """A pool of 6 training views with pinned image sides (tokens 256 / 137 / 256 / 200 / 1 / 256, fixed feature maps), 32 draws from it,
    and 3000 rays away from ReLU ties and from every view's camera plane.  Deterministic: every rank builds the same window."""

    def __init__(self):
        gen = torch.Generator().manual_seed(11)
        self.counts = (256, 137, 256, 200, 1, 256)
        self.toks = [torch.randn(n, 398, generator=gen).cuda() for n in self.counts]
        self.fmaps = torch.randn(len(self.counts), 384, 16, 16, generator=gen).cuda()
        self.cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(len(self.counts), 23, width=16, height=16)]
        test = importlib.import_module("6dgs_amd.test")
        self.poses = torch.stack([test.gt_pose_and_intrinsics(c, "cuda")[0] for c in self.cams]).cuda()
        self.draw = torch.randint(0, len(self.counts), (32,), generator=gen).tolist()
        idm64 = _scorer().double()
        rays = syn.make_rays(3600, 4)
        o, d, c = (torch.from_numpy(rays[k]).cuda() for k in ("ori", "dir", "rgb"))
        ok = _ray_margin(idm64, o, d, c) > MARGIN
        for p in self.poses.double():
            ctr, z = p[:3, 3], p[:3, 2]
            ok &= ((o.double() - ctr) * z).sum(-1).abs() / ((o.double() - ctr).abs() @ z.abs()) > MARGIN
        keep = torch.nonzero(ok).flatten()[:3000]
        assert keep.numel() == 3000
        self.rays = (o[keep].contiguous(), d[keep].contiguous(), c[keep].contiguous())
        self.model_up = torch.tensor([0.0, 1.0, 0.0], device="cuda")

    def pin(self, m, dt):
        m.backbone_wrapper.forward = lambda img, mask: (self.toks[int(img[0, 0, 0])].to(dt),
                                                        self.fmaps[int(img[0, 0, 0])].to(dt).permute(1, 2, 0).reshape(-1, 384),
                                                        self.fmaps[int(img[0, 0, 0])].to(dt))
        m.image_tokens = lambda imgs, masks: ([self.toks[int(i[0, 0, 0])].to(dt) for i in imgs],
                                              torch.stack([self.fmaps[int(i[0, 0, 0])] for i in imgs]).to(dt))

    def image(self, v, dt=torch.float32):
        return torch.full((4, 4, 3), float(v), device="cuda", dtype=dt)

    def targets(self):
        return [ops.distance_target(self.rays[0], self.rays[1], self.poses[v], self.counts[v]) for v in range(len(self.counts))]


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _optimiser_params(m):
    return list(m.ray_preprocessor.parameters()) + list(m.attention.parameters()) + list(m.camera_direction_prediction_network.parameters())


def _per_image_loop(w, m, dt, targets):
    m.zero_grad()
    w.pin(m, dt)
    o, d, c = (t.to(dt) for t in w.rays)
    for v in w.draw:
        s, _, _, up, used = m(w.image(v, dt), None, o, d, c)
        combined = torch.square(s - targets[v].to(dt)[used]).mean() + 0.1 * (-0.5 * torch.cosine_similarity(w.model_up.to(dt), up, dim=-1) + 0.5)
        (combined / 32).backward()
    return _grads(m)


def _check_against(ref, f32, got):
    """Largest error / bound over the parameters, and the parameters out of bound."""
    floor = U * math.sqrt(3000)
    worst, bad = 0.0, []
    for name in ref:
        scale = float(ref[name.replace(".bias", ".weight")].abs().max()) if name in ZERO_GRADIENT else float(ref[name].abs().max())
        e_h = float((got[name].double() - ref[name]).abs().max()) / scale
        e_32 = float((f32[name].double() - ref[name]).abs().max()) / scale
        ratio = e_h / (4 * e_32 + floor)
        worst = max(worst, ratio)
        if ratio > 1.0:
            bad.append(name)
    return worst, bad


def check_gradients(rank, world):
    w = _Window()
    lo, hi = dd.shard_range(32, rank, world)
    draws = w.draw[lo:hi]
    m = _scorer()
    m.zero_grad()
    w.pin(m, torch.float32)
    loss, logs, finite = train.window_step_loss(m, [w.image(v) for v in draws], [None] * len(draws),
                                                w.poses[torch.tensor(draws, device="cuda")], *w.rays, w.model_up, 32, ray_groups=0)
    loss.backward()
    logs = dd.sum_gradients(_optimiser_params(m), logs)
    got = _grads(m)
    out = {"draws": [lo, hi], "finite": bool(finite.all()) and bool(torch.isfinite(logs).all())}
    dd.barrier()
    if rank == 0:
        targets = w.targets()
        m64 = _scorer().double()
        m64.hip_autograd = False
        ref = _per_image_loop(w, m64, torch.float64, targets)
        m32 = _scorer()
        m32.hip_autograd = False
        f32 = _per_image_loop(w, m32, torch.float32, targets)
        worst, bad = _check_against(ref, f32, got)
        out.update(params=len(got), same_names=set(got) == set(ref) == set(f32), worst_ratio=worst, out_of_bound=bad)
    dd.barrier()
    return out


def _state_hash(m):
    h = hashlib.sha256()
    for k, v in m.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _train(scene, info, ckpt, data_parallel):
    torch.manual_seed(0)
    idm = _scorer()
    logged = []
    kw = dict(data_parallel=True, backward_ray_groups=0) if data_parallel else {}
    train.train_id_module(ckpt, "cuda", idm, functools.partial(pkg.generate_all_possible_rays, scene), info, "seq", "cat",
                          n_iterations=4, gradient_accumulation_steps=4, display_every_n_iterations=2, val_every_n_iterations=2,
                          log_fn=lambda tag, v, it: logged.append((tag, v, it)), batched_window=True, **kw)
    return idm, logged


def check_training(rank, world, tmp):
    scene = pkg.GaussianScene.from_dict(syn.make_scene(2000, 3), device="cuda")
    cams = [pkg.CameraInfo(**c) for c in syn.make_cameras(3, 17, width=64, height=64)]
    info = types.SimpleNamespace(train_cameras=cams, test_cameras=cams[:1])
    ckpt_dp = os.path.join(tmp, "id_module_dp.th")
    idm, logged = _train(scene, info, ckpt_dp, True)
    hashes = [None] * world
    dist.all_gather_object(hashes, _state_hash(idm))
    losses = [[v for tag, v, _ in logged if tag == t] for t in ("train/loss", "train/cam_up", "train/loss_score")]
    all_losses = [None] * world
    dist.all_gather_object(all_losses, losses)
    out = {"state_dicts_identical": len(set(hashes)) == 1, "logs_identical_on_ranks": all(x == all_losses[0] for x in all_losses)}
    if rank == 0:
        ckpt_1 = os.path.join(tmp, "id_module_single.th")
        _, logged1 = _train(scene, info, ckpt_1, False)
        single = [[v for tag, v, _ in logged1 if tag == t] for t in ("train/loss", "train/cam_up", "train/loss_score")]
        sd_dp, sd_1 = torch.load(ckpt_dp), torch.load(ckpt_1)
        out.update(logs_dp=losses, logs_single=single, iterations=len(losses[0]),
                   finite=all(math.isfinite(v) for la in losses for v in la),
                   evaluated=any(tag == "val/avg_translation_error" for tag, _, _ in logged),
                   checkpoint_keys_match=(set(sd_dp) == set(sd_1) and set(sd_dp["model_state_dict"]) == set(sd_1["model_state_dict"])
                                          and set(sd_dp["optimizer_state_dict"]["state"]) == set(sd_1["optimizer_state_dict"]["state"])
                                          and sd_dp["epoch"] == sd_1["epoch"] == 4))
    dd.barrier()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default=None)
    ap.add_argument("--device", type=int, default=None, help="force this device on every rank (single-GPU test boxes)")
    a = ap.parse_args()
    rank, world, local = dd.init_from_env(a.backend, set_device=a.device is None)
    dev = torch.device("cuda", a.device if a.device is not None else local)
    torch.cuda.set_device(dev)
    dd.warm_long_wait_group(dev)
    res = {"world": world, "backend": dd.backend_name()}
    res["gradients"] = check_gradients(rank, world)
    with tempfile.TemporaryDirectory() as tmp:
        if dd.is_dist():            # one directory for every rank: rank 0's
            box = [tmp]
            dist.broadcast_object_list(box, 0)
            tmp_shared = box[0]
        else:
            tmp_shared = tmp
        res["training"] = check_training(rank, world, tmp_shared)
    if rank == 0:
        print(json.dumps(res))
    dd.barrier()


if __name__ == "__main__":
    main()
