"""The batched training window without a GPU: the scorer-backward ABI entries (header, binding, library), forward_window against the
per-image training forward in fp64 on the CPU, and the refusal of a window through an unlocked backbone."""
import ctypes
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_GRADIENT = ("ray_preprocessor.mlp2.2.bias", "attention.k_proj.bias")
NEW_SYMBOLS = ("sixdgs_score_backward", "sixdgs_score_backward_workspace_bytes")


def test_score_backward_symbols_are_declared_bound_and_exported():
    lib = importlib.import_module("6dgs_amd._lib")
    with open(os.path.join(ROOT, "include", "sixdgs.h")) as f:
        header = f.read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/sixdgs.h"
        assert name in lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(so, name), f"{name} is not exported by {lib.LIB_PATH}"
    assert lib.ABI_VERSION >= 8


def _module64(seed=0):
    pkg = importlib.import_module("6dgs_amd")
    syn = importlib.import_module("6dgs_amd.synthetic")
    idm = pkg.IdentificationModule("dino")
    idm.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_scorer_state_dict(seed, with_cnn=True).items()}, strict=False)
    idm = idm.double().train()
    idm.hip_autograd = False
    return idm


def test_forward_window_matches_the_per_image_forward_fp64():
    """Three images (256, 137 and 1 tokens) against 300 rays: sum_b (mean((scores_b - target_b)^2) + 0.1 camera-up loss_b) and its
    gradients with respect to every trainable parameter, once through forward_window and once as the sum of per-image forward calls
    (each with its own ray permutation), agree to 1e-10 relative in fp64.  The image side is pinned: the backbone returns fixed tokens
    and feature maps, to both paths."""
    syn = importlib.import_module("6dgs_amd.synthetic")
    idm = _module64()
    gen = torch.Generator().manual_seed(3)
    counts = (256, 137, 1)
    toks = [torch.randn(n, 398, generator=gen, dtype=torch.float64) for n in counts]
    fmaps = torch.randn(len(counts), 384, 16, 16, generator=gen, dtype=torch.float64)
    rays = syn.make_rays(300, 5)
    o, d, c = (torch.from_numpy(rays[k]).double() for k in ("ori", "dir", "rgb"))
    targets = [torch.rand(300, generator=gen, dtype=torch.float64) * n / 150 for n in counts]
    model_up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    params = [p for n, p in idm.named_parameters() if not n.startswith("backbone_wrapper")]

    def cam_loss(up):
        return -0.5 * torch.cosine_similarity(model_up, up, dim=-1) + 0.5

    # window
    idm.zero_grad()
    idm.image_tokens = lambda imgs, masks: (toks, fmaps)
    scores, up, n_host = idm.forward_window([None] * 3, [None] * 3, o, d, c)
    assert n_host == list(counts) and tuple(scores.shape) == (3, 300) and tuple(up.shape) == (3, 3)
    loss_w = sum(torch.square(scores[i] - targets[i]).mean() + 0.1 * cam_loss(up[i]) for i in range(3))
    loss_w.backward()
    grads_w = [p.grad.clone() for p in params]
    # per image
    idm.zero_grad()
    del idm.image_tokens
    loss_p = 0.0
    for i in range(3):
        fm = fmaps[i]
        idm.backbone_wrapper.forward = lambda img, mask, t=toks[i], fm=fm: (t, fm.permute(1, 2, 0).reshape(-1, 384), fm)
        s, att, _, u, used = idm(torch.zeros(8, 8, 3, dtype=torch.float64), None, o, d, c)
        li = torch.square(s - targets[i][used]).mean() + 0.1 * cam_loss(u)
        li.backward()
        loss_p = loss_p + float(li.detach())
    assert abs(float(loss_w.detach()) - loss_p) <= 1e-10 * abs(loss_p)
    ref = {n: p.grad for n, p in idm.named_parameters() if not n.startswith("backbone_wrapper")}
    for (name, r), gw in zip(ref.items(), grads_w):
        assert r is not None and gw is not None, name
        # the biases of mlp2.2 and k_proj shift every logit of a token alike: their true gradient is 0 and both paths return rounding
        # noise, measured against the gradient of the layer's weight instead
        scale = float(ref[name.replace(".bias", ".weight")].abs().max()) if name in ZERO_GRADIENT else float(r.abs().max())
        assert float((gw - r).abs().max()) <= 1e-10 * scale, name


def test_batched_window_needs_a_locked_backbone():
    train = importlib.import_module("6dgs_amd.train")
    with pytest.raises(ValueError):
        train.train_id_module("unused.th", "cpu", None, None, None, 0, "cat", lock_backbone=False, batched_window=True)
