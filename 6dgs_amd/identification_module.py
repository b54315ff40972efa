"""IdentificationModule -- drop-in for pose_estimation/identification_module.py:10-133.

Same constructor, same parameter names (the reference's id_module.th["model_state_dict"] loads with
load_state_dict), same test_image() return tuple.  The ray side (RayPreprocessor MLP + k_proj) and
the attention scorer + top-k run in the HIP library; the DINOv2 backbone and the camera-up CNN stay
on PyTorch-ROCm.  `forward` is the differentiable training path (PyTorch autograd, reference-sized ray sets).

Differences that make the path fast while keeping results:
  * the ray features/keys depend only on (rays, weights): they are computed ONCE per scene and cached
    (the reference recomputes the 1.7 MFLOP/ray MLP for every image, identification_module.py:79);
  * the [T, R] attention map is never handed out as a dense tensor: test_image returns a shape-only
    proxy (test.py:117 only reads .shape[-2]); `attention_map.materialize()` builds it on request;
  * test_images() scores a whole batch of query images against one pass over the key cache.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import ops
from .backbone import BackboneWrapper, BatchedTokens
from .camera_direction_network import CameraDirectionPredictor


def _lib_ray_keys_ws(r: int, max_chunk: int = ops.RAY_KEYS_CHUNK) -> int:
    from . import _lib
    return int(_lib.load().sixdgs_ray_keys_workspace_bytes(int(r), int(max_chunk)))


class RayPreprocessor(torch.nn.Module):
    """Parameter holder with the reference layout (ray_preprocessor.py:11-34)."""

    def __init__(self, viewpe=8, pospe=8, rgbpe=6, featureC=128, fea_output=128):
        super().__init__()
        self.in_mlpC = 2 * viewpe * 3 + 3 + 2 * pospe * 3 + 3 + 2 * rgbpe * 3 + 3
        self.mlp = torch.nn.Sequential(torch.nn.Linear(self.in_mlpC, featureC), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(featureC, featureC), torch.nn.ReLU(inplace=True))
        self.mlp2 = torch.nn.Sequential(torch.nn.Linear(featureC + self.in_mlpC, featureC), torch.nn.ReLU(inplace=True),
                                        torch.nn.Linear(featureC, fea_output))
        self.viewpe, self.pospe, self.rgbpe = viewpe, pospe, rgbpe


class MultiHeadAttention(torch.nn.Module):
    """Parameter holder (our_multihead_attention.py:46-68): q_proj 398->384, k_proj 384->384."""

    def __init__(self, ray_fea_size, img_fea_size, embed_dim, num_heads=1):
        super().__init__()
        assert embed_dim % num_heads == 0
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.q_proj = torch.nn.Linear(img_fea_size, embed_dim)
        self.k_proj = torch.nn.Linear(ray_fea_size, embed_dim)
        torch.nn.init.xavier_uniform_(self.q_proj.weight)
        self.q_proj.bias.data.fill_(0)
        torch.nn.init.xavier_uniform_(self.k_proj.weight)
        self.k_proj.bias.data.fill_(0)


class AttentionMapProxy:
    """Stands in for the dense softmax(QK^T) [T, R] map (32 GB at R = 32 M)."""

    def __init__(self, n_tokens: int, n_rays: int, builder=None):
        self.shape = torch.Size((n_tokens, n_rays))
        self._builder = builder

    def materialize(self) -> torch.Tensor:
        if self._builder is None:
            raise RuntimeError("attention map not retained")
        return self._builder()


class IdentificationModule(torch.nn.Module):
    def __init__(self, backbone_type: str = "dino", camera_up_output_augmentation=None,
                 target_rays_dirs: Optional[torch.Tensor] = None, augmentation_channels: int = 10,
                 backbone: Optional[torch.nn.Module] = None):
        super().__init__()
        if camera_up_output_augmentation not in (None, 0, "NONE") and getattr(camera_up_output_augmentation, "name", "NONE") != "NONE":
            raise NotImplementedError("camera-up output augmentations are not on the accelerated path "
                                      "(reference default is NONE, identification_module.py:11,35-36)")
        self.backbone_wrapper = BackboneWrapper(backbone_type=backbone_type, backbone=backbone)
        nf = self.backbone_wrapper.img_num_features
        self.ray_preprocessor = RayPreprocessor(featureC=512, fea_output=nf)
        self.camera_up_out_augmentation = None
        self.camera_direction_prediction_network = CameraDirectionPredictor(nf, self.backbone_wrapper.backbone_wh, fea_output=3)
        self.attention = MultiHeadAttention(nf, nf + 14, nf, 1)
        self.hip_autograd = True        # training forward/backward of the dense layers on the HIP GEMM when the tensors live on the GPU
        self._packed = None
        self._packed_key = None
        self._key_cache = None
        self._key_cache_id = None
        self._key_cache_rays = None

    # ---- caches -------------------------------------------------------------------------------------
    def _scorer_params(self):
        rp, at = self.ray_preprocessor, self.attention
        return {
            "ray_preprocessor.mlp.0.weight": rp.mlp[0].weight, "ray_preprocessor.mlp.0.bias": rp.mlp[0].bias,
            "ray_preprocessor.mlp.2.weight": rp.mlp[2].weight, "ray_preprocessor.mlp.2.bias": rp.mlp[2].bias,
            "ray_preprocessor.mlp2.0.weight": rp.mlp2[0].weight, "ray_preprocessor.mlp2.0.bias": rp.mlp2[0].bias,
            "ray_preprocessor.mlp2.2.weight": rp.mlp2[2].weight, "ray_preprocessor.mlp2.2.bias": rp.mlp2[2].bias,
            "attention.k_proj.weight": at.k_proj.weight, "attention.k_proj.bias": at.k_proj.bias,
            "attention.q_proj.weight": at.q_proj.weight, "attention.q_proj.bias": at.q_proj.bias,
        }

    def packed_weights(self, device) -> ops.PackedWeights:
        params = self._scorer_params()
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params.values())
        if self._packed is None or self._packed_key != key:
            self._packed = ops.PackedWeights(params, device)
            self._packed_key = key
            self._key_cache = None
        return self._packed

    KEEP_FP32_KEYS_BELOW = 4_000_000   # rays; above, only the scaled fp16 planes are cached (1536 B/ray instead of 1536 + 1536)

    def _ensure_keys(self, rays_ori, rays_dir, rays_rgb, profile=None, sample_min_rays: Optional[int] = None):
        w = self.packed_weights(rays_ori.device)
        # Identity of the cache entry: the three ray tensor OBJECTS (held strongly, so the allocator cannot hand their
        # addresses to a new ray set while the entry lives), their in-place versions, the weights and the MMA mode.
        mode = ops.effective_mma_mode()
        # F16X3 / F16X3_L32 share planes; MMA_F32 / MMA_BF16X6 score on fp32 keys (k_logits<MMA>), computed by the dense layers of that mode
        fmt = "f16-planes" if mode in ops.F16_MODES else f"f32-keys-mma{mode}"
        smin = ops.SELECT_MIN_RAYS if sample_min_rays is None else int(sample_min_rays)     # scenes from this size get the select path's ray sample
        ident = (rays_ori.shape[0], rays_ori._version, rays_dir._version, rays_rgb._version, self._packed_key, fmt, rays_ori.shape[0] >= smin)
        held = self._key_cache_rays
        same = (self._key_cache is not None and self._key_cache_id == ident and held is not None
                and all(h is t or (h.data_ptr() == t.data_ptr() and h.shape == t.shape and h.stride() == t.stride())   # a view of
                        for h, t in zip(held, (rays_ori, rays_dir, rays_rgb))))       # the held (hence still allocated) memory
        if not same:
            self._key_cache = self._key_cache_rays = None        # drop the old planes before allocating the new ones
            if ops.get_arena() is not None:                      # ... and with an arena everything else that was carved from it for the old scene
                self._select_ws = self._stream_sample = None
                ops.get_arena().reset(self)
            r = rays_ori.shape[0]
            planes_mode = mode in ops.F16_MODES
            keep_fp32 = (not planes_mode) or r <= self.KEEP_FP32_KEYS_BELOW
            scale = None
            norm = torch.zeros(1, device=rays_ori.device) if planes_mode else None
            if planes_mode:
                # (norm: max |k_r| of the scene -- the select path's slack is derived from it, sixdgs.h: sixdgs_score_select)
                _, key, (planes, scale) = ops.ray_keys(rays_ori, rays_dir, rays_rgb, w, want_key=keep_fp32, profile=profile, want_planes=True, norm_out=norm)
            else:
                _, key = ops.ray_keys(rays_ori, rays_dir, rays_rgb, w, profile=profile)
                planes = None
            sample = None
            if planes_mode and r >= smin:
                # the ray sample of the select path (ops.score_select): one ray in 16 through the same ray MLP (+6 % set-up work,
                # +96 B per ray); its planes carry their own tile scales
                si = ops.select_sample_indices(r, rays_ori.device)
                _, _, (s_planes, s_scale) = ops.ray_keys(rays_ori[si], rays_dir[si], rays_rgb[si], w, want_key=False, want_planes=True)
                sample = (s_planes, s_scale)
            self._key_cache, self._key_cache_id = {"key": key, "planes": planes, "scale": scale, "sample": sample, "norm": norm}, ident
            self._key_cache_rays = (rays_ori, rays_dir, rays_rgb)
        return self._key_cache

    def ray_keys(self, rays_ori, rays_dir, rays_rgb, profile=None) -> torch.Tensor:
        """K[R,384] = k_proj(RayPreprocessor(rays)) -- computed once per (ray tensors, weights) and cached, as fp32
        and/or as the scaled fp16 planes the fast scorer kernels stream."""
        c = self._ensure_keys(rays_ori, rays_dir, rays_rgb, profile)
        if c["key"] is None:   # large scene: fp32 copy on request only
            _, key = ops.ray_keys(rays_ori, rays_dir, rays_rgb, self.packed_weights(rays_ori.device))
            return key
        return c["key"]

    def ray_features(self, rays_ori, rays_dir, rays_rgb) -> torch.Tensor:
        """RayPreprocessor.forward (ray_preprocessor.py:36-46): [R,384] features (not cached)."""
        feat, _ = ops.ray_keys(rays_ori, rays_dir, rays_rgb, self.packed_weights(rays_ori.device), want_feat=True, want_key=False)
        return feat

    def _full_ntok(self, b, device):
        c = getattr(self, "_ntok_cache", None)
        if c is None or c.shape[0] < b or c.device != device:
            self._ntok_cache = c = torch.full((max(b, 64),), ops.MAX_TOKENS, dtype=torch.int32, device=device)
        return c[:b]

    def _tokens_to_q(self, token_list, device):
        """The Q side of the boundary: (q [B,256,384], n_tok device int32 [B], n_tok host list, tokens as handed in).
        list of [T_i,398] -> zero-padded block + sixdgs_q_proj; BatchedTokens (every image keeps all 256 tokens) -> the fused form:
        q = feats . Wq[:, :384]^T + (pe . Wq[:, 384:]^T + bq), the bracket being one [256,384] table per set of weights -- no
        [B,256,398] concatenation, no padding copy (PE concat + q_proj fused)."""
        w = self.packed_weights(device)
        if isinstance(token_list, BatchedTokens):
            b, t = token_list.shape[0], token_list.shape[1]
            if t != ops.MAX_TOKENS:
                token_list = token_list.dense()
            else:
                wq, bq = self.attention.q_proj.weight, self.attention.q_proj.bias
                # the cache entry HOLDS the position table it was built from (identity + in-place version, like _ensure_keys holds the
                # rays): an address alone could be handed to another table by the allocator while the entry lives
                pe = token_list.pe
                c = getattr(self, "_peq", None)
                if c is None or c[0] != self._packed_key or c[1] is not pe or c[2] != pe._version:
                    self._peq = c = (self._packed_key, pe, pe._version, torch.addmm(bq.detach(), pe, wq.detach()[:, ops.D:].t()).contiguous(),
                                     wq.detach()[:, :ops.D].contiguous())
                q = ops.linear(token_list.feats.reshape(b * t, ops.D), c[4]).view(b, t, ops.D)
                q += c[3]
                return q, self._full_ntok(b, device), [t] * b
        if torch.is_tensor(token_list):          # pre-batched dense [B,256,398]: every image has all 256 tokens
            tokens = token_list.contiguous()
            n_host = [tokens.shape[1]] * tokens.shape[0]
            n_tok = self._full_ntok(tokens.shape[0], tokens.device)
        else:
            tokens, n_tok = ops.pad_tokens(token_list, device)
            n_host = [int(t.shape[0]) for t in token_list]
        return ops.q_proj(tokens, n_tok, w), n_tok, n_host

    def invalidate_caches(self):
        """Drops the packed weights and the key cache (needed only after mutating weights or rays through `.data` tricks
        that bypass the version counters; a NEW ray tensor always misses the cache: entries are keyed on tensor identity)."""
        self._packed = self._key_cache = self._key_cache_rays = self._select_ws = self._stream_sample = self._peq = None
        if ops.get_arena() is not None:       # the planes / workspaces just dropped were carved from it (an arena serves ONE module: ops.Arena)
            ops.get_arena().reset(self)

    # ---- image side (PyTorch-ROCm) --------------------------------------------------------------------
    @torch.no_grad()
    def image_tokens_u8(self, imgs_u8: torch.Tensor, table256: torch.Tensor):
        """A batch of RGB query images of one size as they arrive -- uint8 [B,H,W,3] on the GPU -- -> what image_tokens returns for them, with the whole
        transform pipeline in one kernel (BackboneWrapper.preprocess_batch_u8); None when that kernel does not apply."""
        bw = self.backbone_wrapper
        norm = bw.preprocess_batch_u8(imgs_u8, table256)
        if norm is None:
            return None
        return bw.assemble_batch(bw.features_from_norm(norm))

    @torch.no_grad()
    def image_tokens(self, imgs: Sequence[torch.Tensor], masks: Sequence[Optional[torch.Tensor]]):
        """Batch of images (any sizes; mask None = no alpha channel) -> (tokens, fmaps [B,384,16,16]) where tokens is a
        list of [T_i,398] tensors, or ONE [B,256,398] tensor when every image keeps all 256 tokens and all share a size
        (the common case: one launch sequence for the whole batch instead of one per image)."""
        bw = self.backbone_wrapper
        if all(m is None for m in masks) and all(i.shape == imgs[0].shape for i in imgs):
            stacked = imgs if isinstance(imgs, torch.Tensor) and imgs.dim() == 4 else torch.stack(list(imgs))      # (prepare_images_device hands over one tensor)
            feats = bw.features_from_norm(bw.preprocess_batch(stacked))
            return bw.assemble_batch(feats)
        pre = [bw.preprocess(i, m) for i, m in zip(imgs, masks)]
        feats = bw.features_from_norm(torch.cat([p[0] for p in pre], dim=0))
        toks, fmaps = [], []
        for f, (_, mimg) in zip(feats, pre):
            t_pe, _, fmap = bw.assemble(f, mimg)
            toks.append(t_pe)
            fmaps.append(fmap)
        return toks, torch.stack(fmaps)

    @torch.no_grad()
    def camera_up(self, fmaps: torch.Tensor) -> torch.Tensor:
        up = self.camera_direction_prediction_network(fmaps)
        return torch.nn.functional.normalize(up, dim=-1)

    # ---- scoring -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def score_tokens(self, token_list: List[torch.Tensor], rays_ori, rays_dir, rays_rgb, rays_to_output: int = 100,
                     want_scores: bool = True, workspace: Optional[torch.Tensor] = None, images_in_flight: Optional[int] = None,
                     profile=None, defer_status: bool = False):
        """tokens (the boundary's Q-side input) -> idx [B,k], values [B,k], scores [B,R] or None.

        defer_status (select path only): do NOT read the per-image status on the host here -- the call then enqueues work and
        nothing else (capturable in a hipGraph, no sync in the middle of a step) and leaves `self.pending_select`; the caller
        reads the status together with its own results (one D2H per batch) and calls `finish_select` if any image was refused."""
        rays_to_output = ops.check_topk(rays_to_output)
        kc = self._ensure_keys(rays_ori, rays_dir, rays_rgb)
        w = self.packed_weights(rays_ori.device)
        q, n_tok, n_host = self._tokens_to_q(token_list, rays_ori.device)
        self.last_scoring_path = "two-pass"
        self.pending_select = None
        capturing = torch.cuda.is_current_stream_capturing()
        if (not want_scores and kc.get("sample") is not None and ops.select_enabled() and ops.effective_mma_mode() in ops.F16_MODES
                and rays_to_output <= ops.SELECT_MAX_CANDIDATES and (defer_status or not capturing)):     # (the candidate list must hold k)
            # inference: only the top-k is wanted -> no logits through HBM (sixdgs_score_select); images the bounds cannot decide
            # (status -1: too many near-ties for max_candidates, or an exponent overflow) go through the two-pass scorer below
            b, r = q.shape[0], rays_ori.shape[0]
            need = ops.score_select_workspace_bytes(r, b, rays_to_output, ops.SELECT_MAX_CANDIDATES)
            sw = getattr(self, "_select_ws", None)
            if sw is None or sw.numel() < need or sw.device != q.device:
                if capturing:
                    raise RuntimeError("6dgs_amd: the select workspace must exist before a hipGraph capture (run the batch once eagerly)")
                self._select_ws = sw = None
                self._select_ws = sw = ops.big_empty(need, torch.uint8, q.device)
            # Token packing (round 5): the library packs the images of a launch into the sweep's 256-token tiles by their token counts (two views of
            # <= 128 tokens or four of <= 64 share a tile; csrc/sweep_plan.h) -- masked views (Tanks&Temples / Blender keep 56-176 of 256 tokens) cost what
            # their tokens cost, in ONE call with nothing permuted on the host.  (Round 4 ran one full select pipeline per 64-token row-count class here.)
            idx, val, status = ops.score_select(q, n_tok, kc["planes"], kc["scale"], kc["sample"][0], kc["sample"][1], rays_to_output,
                                                max_candidates=ops.SELECT_MAX_CANDIDATES, workspace=sw, profile=profile, n_tok_host=n_host,
                                                key_norm=kc["norm"])
            self.last_select_launches = ops.select_sweep_plan(n_host)          # [(tiles, images)] per sweep launch
            self.last_scoring_path = "select"
            pend = dict(status=status, q=q, n_tok=n_tok, k=rays_to_output, workspace=workspace, images_in_flight=images_in_flight,
                        rays=(rays_ori, rays_dir, rays_rgb))
            if defer_status:
                self.pending_select = pend
                return idx, val, None
            idx, val, _ = self.finish_select(idx, val, pend)
            return idx, val, None
        idx, val, scores, _ = ops.score_topk(q, n_tok, kc["key"], rays_to_output, want_scores=want_scores, workspace=workspace,
                                             images_in_flight=images_in_flight, profile=profile, n_tok_host=n_host,
                                             key_planes=kc["planes"], key_scale=kc["scale"])
        return idx, val, scores

    @torch.no_grad()
    def finish_select(self, idx, val, pending=None, status_host=None):
        """Second half of a select-path call: read the statuses (unless the caller already has them on the host) and score the refused
        images with the two-pass scorer.  Returns (idx, val, refused image numbers); idx / val are updated in place."""
        pend = pending if pending is not None else self.pending_select
        self.pending_select = None
        if pend is None:
            return idx, val, []
        st = pend["status"].tolist() if status_host is None else [int(v) for v in status_host]      # the one host sync of the path (B ints)
        self.last_select_candidates = st
        redo = [i for i, v in enumerate(st) if v < 0]
        self.last_scoring_path = "select" if not redo else f"select+two-pass({len(redo)})"
        if redo:
            kc = self._ensure_keys(*pend["rays"])
            q, n_tok = pend["q"], pend["n_tok"]
            sel = torch.tensor(redo, device=q.device)
            i2, v2, _, _ = ops.score_topk(q[sel].contiguous(), n_tok[sel].contiguous(), kc["key"], pend["k"], want_scores=False,
                                          workspace=pend["workspace"], images_in_flight=pend["images_in_flight"], key_planes=kc["planes"],
                                          key_scale=kc["scale"])
            idx[sel], val[sel] = i2, v2
        return idx, val, redo

    @torch.no_grad()
    def score_tokens_ray_sharded(self, token_list, rays_ori, rays_dir, rays_rgb, ray_offset: int, r_total: int, rays_to_output: int = 100,
                                 group=None, profile=None, use_select: bool = True):
        """The scorer over a scene whose RAYS are split across the ranks (SURVEY 8(e) fallback: key planes that fit only across
        several GPUs -- cfg-4's 786 GB at N >= 4 -- or one image scored by several GPUs).  This rank holds rays
        [ray_offset, ray_offset + len(rays_ori)) of r_total and keeps THEIR key planes resident (no per-step ray MLP, which is half
        of a streamed step); every rank passes the SAME tokens.  Select path (distributed.score_select_ray_sharded) when only the
        top-k is wanted and every rank has a ray sample; images it cannot decide, and use_select=False, take the two-pass cut
        (distributed.score_topk_ray_sharded).  Returns (global idx [B,k], val [B,k]) identical on every rank."""
        from . import distributed as dd
        dev, k = rays_ori.device, ops.check_topk(rays_to_output)
        world = dd.world()
        kc = self._ensure_keys(rays_ori, rays_dir, rays_rgb, sample_min_rays=max(4096, ops.SELECT_MIN_RAYS // max(world, 1)))
        q, n_tok, n_host = self._tokens_to_q(token_list, dev)
        f16 = ops.effective_mma_mode() in ops.F16_MODES
        have = torch.tensor([1 if (kc.get("sample") is not None and f16 and use_select and ops.select_enabled()
                                  and k <= ops.SELECT_MAX_CANDIDATES) else 0,        # (the candidate list must hold k)
                             0 if kc.get("sample") is None else int(kc["sample"][0].shape[0])], dtype=torch.int64, device=dev)
        if dd.is_dist():
            flag, cnt = have[:1].clone(), have[1:].clone()
            dd._all_reduce(flag, torch.distributed.ReduceOp.MIN, group)
            dd._all_reduce(cnt, torch.distributed.ReduceOp.SUM, group)
            have = torch.cat([flag, cnt])
        use, r_sample_total = bool(int(have[0])), int(have[1])
        b = q.shape[0]
        idx = torch.full((b, k), -1, dtype=torch.int64, device=dev)
        val = torch.full((b, k), float("nan"), device=dev)
        redo = list(range(b))
        self.last_scoring_path = f"ray-sharded x{world} two-pass"
        if use:
            idx, val, st = dd.score_select_ray_sharded(q, n_tok, kc["planes"], kc["scale"], kc["sample"][0], kc["sample"][1], ray_offset, r_total,
                                                       r_sample_total, k, n_tok_host=n_host, profile=profile, group=group, key_norm=kc["norm"])
            self.last_select_candidates = st
            redo = [i for i, v in enumerate(st) if v < 0]
            self.last_scoring_path = f"ray-sharded x{world} select" + (f"+two-pass({len(redo)})" if redo else "")
        if redo:
            sel = torch.tensor(redo, device=dev)
            i2, v2, _ = dd.score_topk_ray_sharded(q[sel].contiguous(), n_tok[sel].contiguous(), kc["key"], ray_offset, k, key_planes=kc["planes"],
                                                  key_scale=kc["scale"], group=group)
            idx[sel], val[sel] = i2, v2
        return idx, val

    @torch.no_grad()
    def score_tokens_streamed(self, token_list, rays_ori, rays_dir, rays_rgb, rays_to_output: int = 100, chunk_rays: int = 8_388_608,
                              profile=None, key_cache_bytes: Optional[int] = None, return_stats: bool = False, use_select: bool = True):
        """The scorer without a resident key cache, for ray sets whose keys (1536 B/ray) plus logits (784 B/ray/image) exceed
        the GPU: the rays go through in chunks, ALL images of the batch share each chunk's keys, and the keys are computed,
        used and dropped -- twice, because the softmax runs over ALL rays: sweep 1 collects each chunk's row statistics and
        merges them (M = max m_c, S = sum s_c e^(m_c - M)), sweep 2 finishes every chunk with the global statistics and merges
        its top-k candidates (value descending, global index ascending).  The key planes of as many chunks as fit in
        `key_cache_bytes` (default: 70 % of the HBM that is free once the logits workspace exists) survive from sweep 1 to
        sweep 2, so only the remaining chunks pay the ray MLP twice.  Same result as score_tokens up to the rounding of the sum
        of exponentials.  Returns (idx [B,k], val [B,k]); no [B,R] score vector.  return_stats: also (global row statistics
        [B,256,2], softmax mass per image = sum of all scores, which must equal the image's token count)."""
        rays_to_output = ops.check_topk(rays_to_output)
        dev = rays_ori.device
        w = self.packed_weights(dev)
        q, n_tok, n_host = self._tokens_to_q(token_list, dev)
        b, r, k = q.shape[0], rays_ori.shape[0], rays_to_output
        chunk = max(256, (min(chunk_rays, max(r, 1)) + 255) // 256 * 256)       # whole 256-ray tiles (and fp16 scale tiles)
        mode = ops.effective_mma_mode()
        f16 = planes_mode = mode in ops.F16_MODES
        self.last_scoring_path = "streamed two-pass"
        if (f16 and use_select and not return_stats and ops.select_enabled() and r >= ops.SELECT_MIN_RAYS and k <= ops.SELECT_MAX_CANDIDATES
                and not torch.cuda.is_current_stream_capturing()):      # (k <= SELECT_MAX_CANDIDATES: the candidate list must hold k)
            # Select path, streamed: ONE sweep of ray MLP + matrix-core pass over the chunks (plus 1/16 for the sample) instead
            # of two -- U (4 B per ray and image) is all that is kept of a chunk; the candidates' keys are recomputed at the end.
            cmax = ops.SELECT_MAX_CANDIDATES
            held = getattr(self, "_stream_sample", None)
            ident = (r, rays_ori._version, rays_dir._version, rays_rgb._version, self._packed_key)
            if not (held is not None and held[0] == ident and all(h.data_ptr() == t.data_ptr() for h, t in zip(held[1], (rays_ori, rays_dir, rays_rgb)))):
                self._stream_sample = held = None
                if ops.get_arena() is not None:                  # a new scene: what the arena held for the previous one goes
                    self._key_cache = self._key_cache_rays = self._select_ws = None
                    ops.get_arena().reset(self)
                si = ops.select_sample_indices(r, dev)
                _, _, (sp, sscale) = ops.ray_keys(rays_ori[si], rays_dir[si], rays_rgb[si], w, want_key=False, want_planes=True)
                self._stream_sample = held = (ident, (rays_ori, rays_dir, rays_rgb), sp, sscale)      # once per scene, like the key cache
            with ops.arena_scope():          # U, the stage workspaces and the chunks' planes: given back to the arena (if any) when the batch is enqueued
                ss = ops.SelectStream(q, n_tok, r, k, cmax, n_host)
                ss.reserve(max(min(chunk, r), int(held[2].shape[0])))
                ss.begin(held[2], held[3])
                for r0 in range(0, r, chunk):
                    r1 = min(r0 + chunk, r)
                    with ops.arena_scope():  # one chunk's key planes
                        _, _, (planes, scale) = ops.ray_keys(rays_ori[r0:r1], rays_dir[r0:r1], rays_rgb[r0:r1], w, want_key=False, want_planes=True,
                                                             norm_out=ss.key_norm)
                        ss.sweep(planes, scale, r0, profile, update_norm=False)
                        del planes, scale
                cand, count = ss.candidates()
                inside = torch.arange(cmax, device=dev)[None, :] < count.clamp(min=0, max=cmax)[:, None]
                ci = torch.where(inside, cand, torch.zeros_like(cand)).reshape(-1)
                _, _, (cp, cs) = ops.ray_keys(rays_ori[ci], rays_dir[ci], rays_rgb[ci], w, want_key=False, want_planes=True)
                idx, val, status = ss.rescore(cp, cs, cand, count, compact=True)
            st = status.tolist()                         # the one host sync of the path
            self.last_select_candidates = st
            redo = [i for i, v in enumerate(st) if v < 0]
            self.last_scoring_path = "streamed select" if not redo else f"streamed select+two-pass({len(redo)})"
            if redo:
                del ss
                sub = token_list[torch.tensor(redo, device=dev)] if (torch.is_tensor(token_list) or isinstance(token_list, BatchedTokens)) else [token_list[i] for i in redo]
                i2, v2 = self.score_tokens_streamed(sub, rays_ori, rays_dir, rays_rgb, k, chunk_rays, profile, key_cache_bytes, use_select=False)
                sel = torch.tensor(redo, device=dev)
                idx[sel], val[sel] = i2, v2
                self.last_scoring_path = f"streamed select+two-pass({len(redo)})"       # (the inner call left "streamed two-pass")
            return idx, val
        # Streamed two-pass.  With an arena installed the scene is streamed BECAUSE its planes exceed the arena: everything taken here is scoped
        # (the chunks' planes used to be carved in both sweeps and never given back -> "arena exhausted" on the refused image of a
        # streamed scene) -- the logits workspace and the planes KEPT from sweep 1 to sweep 2 live until the end of the call, a chunk that is not
        # kept gives its planes back as soon as its pass is enqueued (reuse is ordered by the stream).
        with ops.arena_scope():
            ws = ops.big_empty(ops.score_topk_workspace_bytes(min(chunk, r), b, k, planes=planes_mode), torch.uint8, dev)
            n_c = min(chunk, r)
            per_ray = 1536 if f16 else 4 * ops.D
            if key_cache_bytes is None:
                # 70 % of what is free once the transient needs of ONE chunk are set aside: its key planes (they exist while the chunk is
                # scored, kept or not) and the ray-MLP workspace of sixdgs_ray_keys_ex.  "Free" is the arena's room when the planes come from it.
                transient = n_c * per_ray + int(_lib_ray_keys_ws(n_c, ops.RAY_KEYS_CHUNK_MIN if ops.get_arena() is not None else ops.RAY_KEYS_CHUNK))
                arena = ops.get_arena()
                from_arena = arena is not None and planes_mode and arena.buf.device == dev
                room = (arena.capacity - arena.mark()) if from_arena else torch.cuda.mem_get_info(dev)[0]
                key_cache_bytes = max(0, int(0.7 * (room - transient)))
            kept, kept_bytes = {}, 0                                                  # r0 -> key operand of the chunk, sweep 1 -> sweep 2

            def chunk_keys(r0):
                r1 = min(r0 + chunk, r)
                o, d, c = rays_ori[r0:r1], rays_dir[r0:r1], rays_rgb[r0:r1]             # row slices of contiguous [R,3]: contiguous views
                if not planes_mode:
                    _, key = ops.ray_keys(o, d, c, w)
                    return (key, None, None)
                _, _, (planes, scale) = ops.ray_keys(o, d, c, w, want_key=False, want_planes=True)
                return (None, planes, scale)

            def chunk_pass1(r0, may_keep):
                nonlocal kept_bytes
                run = lambda ent: ops.score_pass1(q, n_tok, ent[0], ws, k, key_planes=ent[1], key_scale=ent[2], profile=profile, n_tok_host=n_host)
                if r0 in kept:
                    return run(kept.pop(r0))
                nbytes = (min(r0 + chunk, r) - r0) * per_ray
                if may_keep and kept_bytes + nbytes <= key_cache_bytes:
                    kept[r0], kept_bytes = chunk_keys(r0), kept_bytes + nbytes         # stays taken until the call's scope ends
                    return run(kept[r0])
                with ops.arena_scope():                                                 # one chunk's planes, given back when its pass is enqueued
                    return run(chunk_keys(r0))

            m_g = torch.full((b, ops.MAX_TOKENS), -float("inf"), device=dev)
            s_g = torch.zeros(b, ops.MAX_TOKENS, device=dev)
            for r0 in range(0, r, chunk):                        # sweep 1: statistics
                st = chunk_pass1(r0, True)
                m_c, s_c = st[..., 0], st[..., 1]
                m_n = torch.maximum(m_g, m_c)
                safe = torch.where(torch.isinf(m_n), torch.zeros_like(m_n), m_n)
                s_g = s_g * torch.exp(torch.where(torch.isinf(m_g), torch.full_like(m_g, -float("inf")), m_g - safe)) + \
                    s_c * torch.exp(torch.where(torch.isinf(m_c), torch.full_like(m_c, -float("inf")), m_c - safe))
                m_g = m_n
            glob = torch.stack([m_g, s_g], dim=-1).contiguous()
            best_i = torch.full((b, k), -1, dtype=torch.int64, device=dev)
            best_v = torch.full((b, k), float("nan"), device=dev)
            mass = torch.zeros(b, dtype=torch.float64, device=dev)
            from . import distributed as dd
            for r0 in range(0, r, chunk):                        # sweep 2: scores of the chunk, candidate merge
                chunk_pass1(r0, False)
                idx, val, sc = ops.score_pass2(glob, n_tok, min(r0 + chunk, r) - r0, ws, k, used_planes=planes_mode, want_scores=return_stats)
                if return_stats:
                    mass += sc.double().sum(dim=1)
                gi = torch.where(idx >= 0, idx + r0, idx)
                best_i, best_v = dd.merge_topk(torch.cat([best_i, gi], dim=1), torch.cat([best_v, val], dim=1), 0, k, group=False)
        if return_stats:
            return best_i, best_v, glob, mass
        return best_i, best_v

    @torch.no_grad()
    def test_images(self, imgs, masks, rays_ori, rays_dir, rays_rgb, rays_to_output: int = 100, want_scores: bool = True,
                    workspace: Optional[torch.Tensor] = None, images_in_flight: Optional[int] = None):
        """Batched test_image: returns dict(idx[B,k], values[B,k], scores[B,R]|None, camera_up_dir[B,3], n_tokens[B])."""
        rays_to_output = ops.check_topk(rays_to_output)          # before the image side runs
        toks, fmaps = self.image_tokens(imgs, masks)
        up = self.camera_up(fmaps)
        idx, val, scores = self.score_tokens(toks, rays_ori, rays_dir, rays_rgb, rays_to_output, want_scores, workspace,
                                             images_in_flight)
        tl = list(toks) if (torch.is_tensor(toks) or isinstance(toks, BatchedTokens)) else toks
        return dict(idx=idx, values=val, scores=scores, camera_up_dir=up, n_tokens=[int(t.shape[0]) for t in tl], tokens=tl)

    @torch.no_grad()
    def test_image(self, img: torch.Tensor, mask: torch.Tensor, rays_ori: torch.Tensor, rays_dir: torch.Tensor,
                   rays_rgb: torch.Tensor, rays_to_output: int = 100):
        """identification_module.py:117-133: (indices, values, scores, camera_up_dir, attention_map)."""
        out = self.test_images([img], [mask], rays_ori, rays_dir, rays_rgb, rays_to_output)
        tok = out["tokens"][0]

        def build():
            q = torch.nn.functional.linear(tok, self.attention.q_proj.weight, self.attention.q_proj.bias)
            return torch.softmax((q @ self.ray_keys(rays_ori, rays_dir, rays_rgb).T) / (q.shape[-1] ** 0.5), dim=-1)

        return (out["idx"][0], out["values"][0], out["scores"][0], out["camera_up_dir"][0],
                AttentionMapProxy(tok.shape[0], rays_ori.shape[0], build))

    def run_attention(self, img, mask, rays_ori, rays_dir, rays_rgb):
        """identification_module.py:77-92 (inference): (score, attention_map, features_img_flat, camera_up_dir)."""
        with torch.no_grad():
            t_pe, t_flat, fmap = self.backbone_wrapper(img, mask)
            _, _, scores = self.score_tokens([t_pe], rays_ori, rays_dir, rays_rgb, 1)
            up = self.camera_up(fmap[None])[0]
        return scores[0], AttentionMapProxy(t_pe.shape[0], rays_ori.shape[0]), t_flat, up

    # ---- training path: differentiable, PyTorch-ROCm autograd ------------------------------
    @staticmethod
    def _pe(x: torch.Tensor, freqs: int) -> torch.Tensor:
        """ray_preprocessor.py:3-9: x[..., c] * 2^f laid out channel-major / frequency-minor, [sin | cos]."""
        bands = torch.pow(2.0, torch.arange(freqs, device=x.device, dtype=torch.float32))
        ph = (x.unsqueeze(-1) * bands).flatten(start_dim=-2)
        return torch.cat((ph.sin(), ph.cos()), dim=-1)

    def ray_features_autograd(self, rays_ori, rays_dir, rays_rgb) -> torch.Tensor:
        """RayPreprocessor.forward (ray_preprocessor.py:36-46) with PyTorch ops, for autograd."""
        rp = self.ray_preprocessor
        x = torch.cat((rays_ori, rays_dir, rays_rgb, self._pe(rays_ori, rp.pospe), self._pe(rays_dir, rp.viewpe),
                       self._pe(rays_rgb, rp.rgbpe)), dim=-1)
        if x.is_cuda and self.hip_autograd:          # forward and backward GEMMs on the MFMA kernel (6dgs_amd/autograd.py)
            from . import autograd as hip
            return hip.ray_mlp(rp, x)
        return rp.mlp2(torch.cat((rp.mlp(x), x), dim=-1))

    def forward(self, img: torch.Tensor, mask: torch.Tensor, rays_ori: torch.Tensor, rays_dir: torch.Tensor, rays_rgb: torch.Tensor,
                rays_to_test: int = -1):
        """The TRAINING forward of the reference (identification_module.py:94-115 -> run_attention :77-92): a random permutation of
        the rays, ray MLP, attention over the rays, column sum, camera-up head -- all PyTorch ops on the module's parameters so
        that autograd reaches them (at the reference's 1000-ellipsoid training size, R ~ 3e4, this is a few ms on PyTorch-ROCm;
        the HIP library serves inference, where R is three orders of magnitude larger).  Returns (scores [R'], attention map
        [T, R'], image features [T, 384], camera-up [3], used_ray_ids [R'])."""
        used = torch.randperm(rays_ori.shape[0], device=img.device, dtype=torch.long)
        if rays_to_test != -1:
            used = used[:rays_to_test]
        t_pe, t_flat, fmap = self.backbone_wrapper(img, mask)
        feat = self.ray_features_autograd(rays_ori[used], rays_dir[used], rays_rgb[used])
        if feat.is_cuda and self.hip_autograd:
            from . import autograd as hip
            q = hip.linear(t_pe, self.attention.q_proj.weight, self.attention.q_proj.bias)
            k = hip.linear(feat, self.attention.k_proj.weight, self.attention.k_proj.bias)
        else:
            q, k = self.attention.q_proj(t_pe), self.attention.k_proj(feat)
        attention_map = torch.softmax((q @ k.transpose(-2, -1)) / (q.shape[-1] ** 0.5), dim=-1)
        scores = attention_map.sum(dim=0)
        up = torch.nn.functional.normalize(self.camera_direction_prediction_network(fmap), dim=-1)
        return scores, attention_map, t_flat, up, used

    def forward_window(self, imgs, masks, rays_ori: torch.Tensor, rays_dir: torch.Tensor, rays_rgb: torch.Tensor, ray_groups: int = 1):
        """The training forward of a whole window of images at once (train_id_module(batched_window=True)).  Every image of the window
        is scored against the SAME keys K = k_proj(ray MLP(rays)), so the ray side runs once -- on the rays as given, unpermuted: the
        scores are permutation-equivariant and the loss is a mean over the rays -- and its backward receives the gradient of all images
        at once.  The image side is frozen (one batch through image_tokens, no autograd); q_proj, the scorer (ops.ray_attention_scores:
        the two-pass scorer forward, sixdgs_score_backward) and the camera-up CNN carry gradients.  On the CPU or with hip_autograd False
        the scorer is PyTorch's softmax and column sum per image.  imgs / masks as image_tokens takes them (mask None = every pixel; a mask
        selects the image's tokens by boolean indexing, the one host sync of a window with masked images).  ray_groups: the split of the
        scorer's backward over the rays (ops.ray_attention_scores; 1 = unsplit, 0 = auto; ignored by the PyTorch scorer).
        Returns (scores [B,R], camera-up [B,3] (unit), token counts [B] as a host list)."""
        toks, fmaps = self.image_tokens(imgs, masks)
        if isinstance(toks, BatchedTokens):
            toks = toks.dense()
        device = rays_ori.device
        if torch.is_tensor(toks):                       # every image keeps all its tokens
            b, n_host = toks.shape[0], [int(toks.shape[1])] * toks.shape[0]
            tokens = toks
        else:
            b, n_host = len(toks), [int(t.shape[0]) for t in toks]
            tokens = toks[0].new_zeros(b, ops.MAX_TOKENS, toks[0].shape[-1])
            for i, t in enumerate(toks):
                tokens[i, : t.shape[0]] = t
        feat = self.ray_features_autograd(rays_ori, rays_dir, rays_rgb)
        at = self.attention
        if feat.is_cuda and self.hip_autograd:
            from . import autograd as hip
            n_tok = self._full_ntok(b, device) if all(n == ops.MAX_TOKENS for n in n_host) else \
                torch.stack([torch.full((), n, dtype=torch.int32, device=device) for n in n_host])      # device-side: no host copy
            q = hip.linear(tokens.reshape(b * ops.MAX_TOKENS, -1), at.q_proj.weight, at.q_proj.bias).view(b, ops.MAX_TOKENS, -1)
            k = hip.linear(feat, at.k_proj.weight, at.k_proj.bias)
            scores = ops.ray_attention_scores(q, n_tok, k, ray_groups)
        else:
            q, k = at.q_proj(tokens), at.k_proj(feat)
            scale = q.shape[-1] ** 0.5
            scores = torch.stack([torch.softmax((q[i, :n] @ k.transpose(-2, -1)) / scale, dim=-1).sum(dim=0) for i, n in enumerate(n_host)])
        up = torch.nn.functional.normalize(self.camera_direction_prediction_network(fmaps), dim=-1)
        return scores, up, n_host
