"""Differentiable dense layers of the scorer on the hand-written MFMA GEMM (backward for the ray MLP and
q_proj / k_proj), for the on-box training of IdentificationModule (pose_estimation/train.py:106-170 drives
identification_module.py:94-115 -> ray_preprocessor.py:36-46 and our_multihead_attention.py:70-79 through autograd).

One torch.autograd.Function, `HipLinear`: y = act(x w^T + b) with all three products of the layer on `sixdgs_linear`
(gemm.hip: 128x128 tiles, fp32 operands as 3 bf16 planes x 6 MFMA terms, fp32-equivalent):

    forward   y   = x  . w^T            [M,K] x [N,K] -> [M,N]     (bias + ReLU in the kernel's epilogue)
    backward  dx  = dy . w              as dy [M,N] x (w^T) [K,N]   -> [M,K]   (when K is a multiple of 128; N zero-padded to a
                                                                                 multiple of 16: the kernel's K constraint)
              dw^T = x^T . dy           as x^T [K,M] x (dy^T) [N,M] -> [K,N]   (M zero-padded to a multiple of 16: the kernel's K constraint)
              db  = column sums of dy   (PyTorch reduction)

The kernel takes any M >= 0 and N > 0 but wants its contraction length K to be a multiple of 4, so the callers pad the
reference's odd widths (141, 653, 398) to multiples of 16 with zeros -- exact in value.  dx for a K that is not a multiple of
128 is only ever needed for inputs without gradient on this path (ray encodings, image tokens of a frozen backbone); if it is
requested anyway it is formed by a PyTorch matmul, said so in the name.  With M = 0 every gradient is zero and no GEMM runs (dW
would be a contraction of length 0, and an empty dy may carry any strides).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops


class HipLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, relu: bool):
        y = ops.linear(x, w, b, relu=relu, split_k=1)
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.relu, ctx.has_bias = relu, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        if x.shape[0] == 0:         # no rows: zero gradients, no GEMM (the kernel rejects a contraction of length 0)
            return (torch.zeros_like(x) if need[0] else None, torch.zeros_like(w) if need[1] else None,
                    w.new_zeros(w.shape[0]) if ctx.has_bias and need[2] else None, None)
        dy = dy.contiguous()
        if ctx.relu:
            dy = dy * (y > 0)
        dx = dw = db = None
        m, k = x.shape
        if ctx.needs_input_grad[0]:
            if k % 128 == 0:
                dyp, wt, padn = dy, w.t().contiguous(), (-w.shape[0]) % 16
                if padn:
                    dyp, wt = F.pad(dy, (0, padn)), F.pad(wt, (0, padn))
                dx = ops.linear(dyp, wt, None, split_k=1)
            else:
                dx = dy @ w                                              # PyTorch matmul (rocBLAS)
        if ctx.needs_input_grad[1]:
            pad = (-m) % 16
            xt, dyt = x.t().contiguous(), dy.t().contiguous()
            if pad:
                xt, dyt = F.pad(xt, (0, pad)), F.pad(dyt, (0, pad))
            dw = ops.linear(xt, dyt, None, split_k=1).t()                # [K,N] -> [N,K]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(dim=0)
        return dx, dw, db, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias, relu: bool = False) -> torch.Tensor:
    """act(x weight^T + bias) through HipLinear; the input width is zero-padded to a multiple of 16 when needed."""
    k = x.shape[-1]
    pad = (-k) % 16
    if pad:
        x, weight = F.pad(x, (0, pad)), F.pad(weight, (0, pad))
    return HipLinear.apply(x.contiguous(), weight.contiguous(), bias, relu)


def ray_mlp(rp, x: torch.Tensor) -> torch.Tensor:
    """RayPreprocessor.forward (ray_preprocessor.py:36-46) on the encoded input x [R,141]: mlp, then mlp2 on cat([h, x]) -- evaluated as
    h W3[:, :512]^T + x W3[:, 512:]^T so that the gradient with respect to h (K = 512) runs on the kernel too."""
    h = linear(x, rp.mlp[0].weight, rp.mlp[0].bias, relu=True)
    h = linear(h, rp.mlp[2].weight, rp.mlp[2].bias, relu=True)
    w3, hid = rp.mlp2[0].weight, rp.mlp[2].weight.shape[0]
    z = linear(h, w3[:, :hid], rp.mlp2[0].bias) + linear(x, w3[:, hid:], None)
    return linear(torch.relu(z), rp.mlp2[2].weight, rp.mlp2[2].bias)


class RasterViews(torch.autograd.Function):
    """image_f32 of ops.raster_views, differentiable in the six scene tensors and cams (ops.raster_views_backward).  ctx keeps the
    forward's workspace: the backward reads the records, the tile ranges and the sorted instances from it, no second sort."""

    @staticmethod
    def forward(ctx, xyz, scale, rot, opacity, f_dc, f_rest, cams, sh_degree, width, height, kw):
        image, state = ops.raster_views(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree, cams, width, height, want_float=True,
                                        want_u8=False, want_state=True, **kw)
        ctx.save_for_backward(xyz, scale, rot, opacity, f_dc, f_rest, cams)
        ctx.state, ctx.args = state, (sh_degree, width, height, {k: v for k, v in kw.items() if k != "max_instances"})
        return image

    @staticmethod
    def backward(ctx, grad_image):
        inputs = ctx.saved_tensors
        sh_degree, width, height, kw = ctx.args
        want = tuple(name for name, need in zip(ops.RASTER_GRADIENTS, ctx.needs_input_grad[:7]) if need)
        if not want:
            return (None,) * 11
        grads = ops.raster_views_backward(*inputs[:6], sh_degree, inputs[6], width, height, grad_image, ctx.state, want=want, **kw)
        return tuple(None if g is None else g.to(x.dtype) for g, x in zip(grads, inputs)) + (None,) * 4


def raster_views(xyz, scale, rot, opacity, f_dc, f_rest, sh_degree: int, cams: torch.Tensor, width: int, height: int, *, background,
                 scale_modifier: float = 1.0, scale_is_log: bool = True, opacity_is_logit: bool = True, max_instances=None):
    """The float image [V,height,width,4] (rgb, 1 - T) of ops.raster_views, differentiable in xyz, scale, rot, opacity, f_dc, f_rest
    and cams [V,16] (the 12 w2c entries as free numbers, fx, fy, cx, cy); the gradient is the one sixdgs_raster_views_backward in
    include/sixdgs.h defines.  The forward retries on an instance overflow as ops.raster_views does."""
    kw = dict(background=tuple(float(b) for b in background), scale_modifier=float(scale_modifier), scale_is_log=bool(scale_is_log),
              opacity_is_logit=bool(opacity_is_logit), max_instances=max_instances)
    return RasterViews.apply(xyz, scale, rot, opacity, f_dc, f_rest, cams, int(sh_degree), int(width), int(height), kw)


class PhotometricLoss(torch.autograd.Function):
    """loss [V] of ops.photometric_loss, differentiable in the image.  The forward asks the one C call for the gradient as well, with
    grad_loss = 1; the backward scales it per view."""

    @staticmethod
    def forward(ctx, image, target, lambda_dssim: float):
        if not ctx.needs_input_grad[0]:
            return ops.photometric_loss(image, target, lambda_dssim=lambda_dssim)
        loss, grad = ops.photometric_loss(image, target, lambda_dssim=lambda_dssim, want_grad=True)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        out = grad * grad_loss.to(grad.dtype).reshape(-1, 1, 1, 1)
        if out.shape[3] == 4:
            out[..., 3] = 0.0           # exact zero, as the C call writes it (0 x a negative grad_loss would be -0)
        return out, None, None


def photometric_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """(1 - lambda) L1 + lambda (1 - SSIM) per view [V] (sixdgs_photometric_loss in include/sixdgs.h), differentiable in image fp32
    [V,H,W,3|4]; target fp32 [V,H,W,3|4] or uint8 [V,H,W,3], a constant."""
    return PhotometricLoss.apply(image, target, float(lambda_dssim))
