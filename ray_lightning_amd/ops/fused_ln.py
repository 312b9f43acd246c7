"""FusedLayerNorm + fused residual-add+LayerNorm (CDNA4 row kernels).

Transformer pre-norm blocks compute ``x = x + sublayer(ln(x))``: the
fused op merges the residual add into the next LayerNorm's forward (one
read of each input, one write of x_new and the normalized output) and
the whole chain's backward into two passes (see ops/csrc/fused_ln.hip).
ATen's path is add + vectorized_layer_norm forward and
layer_norm_grad_input + cuComputePartGradGammaBeta (+fold) + add-grad
backward — ~8 ms/step of the GPT-2-XL profile
(profiles/r01_gpt2xl_1gpu_baseline.md).

Residual / embedding dropout rides in the same kernels
(``dropout_add_layer_norm``): ``x_new = residual + dropout(sub_out)``
with the keep mask drawn from a counter-based RNG in forward and drawn
again in backward, so no mask is stored and no extra pass is made.

Falls back to composed torch ops off-GPU / unsupported shapes.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _load_ext


def _ln_fusable(x: torch.Tensor, weight: torch.Tensor) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    if weight is None or weight.dtype != torch.float32:
        return False
    v = 8 if x.dtype == torch.bfloat16 else 4
    c = x.shape[-1]
    return c % v == 0 and c <= 16384 and _load_ext() is not None


class _FusedLN(torch.autograd.Function):
    """Plain LayerNorm: x -> ln(x)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = _load_ext()
        x = x.contiguous()
        y, _x_new, mean, invstd, _seed, _offset = ext.fused_ln_fwd(
            x, None, weight, bias, eps, 0.0)
        ctx.save_for_backward(x, mean, invstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight = ctx.saved_tensors
        ext = _load_ext()
        _d_res, dx, dgamma, dbeta = ext.fused_ln_bwd(
            dy, x, None, weight, mean, invstd, 0.0, 0, 0, False)
        return dx, dgamma, dbeta, None


class _FusedAddLN(torch.autograd.Function):
    """(sub_out, residual | None) -> (x_new, ln(x_new)) with
    ``x_new = residual + keep * sub_out / (1-p)`` (``residual`` absent:
    ``keep * sub_out / (1-p)``; ``p == 0``: ``keep = 1`` and the
    generator is not touched). The mask is a function of the (seed,
    offset) pair the forward kernel drew from the device's default
    generator; the pair is kept on ctx as two ints and backward draws
    the mask again from it. Nothing mask-sized is saved."""

    @staticmethod
    def forward(ctx, sub_out, residual, weight, bias, eps, p):
        ext = _load_ext()
        y, x_new, mean, invstd, seed, offset = ext.fused_ln_fwd(
            sub_out.contiguous(),
            residual.contiguous() if residual is not None else None,
            weight, bias, eps, p)
        ctx.save_for_backward(x_new, mean, invstd, weight)
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        ctx.has_res = residual is not None
        return x_new, y

    @staticmethod
    def backward(ctx, d_xnew, dy):
        x_new, mean, invstd, weight = ctx.saved_tensors
        ext = _load_ext()
        dext = d_xnew.contiguous() if d_xnew is not None else None
        # p == 0: d_res and d_sub are one buffer, both inputs get it
        d_res, d_sub, dgamma, dbeta = ext.fused_ln_bwd(
            dy, x_new, dext, weight, mean, invstd, ctx.p, ctx.seed,
            ctx.offset, ctx.has_res)
        return d_sub, d_res, dgamma, dbeta, None, None


def _check_p(p: float) -> None:
    if not 0.0 <= p < 1.0:
        raise ValueError(
            f"dropout probability has to be in [0, 1), but got {p}")


def dropout_add_layer_norm(sub_out: torch.Tensor,
                           residual: Optional[torch.Tensor],
                           weight: torch.Tensor, bias: torch.Tensor,
                           eps: float, p: float, training: bool = True):
    """``x_new = residual + dropout(sub_out, p)`` (``residual=None``:
    just the dropout) and ``y = layer_norm(x_new)``; returns
    ``(x_new, y)``. One HIP kernel each way on GPU. With ``p == 0`` or
    ``training=False`` it is the dropout-free op, on the dropout-free
    instantiations of the same kernels, and ``residual=None`` returns
    ``sub_out`` itself as ``x_new``."""
    _check_p(p)
    drop = p > 0.0 and training
    if _ln_fusable(sub_out, weight):
        if not drop and residual is None:
            return sub_out, _FusedLN.apply(sub_out, weight, bias, eps)
        return _FusedAddLN.apply(sub_out, residual, weight, bias, eps,
                                 p if drop else 0.0)
    if drop:
        sub_out = F.dropout(sub_out, p, True)
    x_new = sub_out if residual is None else residual + sub_out
    return x_new, F.layer_norm(x_new, (x_new.shape[-1],), weight, bias,
                               eps)


class FusedLayerNorm(nn.LayerNorm):
    """Drop-in ``nn.LayerNorm`` with the fused HIP path; also provides
    ``forward(sub_out, residual=prev_x)`` -> ``(x_new, ln(x_new))`` for
    pre-norm residual chains. ``dropout_p > 0`` drops ``sub_out`` inside
    the same kernel in training mode and always returns the pair
    (``residual=None``: ``x_new = dropout(x)``; eval: ``x_new = x``)."""

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None,
                dropout_p: float = 0.0):
        if residual is None and dropout_p == 0.0:
            if _ln_fusable(x, self.weight):
                return _FusedLN.apply(x, self.weight, self.bias,
                                      self.eps)
            return super().forward(x)
        return dropout_add_layer_norm(
            x, residual, self.weight, self.bias, self.eps, dropout_p,
            self.training)
