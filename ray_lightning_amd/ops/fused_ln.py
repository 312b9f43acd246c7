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
    return c % v == 0 and c // v <= 16384 and _load_ext() is not None


class _FusedLN(torch.autograd.Function):
    """Plain LayerNorm: x -> ln(x)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = _load_ext()
        x = x.contiguous()
        y, _x_new, mean, invstd = ext.fused_ln_fwd(
            x, None, weight, bias, eps)
        ctx.save_for_backward(x, mean, invstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight = ctx.saved_tensors
        ext = _load_ext()
        dx, dgamma, dbeta = ext.fused_ln_bwd(
            dy, x, None, weight, mean, invstd)
        return dx, dgamma, dbeta, None


class _FusedAddLN(torch.autograd.Function):
    """(residual, sub_out) -> (x_new = residual + sub_out, ln(x_new))."""

    @staticmethod
    def forward(ctx, residual, sub_out, weight, bias, eps):
        ext = _load_ext()
        y, x_new, mean, invstd = ext.fused_ln_fwd(
            residual.contiguous(), sub_out.contiguous(), weight, bias,
            eps)
        ctx.save_for_backward(x_new, mean, invstd, weight)
        return x_new, y

    @staticmethod
    def backward(ctx, d_xnew, dy):
        x_new, mean, invstd, weight = ctx.saved_tensors
        ext = _load_ext()
        dext = d_xnew.contiguous() if d_xnew is not None else None
        dx, dgamma, dbeta = ext.fused_ln_bwd(
            dy, x_new, dext, weight, mean, invstd)
        # x_new = residual + sub_out: both get the same gradient
        return dx, dx, dgamma, dbeta, None


class _FusedDropoutAddLN(torch.autograd.Function):
    """(sub_out, residual | None) -> (x_new, ln(x_new)) with
    ``x_new = residual + keep * sub_out / (1-p)`` (``residual`` absent:
    ``keep * sub_out / (1-p)``). The mask is a function of the (seed,
    offset) pair the forward kernel drew from the device's default
    generator; the pair is kept on ctx as two ints and backward draws
    the mask again from it. Saved tensors are those of ``_FusedAddLN``."""

    @staticmethod
    def forward(ctx, sub_out, residual, weight, bias, eps, p):
        ext = _load_ext()
        y, x_new, mean, invstd, seed, offset = ext.fused_dropout_ln_fwd(
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
        d_res, d_sub, dgamma, dbeta = ext.fused_dropout_ln_bwd(
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
    kernels."""
    _check_p(p)
    drop = p > 0.0 and training
    if _ln_fusable(sub_out, weight):
        if drop:
            return _FusedDropoutAddLN.apply(sub_out, residual, weight,
                                            bias, eps, p)
        if residual is None:
            return sub_out, _FusedLN.apply(sub_out, weight, bias, eps)
        return _FusedAddLN.apply(residual, sub_out, weight, bias, eps)
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
        if dropout_p != 0.0:
            _check_p(dropout_p)
            if self.training:
                return dropout_add_layer_norm(
                    x, residual, self.weight, self.bias, self.eps,
                    dropout_p, True)
            if residual is None:
                return x, self.forward(x)
        if _ln_fusable(x, self.weight):
            if residual is None:
                return _FusedLN.apply(x, self.weight, self.bias,
                                      self.eps)
            return _FusedAddLN.apply(residual, x, self.weight,
                                     self.bias, self.eps)
        if residual is None:
            return super().forward(x)
        x_new = residual + x
        return x_new, super().forward(x_new)
