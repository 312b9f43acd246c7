"""FusedBatchNorm2d: hand-written CDNA4 NHWC BN(+ReLU)(+residual).

Replaces the MIOpen BN kernel set plus the separate residual-add and
ReLU elementwise kernels that together dominate the ResNet-50 training
step on MI355X (profiles/r01_resnet50_1gpu_fixedfind.md: BN ~34% +
elementwise ~22% of step time vs convs ~33%). The fused train forward
makes 2 passes over the activation instead of eager's 7 tensor
traversals; the backward 2 instead of 5.

Drop-in: ``FusedBatchNorm2d`` subclasses ``nn.BatchNorm2d`` (same
parameters/buffers/state_dict). The fused HIP path engages on GPU for
channels_last bf16/fp32 inputs; anything else falls back to composed
torch ops so CPU tests and odd shapes stay correct.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from . import _load_ext


def _fusable(x: torch.Tensor, c: int) -> bool:
    if not x.is_cuda or x.dim() != 4:
        return False
    if x.dtype not in (torch.bfloat16, torch.float32):
        return False
    v = 8 if x.dtype == torch.bfloat16 else 4
    if c % v or c // v > 256:
        return False
    return x.is_contiguous(memory_format=torch.channels_last) and \
        _load_ext() is not None


class _FusedBNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean,
                running_var, training, momentum, eps, relu):
        ext = _load_ext()
        res_opt = residual
        y, mean, invstd, mask = ext.fused_bn_fwd(
            x, weight, bias,
            running_mean if running_mean is not None else torch.Tensor(),
            running_var if running_var is not None else torch.Tensor(),
            res_opt, relu, training, momentum, eps)
        ctx.relu = relu
        ctx.has_res = residual is not None
        # the ReLU bitmask (1 byte / 8 elems) replaces saving+re-reading
        # y in backward
        ctx.save_for_backward(x, mask, mean, invstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, mean, invstd, weight = ctx.saved_tensors
        ext = _load_ext()
        outs = ext.fused_bn_bwd(dy, mask, x, mean, invstd, weight,
                                ctx.relu, ctx.has_res)
        dx, dgamma, dbeta = outs[0], outs[1], outs[2]
        dres = outs[3] if ctx.has_res else None
        return (dx, dres, dgamma, dbeta, None, None, None, None, None,
                None)


class _FusedBNReluPoolFunction(torch.autograd.Function):
    """BN(train) + ReLU + MaxPool2d(3, 2, 1). Saves x and a 4-bit argmax
    code per pooled element: no full-resolution y, ReLU mask, int64
    indices or full-resolution pool gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps):
        ext = _load_ext()
        pooled, mean, invstd, code = ext.fused_bn_relu_pool_fwd(
            x, weight, bias,
            running_mean if running_mean is not None else torch.Tensor(),
            running_var if running_var is not None else torch.Tensor(),
            momentum, eps)
        ctx.save_for_backward(x, code, mean, invstd, weight)
        return pooled

    @staticmethod
    def backward(ctx, dpool):
        x, code, mean, invstd, weight = ctx.saved_tensors
        dx, dgamma, dbeta = _load_ext().fused_bn_relu_pool_bwd(
            dpool, code, x, mean, invstd, weight)
        return dx, dgamma, dbeta, None, None, None, None


class _FusedDualBNFunction(torch.autograd.Function):
    """relu(BN3(x3) + BNd(xd)), both in training mode: the identity
    branch's BN output and its gradient are never materialised."""

    @staticmethod
    def forward(ctx, x3, xd, w3, b3, rm3, rv3, wd, bd, rmd, rvd,
                momentum3, momentumd, eps3, epsd):
        def _t(t):
            return t if t is not None else torch.Tensor()
        y, mean3, invstd3, meand, invstdd, mask = \
            _load_ext().fused_bn_dual_fwd(
                x3, xd, w3, b3, _t(rm3), _t(rv3), wd, bd, _t(rmd),
                _t(rvd), momentum3, momentumd, eps3, epsd)
        ctx.save_for_backward(x3, xd, mask, mean3, invstd3, w3, meand,
                              invstdd, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x3, xd, mask, mean3, invstd3, w3, meand, invstdd, wd = \
            ctx.saved_tensors
        dx3, dxd, dg3, db3, dgd, dbd = _load_ext().fused_bn_dual_bwd(
            dy, mask, x3, xd, mean3, invstd3, w3, meand, invstdd, wd)
        return (dx3, dxd, dg3, db3, None, None, dgd, dbd, None, None,
                None, None, None, None)


def bn_fusions_enabled() -> bool:
    """``RLA_BN_FUSIONS=0`` keeps the stem (BN+ReLU+maxpool) and the
    downsample junction (dual BN) on the composed path. Models read it
    once, at construction."""
    return os.environ.get("RLA_BN_FUSIONS", "1") != "0"


def _pool_is_3_2_1(pool: nn.Module) -> bool:
    def _is(v, want):
        return v == want or v == (want, want)
    return isinstance(pool, nn.MaxPool2d) and \
        _is(pool.kernel_size, 3) and _is(pool.stride, 2) and \
        _is(pool.padding, 1) and _is(pool.dilation, 1) and \
        not pool.ceil_mode and not pool.return_indices


class FusedBatchNorm2d(nn.BatchNorm2d):
    """BatchNorm2d with optional fused ReLU and fused residual add.

    ``forward(x)`` == BN(x) [+ReLU]; ``forward(x, residual)`` ==
    ReLU?(BN(x) + residual) — the three fusion shapes a ResNet
    bottleneck needs (bn+relu, plain bn for the downsample branch,
    bn+add+relu for the block output). ``forward_pool`` and
    ``forward_dual`` fuse one step further at the stem and at the
    downsample junction."""

    def __init__(self, num_features: int, relu: bool = False, **kwargs):
        super().__init__(num_features, **kwargs)
        self.relu = relu

    def _kernel_ready(self, x: torch.Tensor) -> bool:
        return _fusable(x, self.num_features) and \
            self.weight is not None and \
            self.weight.dtype == torch.float32

    def _step_momentum(self) -> float:
        """Count one training batch and return the running-stat factor
        the kernel binds as a double."""
        if self.track_running_stats and \
                self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        # momentum=None means cumulative moving average
        # (nn.BatchNorm2d semantics): effective factor is
        # 1/num_batches_tracked.
        momentum = self.momentum
        if momentum is None:
            momentum = (1.0 / float(self.num_batches_tracked)
                        if (self.track_running_stats and
                            self.num_batches_tracked is not None and
                            int(self.num_batches_tracked) > 0)
                        else 0.0)
        return momentum

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        training = self.training
        if self._kernel_ready(x) and \
                (residual is None or residual.dtype == x.dtype) and \
                (training or (not torch.is_grad_enabled()
                              and self.running_mean is not None)):
            if residual is not None:
                residual = residual.contiguous(
                    memory_format=torch.channels_last)
            momentum = self._step_momentum() if training else 0.0
            return _FusedBNFunction.apply(
                x, residual, self.weight, self.bias, self.running_mean,
                self.running_var, training, momentum, self.eps,
                self.relu)
        # composed fallback (CPU, odd channel counts, missing ext)
        out = super().forward(x)
        if residual is not None:
            out = out + residual
        if self.relu:
            out = torch.relu(out)
        return out

    def forward_pool(self, x: torch.Tensor,
                     pool: nn.Module) -> torch.Tensor:
        """``pool(self(x))``; one fused BN+ReLU+maxpool kernel set when
        training with ReLU and ``pool`` is MaxPool2d(3, stride 2,
        padding 1)."""
        if self.training and self.relu and _pool_is_3_2_1(pool) and \
                self._kernel_ready(x) and x.numel() < 2 ** 31:
            return _FusedBNReluPoolFunction.apply(
                x, self.weight, self.bias, self.running_mean,
                self.running_var, self._step_momentum(), self.eps)
        return pool(self(x))

    def forward_dual(self, x: torch.Tensor, other_x: torch.Tensor,
                     other_bn: nn.Module) -> torch.Tensor:
        """``self(x, other_bn(other_x))``; one fused dual-BN kernel set
        when both are training-mode FusedBatchNorm2d over same-shaped
        inputs, ``self`` with ReLU and ``other_bn`` without."""
        if self.training and self.relu and \
                isinstance(other_bn, FusedBatchNorm2d) and \
                other_bn.training and not other_bn.relu and \
                other_x.shape == x.shape and other_x.dtype == x.dtype and \
                self._kernel_ready(x) and other_bn._kernel_ready(other_x):
            momentumd = other_bn._step_momentum()
            return _FusedDualBNFunction.apply(
                x, other_x, self.weight, self.bias, self.running_mean,
                self.running_var, other_bn.weight, other_bn.bias,
                other_bn.running_mean, other_bn.running_var,
                self._step_momentum(), momentumd, self.eps, other_bn.eps)
        return self(x, other_bn(other_x))
