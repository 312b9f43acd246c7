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

``FusedSyncBatchNorm2d`` / ``convert_sync_batchnorm`` (end of this file)
take the training-mode statistics over all ranks of a communicator, on
the same kernels cut where the per-channel sums exist.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from . import _load_ext


def _fusable(x: torch.Tensor, c: int) -> bool:
    """What the extension's operand check admits as the activation."""
    if not x.is_cuda or x.dim() != 4 or x.numel() == 0:
        return False
    if x.dtype not in (torch.bfloat16, torch.float32):
        return False
    v = 8 if x.dtype == torch.bfloat16 else 4
    tpr = c // v
    # a power-of-two C/V: only then do the stage-1 reduction trees cover
    # every row of a block
    if c % v or tpr > 256 or tpr & (tpr - 1):
        return False
    return x.is_contiguous(memory_format=torch.channels_last) and \
        _load_ext() is not None


def _or_empty(t: Optional[torch.Tensor]) -> torch.Tensor:
    """The extension takes an empty tensor for "no running stats"."""
    return t if t is not None else torch.Tensor()


class _FusedBNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean,
                running_var, training, momentum, eps, relu):
        y, mean, invstd, mask = _load_ext().fused_bn_fwd(
            x, weight, bias, _or_empty(running_mean),
            _or_empty(running_var), residual, relu, training, momentum,
            eps)
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
            x, weight, bias, _or_empty(running_mean),
            _or_empty(running_var), momentum, eps)
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
        y, mean3, invstd3, meand, invstdd, mask = \
            _load_ext().fused_bn_dual_fwd(
                x3, xd, w3, b3, _or_empty(rm3), _or_empty(rv3), wd, bd,
                _or_empty(rmd), _or_empty(rvd), momentum3, momentumd,
                eps3, epsd)
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

    def _sync_active(self) -> bool:
        """True when this forward reduces its statistics across ranks
        (``FusedSyncBatchNorm2d`` in training mode with more than one
        rank). The stem and junction fusions then stay composed."""
        return False

    def forward_pool(self, x: torch.Tensor,
                     pool: nn.Module) -> torch.Tensor:
        """``pool(self(x))``; one fused BN+ReLU+maxpool kernel set when
        training with ReLU and ``pool`` is MaxPool2d(3, stride 2,
        padding 1)."""
        if self.training and self.relu and _pool_is_3_2_1(pool) and \
                not self._sync_active() and \
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
                not self._sync_active() and \
                not other_bn._sync_active() and \
                other_x.shape == x.shape and other_x.dtype == x.dtype and \
                self._kernel_ready(x) and other_bn._kernel_ready(other_x):
            momentumd = other_bn._step_momentum()
            return _FusedDualBNFunction.apply(
                x, other_x, self.weight, self.bias, self.running_mean,
                self.running_var, other_bn.weight, other_bn.bias,
                other_bn.running_mean, other_bn.running_var,
                self._step_momentum(), momentumd, self.eps, other_bn.eps)
        return self(x, other_bn(other_x))


# ---------------------------------------------------------------------
# synchronized BN: batch statistics over all ranks
#
# The forward and the backward are each cut where the per-channel sums
# exist; the sums are all-reduced there and the coefficients derived
# from the global sums and the global row count. Each of the four
# phases has a HIP backend (the extension's fused_bn_sync_* entry
# points) and a torch twin that forms the same fp32 sums, so CPU runs go
# through the same communication choreography.
#   sums  = [sum(x) | sum(x^2) | row count]     fp32 [2C+1]
#   bsums = [sum(dy_eff) | sum(dy_eff * xhat)]  fp32 [2C]
# ---------------------------------------------------------------------
def _per_channel(v: torch.Tensor) -> torch.Tensor:
    return v.view(1, -1, 1, 1)


def _twin_stats(x: torch.Tensor) -> torch.Tensor:
    c = x.shape[1]
    xw = x.to(torch.promote_types(x.dtype, torch.float32))
    count = xw.new_full((1,), x.numel() // c)
    return torch.cat([xw.sum(dim=(0, 2, 3)), (xw * xw).sum(dim=(0, 2, 3)),
                      count]).float()


def _twin_apply(x, sums, weight, bias, running_mean, running_var, res,
                relu, momentum, eps):
    c = x.shape[1]
    count = sums[2 * c]
    mean = sums[:c] / count
    var = (sums[c:2 * c] / count - mean * mean).clamp_min(0.0)
    invstd = torch.rsqrt(var + eps)
    if running_mean is not None:
        var_unb = torch.where(count > 1, var * count / (count - 1), var)
        running_mean.mul_(1.0 - momentum).add_(
            mean.to(running_mean.dtype), alpha=momentum)
        running_var.mul_(1.0 - momentum).add_(
            var_unb.to(running_var.dtype), alpha=momentum)
    scale = invstd if weight is None else weight.float() * invstd
    shift = -mean * scale
    if bias is not None:
        shift = shift + bias.float()
    out_dtype = x.dtype if res is None else \
        torch.result_type(x, res)
    y = x.float() * _per_channel(scale) + _per_channel(shift)
    if res is not None:
        y = y + res.float()
    mask = None
    if relu:
        mask = y > 0
        y = torch.relu(y)
    return y.to(out_dtype), mean, invstd, mask


def _twin_dy_eff(dy, mask, relu):
    d = dy.float()
    return d * mask if relu else d


def _twin_bwd_reduce(dy, mask, x, mean, invstd, relu):
    d = _twin_dy_eff(dy, mask, relu)
    xhat = (x.float() - _per_channel(mean)) * _per_channel(invstd)
    return torch.cat([d.sum(dim=(0, 2, 3)), (d * xhat).sum(dim=(0, 2, 3))])


def _twin_bwd_dx(dy, mask, x, mean, invstd, weight, bsums, count, relu):
    """dx = P*dy_eff + Q*x + S with the coefficients of
    bn_bwd_coef_kernel; also returns dy_eff (the residual's gradient)."""
    c = x.shape[1]
    d = _twin_dy_eff(dy, mask, relu)
    p = invstd if weight is None else weight.float() * invstd
    q = -p * invstd * bsums[c:] / count
    s = -p * bsums[:c] / count - q * mean
    dx = _per_channel(p) * d + _per_channel(q) * x.float() + \
        _per_channel(s)
    return dx.to(x.dtype), d


class _FusedSyncBNFunction(torch.autograd.Function):
    """Training-mode BN(+ReLU)(+residual) with statistics over all ranks
    of ``comm``. One all-reduce in forward, one in backward, both
    synchronous on the caller's stream."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean,
                running_var, momentum, eps, relu, comm, use_ext):
        c = x.shape[1]
        if use_ext:
            ext = _load_ext()
            sums = ext.fused_bn_sync_stats(x)
        else:
            sums = _twin_stats(x)
        comm.all_reduce_(sums, op="sum", async_op=False)
        if use_ext:
            y, mean, invstd, mask = ext.fused_bn_sync_apply(
                x, sums, weight, bias, _or_empty(running_mean),
                _or_empty(running_var), residual, relu, momentum, eps)
        else:
            y, mean, invstd, mask = _twin_apply(
                x, sums, weight, bias, running_mean, running_var,
                residual, relu, momentum, eps)
        ctx.relu = relu
        ctx.use_ext = use_ext
        ctx.comm = comm
        ctx.res_dtype = None if residual is None else residual.dtype
        # the global row count stays on the device for backward
        ctx.save_for_backward(x, mask, mean, invstd, weight,
                              sums[2 * c:])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, mean, invstd, weight, count = ctx.saved_tensors
        c = x.shape[1]
        has_res = ctx.res_dtype is not None
        if ctx.use_ext:
            ext = _load_ext()
            bsums = ext.fused_bn_sync_bwd_reduce(dy, mask, x, mean,
                                                 invstd, ctx.relu)
        else:
            bsums = _twin_bwd_reduce(dy, mask, x, mean, invstd, ctx.relu)
        # dgamma/dbeta stay this rank's sums (torch.nn.SyncBatchNorm
        # semantics): the gradient engine averages them like any other
        # gradient
        local = bsums.clone()
        ctx.comm.all_reduce_(bsums, op="sum", async_op=False)
        if ctx.use_ext:
            outs = ext.fused_bn_sync_bwd_dx(
                dy, mask, x, mean, invstd, weight, bsums, count,
                ctx.relu, has_res)
            dx = outs[0]
            dres = outs[1] if has_res else None
        else:
            dx, d = _twin_bwd_dx(dy, mask, x, mean, invstd, weight,
                                 bsums, count, ctx.relu)
            dres = d.to(ctx.res_dtype) if has_res else None
        dgamma = dbeta = None
        if weight is not None:
            dbeta = local[:c].to(weight.dtype)
            dgamma = local[c:].to(weight.dtype)
        return (dx, dres, dgamma, dbeta, None, None, None, None, None,
                None, None)


class FusedSyncBatchNorm2d(FusedBatchNorm2d):
    """``FusedBatchNorm2d`` whose training-mode statistics span all ranks
    of ``comm`` (an ``engine.comm.Communicator``).

    Same parameters, buffers and ``state_dict`` keys; ``comm`` is not
    state and is dropped on pickling and copying. In eval mode, with
    ``comm is None`` or with one rank, this is ``FusedBatchNorm2d``
    exactly. Otherwise every training-mode forward, also under
    ``torch.no_grad()`` or ``NativeDDP.no_sync()``, all-reduces the
    per-channel sums and the row count, so ranks may hold different
    batch sizes but must run the same number of training forwards.
    ``forward_pool`` and ``forward_dual`` then take their composed
    forms and synchronise through ``forward``."""

    def __init__(self, num_features: int, relu: bool = False, comm=None,
                 **kwargs):
        super().__init__(num_features, relu=relu, **kwargs)
        self.comm = comm

    def __getstate__(self):
        state = self.__dict__.copy()
        state["comm"] = None  # live process-group handles do not travel
        return state

    def _sync_active(self) -> bool:
        return self.training and self.comm is not None and \
            self.comm.world_size > 1

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not self._sync_active():
            return super().forward(x, residual)
        self._check_input_dim(x)
        use_ext = self._kernel_ready(x) and \
            self.bias is not None and \
            (residual is None or (residual.dtype == x.dtype and
                                  residual.shape == x.shape)) and \
            (self.running_mean is None or
             self.running_mean.dtype == torch.float32)
        if use_ext and residual is not None:
            residual = residual.contiguous(
                memory_format=torch.channels_last)
        return _FusedSyncBNFunction.apply(
            x, residual, self.weight, self.bias, self.running_mean,
            self.running_var, self._step_momentum(), self.eps, self.relu,
            self.comm, use_ext)


def convert_sync_batchnorm(module: nn.Module, comm) -> nn.Module:
    """Replace every ``nn.BatchNorm2d`` in ``module`` (``FusedBatchNorm2d``
    included, keeping its ``relu`` flag) with a ``FusedSyncBatchNorm2d``
    bound to ``comm``. The replacement carries the same Parameter and
    buffer objects, so optimizers built earlier stay valid. A module
    that already is a ``FusedSyncBatchNorm2d`` is kept and rebound to
    ``comm``. ``BatchNorm1d``/``BatchNorm3d`` are left alone, with one
    warning that names them. Returns the converted module (a new object
    only when ``module`` itself is a BatchNorm2d)."""
    skipped: list = []
    out = _convert_sync(module, comm, "", {}, skipped)
    if skipped:
        import warnings
        warnings.warn(
            "convert_sync_batchnorm only synchronises BatchNorm2d; left "
            "with per-rank statistics: " + ", ".join(skipped))
    return out


def _convert_sync(module, comm, name, memo, skipped):
    if id(module) in memo:
        return memo[id(module)]
    out = module
    if isinstance(module, FusedSyncBatchNorm2d):
        module.comm = comm
    elif isinstance(module, nn.BatchNorm2d):
        out = FusedSyncBatchNorm2d(
            module.num_features, relu=getattr(module, "relu", False),
            comm=comm, eps=module.eps, momentum=module.momentum,
            affine=module.affine,
            track_running_stats=module.track_running_stats)
        if module.affine:
            out.weight = module.weight
            out.bias = module.bias
        if module.track_running_stats:
            out.running_mean = module.running_mean
            out.running_var = module.running_var
            out.num_batches_tracked = module.num_batches_tracked
        out.training = module.training
    elif isinstance(module, (nn.BatchNorm1d, nn.BatchNorm3d)):
        skipped.append(f"{name or '<root>'} ({type(module).__name__})")
    memo[id(module)] = out
    for child_name, child in module.named_children():
        new = _convert_sync(child, comm,
                            f"{name}.{child_name}" if name else child_name,
                            memo, skipped)
        if new is not child:
            module.add_module(child_name, new)
    return out
