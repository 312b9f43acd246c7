"""1x1 stride-1 convolution whose input has a second consumer.

At a ResNet bottleneck junction the block input ``x`` feeds ``conv1`` and
the identity (or the downsample conv), so autograd adds two gradients of
block-input size: MIOpen zero-fills ``dx``, runs its backward-data kernel
into it, and an elementwise add reads it back together with the skip
gradient. ``conv1x1_fork`` returns ``(conv(x, w), x_skip)`` with
``x_skip`` an alias of ``x``; its backward hands both gradients to one
HIP kernel (``csrc/conv1x1_bwd.hip``) that writes
``dx = bf16(fp32(dy . w) + fp32(g_skip))`` once.

Forward is the ATen convolution as before; ``dw`` is MIOpen's
``convolution_backward`` as before. Where the kernel does not apply (CPU,
fp32, not channels_last, other channel counts, extension not built) or
``RLA_CONV1X1_BWD=0``, ``dx`` is the composed math:
``convolution_backward`` plus ``g_skip``.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import _load_ext

# conv1 output widths (Cout) whose junctions models wire to the kernel:
# those where the kernel trace shows it below what it replaces
# (profiles/conv1x1_bwd_data.md)
WIRED_WIDTHS = (64, 128, 256)


def conv1x1_bwd_enabled() -> bool:
    """``RLA_CONV1X1_BWD=0`` keeps the junctions on the composed path.
    Models read it once, at construction."""
    return os.environ.get("RLA_CONV1X1_BWD", "1") != "0"


def _cl_bf16(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dim() == 4 and t.dtype == torch.bfloat16 and \
        t.is_contiguous(memory_format=torch.channels_last)


def conv1x1_bwd_supported(dy: torch.Tensor, w: torch.Tensor,
                          skip: Optional[torch.Tensor] = None) -> bool:
    """Whether ``conv1x1_bwd_data(dy, w, skip)`` has a kernel: bf16
    channels_last ``dy [N,Cout,H,W]`` (and ``skip [N,Cin,H,W]``) on the
    GPU, bf16 contiguous ``w [Cout,Cin,1,1]``, a supported channel pair,
    and the extension built."""
    if not _cl_bf16(dy):
        return False
    if not (w.is_cuda and w.dim() == 4 and w.dtype == torch.bfloat16 and
            w.device == dy.device and w.is_contiguous() and
            w.shape[0] == dy.shape[1] and tuple(w.shape[2:]) == (1, 1)):
        return False
    if skip is not None and not (
            _cl_bf16(skip) and skip.device == dy.device and
            tuple(skip.shape) == (dy.shape[0], w.shape[1], dy.shape[2],
                                  dy.shape[3])):
        return False
    ext = _load_ext()
    return ext is not None and \
        ext.conv1x1_bwd_data_supported(w.shape[0], w.shape[1])


def conv1x1_bwd_data(dy: torch.Tensor, w: torch.Tensor,
                     skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dx = bf16(fp32(dy . w) + fp32(skip))``, one rounding. Raises
    where ``conv1x1_bwd_supported`` is false."""
    if not conv1x1_bwd_supported(dy, w, skip):
        raise RuntimeError(
            "conv1x1_bwd_data: unsupported arguments (need bf16 "
            "channels_last GPU tensors, supported channels and the built "
            "HIP extension)")
    return _load_ext().conv1x1_bwd_data(dy, w, skip)


_CONV_ARGS = ([1, 1], [0, 0], [1, 1], False, [0, 0], 1)


class _Conv1x1ForkFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, fused):
        # an unused output's gradient arrives as None, not as zeros
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, weight)
        ctx.fused = fused
        return F.conv2d(x, weight), x.view_as(x)

    @staticmethod
    def backward(ctx, g_out, g_skip):
        x, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_out is None:  # only the skip output was used
            return (g_skip if need_dx else None), None, None
        fused = need_dx and ctx.fused and \
            conv1x1_bwd_supported(g_out, weight, g_skip)
        mask = [need_dx and not fused, need_dw, False]
        dx = dw = None
        if any(mask):
            dx, dw, _ = torch.ops.aten.convolution_backward(
                g_out, x, weight, None, *_CONV_ARGS, mask)
        if fused:
            dx = _load_ext().conv1x1_bwd_data(g_out, weight, g_skip)
        elif need_dx and g_skip is not None:
            dx = dx + g_skip
        return dx, dw, None


def conv1x1_fork(x: torch.Tensor, weight: torch.Tensor,
                 fused: Optional[bool] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(conv2d(x, weight), x_skip)`` for a 1x1 stride-1 unpadded
    convolution without bias. ``x_skip`` aliases ``x`` and is what the
    second consumer of ``x`` reads, so both gradients meet in this
    function's backward. ``fused=None`` reads ``RLA_CONV1X1_BWD``."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise ValueError("conv1x1_fork needs a [Cout, Cin, 1, 1] weight")
    if fused is None:
        fused = conv1x1_bwd_enabled()
    # the autocast cast stays outside the Function, so that autograd
    # casts dw back to the parameter's dtype as for nn.Conv2d
    dev = x.device.type
    if torch.is_autocast_enabled(dev):
        dtype = torch.get_autocast_dtype(dev)
        x, weight = x.to(dtype), weight.to(dtype)
    return _Conv1x1ForkFunction.apply(x, weight, fused)
