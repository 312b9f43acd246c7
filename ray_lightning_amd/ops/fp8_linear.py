"""Linear layers over fp8 weights at any row count.

``fp8_linear(x, weight_fp8, weight_scale, bias, gelu=)`` computes ``y =
act(x @ dequant(W).T + bias)`` for ``x`` [..., K], ``weight_fp8`` [N, K]
float8_e4m3fn and ``weight_scale`` [N] fp32 powers of two, the pair that
``quantize_weight`` (ops/skinny_linear.py) makes; ``act`` is the identity
or, with ``gelu=True``, tanh-GELU. The accumulation and GELU are fp32 and
``y`` is rounded once, after bias and GELU: ``skinny_linear``'s rounding
points. ``q * scale`` is exact in bf16, so this is ``F.linear`` on the
dequantized weight with another summation order and one rounding where
the composed path has two (three with GELU).

It is what lets a model do without the bf16 copy of a quantized matrix
(``GPT2.quantize_weights_fp8(drop_bf16=True)``): prefill, ``extend`` and
every decode step read the codes.

On the GPU, for bf16 ``x`` and ``K`` in 32s: up to ``MAX_SKINNY_ROWS`` rows
run the skinny fp8 weight stream (csrc/skinny_linear.hip), called directly,
whatever ``RLA_SKINNY_LINEAR`` says (that gates the bf16 model's route);
more rows run the tiled LDS MFMA GEMM of csrc/fp8_linear.hip (docs/DESIGN.md
§22, profiles/fp8_linear.md). Everything else (CPU, other dtypes, other
``K``, ``RLA_FP8_LINEAR=0``) runs the torch twin with the same rounding
points.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from .skinny_linear import FP8, _ext_with, dequantize_weight

# The largest M in {8, 16, 32, 64} at which the skinny fp8 kernel is not
# slower than the tiled one on GPT-2-XL's four layer shapes, 0 if none
# (profiles/fp8_linear.md: at M = 64 it takes 9 to 28 us where the tiled one
# takes 15 to 51). At most 64, the skinny kernel's limit.
MAX_SKINNY_ROWS = 64


def kernel_enabled() -> bool:
    """The gate: on unless ``RLA_FP8_LINEAR=0``."""
    return os.environ.get("RLA_FP8_LINEAR") != "0"


def _twin(x, weight_fp8, weight_scale, bias, gelu):
    dt = x.dtype
    wide = torch.promote_types(dt, torch.float32)
    y = x.to(wide) @ dequantize_weight(weight_fp8, weight_scale, wide).t()
    if bias is not None:
        y = y + bias.to(wide)
    if gelu:
        y = F.gelu(y, approximate="tanh")
    return y.to(dt)


def fp8_linear(x: torch.Tensor, weight_fp8: torch.Tensor,
               weight_scale: torch.Tensor,
               bias: Optional[torch.Tensor] = None, *,
               gelu: bool = False) -> torch.Tensor:
    """``act(x @ dequant(weight_fp8, weight_scale).T + bias)`` (module
    docstring) for ``x`` [..., K]; returns [..., N] in ``x``'s dtype."""
    if weight_fp8.dtype != FP8 or weight_fp8.dim() != 2:
        raise ValueError(
            f"weight_fp8 must be float8_e4m3fn [N, K], got "
            f"{weight_fp8.dtype} {list(weight_fp8.shape)}")
    N, K = weight_fp8.shape
    if N < 1:
        raise ValueError("weight_fp8 has no rows")
    if weight_scale.dtype != torch.float32 or \
            tuple(weight_scale.shape) != (N,):
        raise ValueError(f"weight_scale must be fp32 [N] = [{N}]")
    if x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(
            f"x must be [..., K = {K}], got {list(x.shape)}")
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError(
            f"bias must be [N] = [{N}], got {list(bias.shape)}")
    x2 = x.reshape(-1, K)
    if (x.is_cuda and x.dtype == torch.bfloat16 and K % 32 == 0
            and kernel_enabled()):
        # the checked host paths: every other operand check is there
        x2 = x2.contiguous()
        if x2.shape[0] <= MAX_SKINNY_ROWS:
            y, _ = _ext_with("skinny_linear_fwd").skinny_linear_fwd(
                x2, weight_fp8, bias, None, None, None, 0.0, bool(gelu),
                weight_scale)
        else:
            y = _ext_with("fp8_linear_fwd").fp8_linear_fwd(
                x2, weight_fp8, weight_scale, bias, bool(gelu))
    else:
        y = _twin(x2, weight_fp8, weight_scale, bias, gelu)
    return y.view(*x.shape[:-1], N)
