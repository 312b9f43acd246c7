"""Linear layers of a decode step: at most 64 rows against a weight matrix.

``skinny_linear(x, weight, bias, residual=, ln_weight=, ln_bias=, eps=,
gelu=)`` computes ``y = act(h @ weight.T + bias)`` for ``x`` [M, K] and
``weight`` [N, K] as ``nn.Linear`` stores it, where ``h`` is

- ``x`` itself,
- ``LN(x)`` when ``ln_weight`` / ``ln_bias`` are given, or
- ``LN(x_new)`` with ``x_new = x + residual`` when ``residual`` is given
  too (then the call returns ``(y, x_new)``: ``x_new`` is the residual
  stream of a pre-norm block),

and ``act`` is the identity or, with ``gelu=True``, tanh-GELU. Rounding
points, in the operands' dtype: ``x_new``, ``h``, and ``y`` once after
bias and GELU; LayerNorm statistics, the accumulation and GELU are fp32.

``decode_layer(...)`` is one GPT-2 block of a decode step built from it:
[add + LN1 + c_attn], ``decode_attention`` over the KV cache (with the
append; bf16 or, with ``k_scale`` / ``v_scale``, fp8), [c_proj], [add + LN2 + c_fc + GELU], [c_proj].

On the GPU, for bf16 with ``M <= 64``, ``K % 32 == 0`` and fp32 LayerNorm
parameters, both are the HIP code of csrc/skinny_linear.hip: an MFMA
kernel that streams the weights once, with the pointwise neighbours in
its prologue and epilogue, and for ``decode_layer`` one host call that
enqueues the block's six kernels (docs/DESIGN.md §18,
profiles/skinny_linear.md). With ``RLA_DECODE_ATTN=0`` the block is
composed here instead, from the linear kernels and ``decode_attention``'s
twin. Whether that is the default is
``_SKINNY_DEFAULT`` below; ``RLA_SKINNY_LINEAR=1`` / ``=0`` forces it on
/ off. Everything else (CPU, other dtypes, more rows, other ``K``, the
gate off) runs the torch twin with the same semantics.

fp8 weights. ``quantize_weight(weight)`` gives ``(q, scale)``: OCP
``float8_e4m3fn`` codes [N, K] and one fp32 power-of-two scale per row,
``scale[n] = 2^ceil(log2(absmax[n] / 448))``. ``skinny_linear(x, q, ...,
weight_scale=scale)`` then streams the bytes and converts them to bf16 in
registers (the fp8 kernels of csrc/skinny_linear.hip, docs/DESIGN.md §19,
profiles/skinny_linear_fp8.md). ``q * scale`` is exact in bf16, so the
same function is ``skinny_linear`` on the dequantized bf16 weight, which
is what the twin computes. ``decode_layer`` takes the fp8 kernels when its
four ``nn.Linear`` modules carry ``weight_fp8`` / ``weight_scale`` buffers
(``GPT2.quantize_weights_fp8``) and ``RLA_SKINNY_FP8`` allows it
(``_FP8_DEFAULT`` below when unset, ``1`` / ``0`` forces it).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _load_ext
from .decode_attn import _kernel_enabled as _attn_kernel_enabled
from .decode_attn import decode_attention

# Off although the measurement in profiles/skinny_linear.md meets the rule
# set for it (GPT-2-XL's decode step faster at both B = 8 and B = 1 by more
# than the runs' spread): the one-call-per-block path reaches decode
# attention from C++, past the Python entry at which the generation tests
# count its calls, and M = 64 loses per call. The profile has both.
_SKINNY_DEFAULT = False

# Once a model is quantized, the fp8 kernels are the route: by the rule set
# before the run, GPT-2-XL's decode step is faster with them than with the
# bf16 kernels at both B = 8 and B = 1 by more than the runs' spread
# (profiles/skinny_linear_fp8.md).
_FP8_DEFAULT = True

MAX_ROWS = 64
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def kernel_enabled() -> bool:
    """The gate: ``RLA_SKINNY_LINEAR`` when set, else the default."""
    env = os.environ.get("RLA_SKINNY_LINEAR")
    if env is None:
        return _SKINNY_DEFAULT
    return env == "1"


def fp8_enabled() -> bool:
    """Whether quantized linears run the fp8 kernels: ``RLA_SKINNY_FP8``
    when set, else the default."""
    env = os.environ.get("RLA_SKINNY_FP8")
    if env is None:
        return _FP8_DEFAULT
    return env != "0"


def quantize_weight(weight: torch.Tensor):
    """``(q, scale)`` for ``weight`` [N, K]: ``q`` float8_e4m3fn [N, K] and
    ``scale`` fp32 [N], the smallest power of two with
    ``absmax[n] / scale[n] <= 448`` (1 for an all-zero row).
    ``q.float() * scale[:, None]`` is exact in bf16, and quantizing it
    again gives the same values."""
    if weight.dim() != 2:
        raise ValueError(f"weight must be [N, K], got {list(weight.shape)}")
    w = weight.detach().float()
    # frexp: absmax / 448 = m * 2^e with m in [0.5, 1), so ceil(log2) is e,
    # or e - 1 at m = 0.5; exact, where log2 would round
    m, e = torch.frexp(w.abs().amax(dim=1) / FP8_MAX)
    e = torch.where(m == 0.5, e - 1, e)
    scale = torch.where(m == 0, torch.ones_like(m),
                        torch.ldexp(torch.ones_like(m), e))
    return (w / scale[:, None]).to(FP8), scale


def dequantize_weight(q: torch.Tensor, scale: torch.Tensor,
                      dtype=torch.bfloat16) -> torch.Tensor:
    """``q * scale`` per row in ``dtype`` (exact in bf16 and wider)."""
    return (q.float() * scale[:, None]).to(dtype)


def kernel_serves(weight, ln_weight=None) -> bool:
    """Whether the kernel takes this ``weight`` [N, K], bf16 or fp8, (and
    LayerNorm parameter) for up to ``MAX_ROWS`` bf16 rows; the gate is
    apart."""
    return (weight.is_cuda and weight.dtype in (torch.bfloat16, FP8)
            and weight.dim() == 2 and weight.shape[1] % 32 == 0
            and weight.shape[1] >= 32
            and (ln_weight is None or ln_weight.dtype == torch.float32)
            and _load_ext() is not None)


def _kernel_shape(x, weight, ln_weight) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[0] <= MAX_ROWS and kernel_serves(weight, ln_weight))


def _ext_with(symbol: str):
    ext = _load_ext()
    if not hasattr(ext, symbol):
        raise RuntimeError(
            f"_hip_ops has no {symbol}: rebuild with "
            "`python -m ray_lightning_amd.ops.build`")
    return ext


def _twin(x, weight, bias, residual, ln_weight, ln_bias, eps, gelu):
    dt = x.dtype
    wide = torch.promote_types(dt, torch.float32)
    x_new = None
    if residual is not None:
        x_new = (x.to(wide) + residual.to(wide)).to(dt)
        x = x_new
    if ln_weight is not None:
        x = F.layer_norm(x.to(wide), (x.shape[-1],), ln_weight.to(wide),
                         ln_bias.to(wide), eps).to(dt)
    y = x.to(wide) @ weight.to(wide).t()
    if bias is not None:
        y = y + bias.to(wide)
    if gelu:
        y = F.gelu(y, approximate="tanh")
    return y.to(dt), x_new


def _check(x, weight, bias, residual, ln_weight, ln_bias,
           weight_scale=None):
    if (weight.dtype == FP8) != (weight_scale is not None):
        raise ValueError(
            "a float8_e4m3fn weight and weight_scale come together or not "
            "at all")
    if weight_scale is not None and (
            tuple(weight_scale.shape) != (weight.shape[0],)
            or weight_scale.dtype != torch.float32):
        raise ValueError(
            f"weight_scale must be fp32 [N] = [{weight.shape[0]}]")
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(
            f"x must be [M, K] and weight [N, K], got {list(x.shape)} and "
            f"{list(weight.shape)}")
    if weight.shape[0] < 1:
        raise ValueError("weight has no rows")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(
            f"bias must be [N] = [{weight.shape[0]}], got "
            f"{list(bias.shape)}")
    if (ln_weight is None) != (ln_bias is None):
        raise ValueError("ln_weight and ln_bias come together or not at all")
    if ln_weight is not None:
        for p in (ln_weight, ln_bias):
            if tuple(p.shape) != (x.shape[1],):
                raise ValueError(
                    f"ln_weight and ln_bias must be [K] = [{x.shape[1]}]")
    if residual is not None:
        if ln_weight is None:
            raise ValueError(
                "a residual is only taken together with LayerNorm")
        if residual.shape != x.shape or residual.dtype != x.dtype:
            raise ValueError("residual must have x's shape and dtype")


def skinny_linear(x: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor] = None, *,
                  residual: Optional[torch.Tensor] = None,
                  ln_weight: Optional[torch.Tensor] = None,
                  ln_bias: Optional[torch.Tensor] = None,
                  eps: float = 1e-5, gelu: bool = False,
                  weight_scale: Optional[torch.Tensor] = None):
    """``act(LN(x + residual) @ weight.T + bias)`` (module docstring);
    ``weight`` is float8_e4m3fn when ``weight_scale`` [N] is given.
    Returns ``y`` [M, N], or ``(y, x_new)`` when ``residual`` is given."""
    _check(x, weight, bias, residual, ln_weight, ln_bias, weight_scale)
    if _kernel_shape(x, weight, ln_weight) and kernel_enabled():
        # the one checked host path: every other operand check is there
        y, x_new = _ext_with("skinny_linear_fwd").skinny_linear_fwd(
            x, weight, bias, residual, ln_weight, ln_bias, float(eps),
            bool(gelu), weight_scale)
    else:
        if weight_scale is not None:
            weight = dequantize_weight(weight, weight_scale, x.dtype)
        y, x_new = _twin(x, weight, bias, residual, ln_weight, ln_bias, eps,
                         gelu)
    return y if residual is None else (y, x_new)


def decode_layer(x: torch.Tensor, residual: Optional[torch.Tensor],
                 ln1, c_attn, k_cache: torch.Tensor, v_cache: torch.Tensor,
                 pos: torch.Tensor, max_pos: int, attn_proj, ln2, c_fc,
                 mlp_proj, k_scale: Optional[torch.Tensor] = None,
                 v_scale: Optional[torch.Tensor] = None):
    """One pre-norm GPT-2 block of a decode step. ``x`` [B, C] is the
    previous block's MLP output and ``residual`` the stream it is added
    to; for the first block ``x`` is the stream and ``residual`` is
    ``None``. ``ln1`` / ``ln2`` are the block's LayerNorm modules and
    ``c_attn`` / ``attn_proj`` / ``c_fc`` / ``mlp_proj`` its ``nn.Linear``
    modules; the caches [B, H, Tmax, hs], ``pos`` and ``max_pos`` are
    ``decode_attention``'s, ``k_scale`` / ``v_scale`` [B, H, Tmax] included
    when the caches are float8_e4m3fn (ops/decode_attn.py). Returns ``(x_mid, mlp_out)``: the stream after
    the attention sublayer and the MLP's output, which the next block (or
    the final LayerNorm) takes as ``(residual, x)``."""
    B, C = x.shape
    hs = k_cache.shape[-1]
    if ln1.eps != ln2.eps:
        raise ValueError("ln1 and ln2 differ in eps")
    linears = (c_attn, attn_proj, c_fc, mlp_proj)
    # (weight, scale) per linear: the fp8 pair where all four carry one
    # and RLA_SKINNY_FP8 allows it, else the bf16 weight, which holds the
    # same values
    if fp8_enabled() and all(
            getattr(m, "weight_fp8", None) is not None for m in linears):
        ws = [(m.weight_fp8, m.weight_scale) for m in linears]
    elif any(m.weight.numel() == 0 for m in linears):
        # GPT2.quantize_weights_fp8(drop_bf16=True) left the fp8 pair only
        raise RuntimeError(
            "decode_layer: the bf16 weights were dropped and RLA_SKINNY_FP8=0 "
            "keeps the fp8 kernels off; apply the linears with fp8_linear")
    else:
        ws = [(m.weight, None) for m in linears]
    (aw, as_), (pw, ps), (fw, fs), (mw, ms) = ws
    # the one call reaches decode attention's kernel from C++, so that
    # kernel's own gate (RLA_DECODE_ATTN) has to be on as well. The shapes
    # are read from the matrices chosen above: a dropped weight is empty.
    if (_kernel_shape(x, aw, ln1.weight) and kernel_enabled()
            and _attn_kernel_enabled()
            and hs == 64 and k_cache.dtype == (
                torch.bfloat16 if k_scale is None else FP8)
            and fw.shape[0] % 32 == 0
            and ln2.weight.dtype == torch.float32
            and all(m.bias is not None for m in linears)):
        if as_ is not None:
            return _ext_with("decode_layer_fp8_fwd").decode_layer_fp8_fwd(
                x, residual, ln1.weight, ln1.bias, aw, as_, c_attn.bias,
                k_cache, v_cache, pos, int(max_pos), 1.0 / math.sqrt(hs),
                pw, ps, attn_proj.bias, ln2.weight, ln2.bias, fw, fs,
                c_fc.bias, mw, ms, mlp_proj.bias, float(ln1.eps), k_scale,
                v_scale)
        return _ext_with("decode_layer_fwd").decode_layer_fwd(
            x, residual, ln1.weight, ln1.bias, c_attn.weight, c_attn.bias,
            k_cache, v_cache, pos, int(max_pos), 1.0 / math.sqrt(hs),
            attn_proj.weight, attn_proj.bias, ln2.weight, ln2.bias,
            c_fc.weight, c_fc.bias, mlp_proj.weight, mlp_proj.bias,
            float(ln1.eps), k_scale, v_scale)
    ln = dict(ln_weight=ln1.weight, ln_bias=ln1.bias, eps=ln1.eps,
              weight_scale=as_)
    if residual is None:
        qkv, x1 = skinny_linear(x, aw, c_attn.bias, **ln), x
    else:
        qkv, x1 = skinny_linear(x, aw, c_attn.bias, residual=residual, **ln)
    att = decode_attention(qkv, k_cache, v_cache, pos, max_pos,
                           k_scale=k_scale, v_scale=v_scale)
    att = skinny_linear(att, pw, attn_proj.bias, weight_scale=ps)
    hid, x_mid = skinny_linear(att, fw, c_fc.bias, residual=x1,
                               ln_weight=ln2.weight, ln_bias=ln2.bias,
                               eps=ln2.eps, gelu=True, weight_scale=fs)
    return x_mid, skinny_linear(hid, mw, mlp_proj.bias, weight_scale=ms)
