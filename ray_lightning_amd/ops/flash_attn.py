"""Hand-written CDNA4 MFMA flash attention (causal, hs=64, bf16).

``flash_attention(q, k, v)`` is SDPA-shaped: [B, H, T, hs] in/out.
The custom v3 kernels (swapped-operand S^T, in-register permlane
redistribution, ds_read_b64_tr_b16 transposed fragments — see
flash_attn.hip) engage for causal bf16 hs=64 T%64==0 on GPU, with
``k`` and ``v`` of ``q``'s shape, dtype and device, and are the
DEFAULT: measured 0.421 ms fwd+bwd vs AOTriton SDPA's 0.710 ms on
the GPT-2-XL shape (B=8, H=25, T=1024) — 41% faster, winning both
directions (fwd -12%, bwd -47%); profiles/r02_flash_v3.md.
Anything else falls back to ``F.scaled_dot_product_attention``.

Attention dropout (``dropout_p > 0``) runs inside the same kernels
(their DROPOUT instantiations): the keep mask over the [B, H, T, T]
probabilities is a counter-based Philox function of the (seed, offset)
the forward draws from the device's default generator, regenerated in
backward, so nothing of size T x T is ever stored (docs/DESIGN.md §8,
profiles/flash_attn_dropout.md). Whether that path is taken by default
is ``_DROPOUT_DEFAULT`` below; ``RLA_FLASH_DROPOUT=1`` / ``=0`` forces
it on / off (off: SDPA does the dropout).

``RLA_FLASH=0`` disables the custom path; ``RLA_FLASH_SHFL=1`` selects
the ds_bpermute redistribution variant (debug), for the dropout kernels
too.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from . import _load_ext

# Set by the measurement in profiles/flash_attn_dropout.md: the dropout
# kernels are the default iff they beat SDPA-with-dropout there.
_DROPOUT_DEFAULT = True


def _usable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    if os.environ.get("RLA_FLASH", "1") == "0":
        return False
    # the kernels index k and v with q's extents
    for t in (k, v):
        if (t.shape != q.shape or t.dtype != q.dtype
                or t.device != q.device):
            return False
    return (q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 4
            and q.shape[-1] == 64 and q.shape[2] % 64 == 0
            and _load_ext() is not None
            and hasattr(_load_ext(), "flash_attn_fwd_v3"))


def _use_permlane() -> bool:
    return os.environ.get("RLA_FLASH_SHFL", "0") != "1"


def _dropout_kernels_enabled() -> bool:
    env = os.environ.get("RLA_FLASH_DROPOUT")
    if env is None:
        return _DROPOUT_DEFAULT
    return env == "1"


def _check_p(p: float) -> None:
    if not 0.0 <= p < 1.0:
        raise ValueError(
            f"dropout probability has to be in [0, 1), but got {p}")


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        ext = _load_ext()
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, _use_permlane())
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        ext = _load_ext()
        dq, dk, dv = ext.flash_attn_bwd_v3(dout, q, k, v, o, lse,
                                           ctx.scale, _use_permlane())
        return dq, dk, dv, None


class _FlashAttnDropout(torch.autograd.Function):
    """``dropout(softmax(q k^T * scale), p) @ v`` on the DROPOUT
    instantiations of the v3 kernels. Saves what ``_FlashAttn`` saves
    (``lse`` is that of the undropped softmax); the mask lives on as
    ``(p, seed, offset)``, three Python numbers on ctx."""

    @staticmethod
    def forward(ctx, q, k, v, scale, p):
        ext = _load_ext()
        o, lse, seed, offset = ext.flash_attn_fwd_v3_dropout(
            q, k, v, scale, p, _use_permlane())
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        ext = _load_ext()
        dq, dk, dv = ext.flash_attn_bwd_v3_dropout(
            dout, q, k, v, o, lse, ctx.scale, ctx.p, ctx.seed,
            ctx.offset, _use_permlane())
        return dq, dk, dv, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    dropout_p: float = 0.0) -> torch.Tensor:
    """Causal attention; custom MFMA kernels when usable, SDPA
    otherwise.

    ``dropout_p > 0`` drops attention probabilities (and scales the kept
    ones by ``1/(1-p)``): inside the custom kernels when the call is
    usable and the dropout kernels are enabled (module docstring), else
    through ``F.scaled_dot_product_attention``. Raises ``ValueError``
    for ``dropout_p`` outside ``[0, 1)``."""
    _check_p(dropout_p)
    usable = _usable(q, k, v)
    if dropout_p > 0.0:
        if usable and _dropout_kernels_enabled():
            if not hasattr(_load_ext(), "flash_attn_fwd_v3_dropout"):
                raise RuntimeError(
                    "_hip_ops has no flash_attn_fwd_v3_dropout: rebuild "
                    "with `python -m ray_lightning_amd.ops.build`")
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            scale = 1.0 / math.sqrt(q.shape[-1])
            return _FlashAttnDropout.apply(q, k, v, scale,
                                           float(dropout_p))
        return F.scaled_dot_product_attention(
            q, k, v, dropout_p=dropout_p, is_causal=True)
    if usable:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        scale = 1.0 / math.sqrt(q.shape[-1])
        return _FlashAttn.apply(q, k, v, scale)
    return F.scaled_dot_product_attention(q, k, v, is_causal=True)
