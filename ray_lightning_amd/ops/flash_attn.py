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

Packed rows (``doc_ids``): ``flash_attention(q, k, v, doc_ids=ids)``
with integer ``ids`` of shape [B, T] is causal attention WITHIN each
document of a packed row. A document begins at position 0 and wherever
``ids[b, t] != ids[b, t-1]`` (an id that comes back later starts a new
document); query ``q`` attends key ``kv`` iff ``doc_start[b, q] <= kv
<= q``. ``doc_bounds(ids)`` derives the int32 ``(doc_start, doc_end)``
pair; a model computes it once per batch and passes the pair in place
of the ids. The DOCS instantiations of the v3 kernels take the bounds,
start (forward, dq) or end (dkv) their tile loop at the document's
first or last tile and skip, per wave, tiles wholly in another document
(docs/DESIGN.md §10, profiles/flash_attn_docs.md); dropout composes
with it, on the same mask bits. They engage under the conditions above;
whether by default is ``_DOCS_DEFAULT`` below, and ``RLA_FLASH_DOCS=1``
/ ``=0`` forces them on / off. Otherwise (CPU included) the call goes
through SDPA with the boolean [B, 1, T, T] mask built from the bounds.

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

# Set by the measurement in profiles/flash_attn_docs.md: the DOCS
# kernels are the default iff they beat SDPA with the boolean mask there.
_DOCS_DEFAULT = True


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


def _docs_kernels_enabled() -> bool:
    env = os.environ.get("RLA_FLASH_DOCS")
    if env is None:
        return _DOCS_DEFAULT
    return env == "1"


def doc_bounds(doc_ids: torch.Tensor):
    """``(doc_start, doc_end)``, int32 [B, T], from integer ``doc_ids``
    [B, T]: the first and the last position of the document that holds
    each position. A document begins at 0 and wherever the id differs
    from the one before it; the values carry no other meaning."""
    if not isinstance(doc_ids, torch.Tensor) or doc_ids.dim() != 2:
        raise ValueError("doc_ids must be a [B, T] tensor")
    if doc_ids.is_floating_point() or doc_ids.is_complex():
        raise ValueError(
            f"doc_ids must be an integer tensor, got {doc_ids.dtype}")
    B, T = doc_ids.shape
    pos = torch.arange(T, device=doc_ids.device, dtype=torch.int32)
    first = torch.ones(B, T, dtype=torch.bool, device=doc_ids.device)
    first[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    last = torch.ones_like(first)
    last[:, :-1] = first[:, 1:]
    zero = torch.zeros((), dtype=torch.int32, device=doc_ids.device)
    # running maximum of the boundary positions seen so far ...
    start = torch.cummax(torch.where(first, pos, zero), dim=1).values
    # ... and its mirror image from the right
    rev = torch.where(last, T - 1 - pos, zero).flip(1)
    end = T - 1 - torch.cummax(rev, dim=1).values.flip(1)
    return start.to(torch.int32).contiguous(), \
        end.to(torch.int32).contiguous()


def _as_bounds(doc_ids, q: torch.Tensor):
    """The ``(doc_start, doc_end)`` pair of a ``doc_ids`` argument: ids
    [B, T], or the precomputed pair."""
    if isinstance(doc_ids, (tuple, list)):
        if len(doc_ids) != 2:
            raise ValueError("doc_ids: expected ids or (doc_start, doc_end)")
        start, end = doc_ids
        for t in (start, end):
            if not isinstance(t, torch.Tensor) or t.is_floating_point():
                raise ValueError("doc_ids: bounds must be integer tensors")
    else:
        start, end = doc_bounds(doc_ids)
    want = (q.shape[0], q.shape[2])
    for t in (start, end):
        if t.dim() != 2 or tuple(t.shape) != want:
            raise ValueError(
                f"doc_ids must have shape [B, T] = {list(want)}, got "
                f"{list(t.shape)}")
    return (start.to(device=q.device, dtype=torch.int32).contiguous(),
            end.to(device=q.device, dtype=torch.int32).contiguous())


def doc_mask(doc_start: torch.Tensor) -> torch.Tensor:
    """Boolean [B, 1, T, T] mask of the allowed (q, kv) pairs: what the
    SDPA fallback materialises and the kernels never do."""
    T = doc_start.shape[1]
    pos = torch.arange(T, device=doc_start.device)
    allowed = (pos[None, None, :] <= pos[None, :, None]) & \
        (pos[None, None, :] >= doc_start[:, :, None])
    return allowed[:, None]


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


class _FlashAttnDocs(torch.autograd.Function):
    """Document-masked causal attention on the DOCS instantiations of
    the v3 kernels, with dropout when ``p > 0``. Saves what
    ``_FlashAttn`` saves plus the two [B, T] int32 bounds; nothing of
    size T x T."""

    @staticmethod
    def forward(ctx, q, k, v, doc_start, doc_end, scale, p):
        ext = _load_ext()
        if p > 0.0:
            o, lse, seed, offset = ext.flash_attn_fwd_v3_docs_dropout(
                q, k, v, doc_start, scale, p, _use_permlane())
            ctx.seed, ctx.offset = seed, offset
        else:
            o, lse = ext.flash_attn_fwd_v3_docs(q, k, v, doc_start, scale,
                                                _use_permlane())
        ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
        ctx.scale, ctx.p = scale, p
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, doc_start, doc_end = ctx.saved_tensors
        ext = _load_ext()
        if ctx.p > 0.0:
            dq, dk, dv = ext.flash_attn_bwd_v3_docs_dropout(
                dout, q, k, v, o, lse, doc_start, doc_end, ctx.scale,
                ctx.p, ctx.seed, ctx.offset, _use_permlane())
        else:
            dq, dk, dv = ext.flash_attn_bwd_v3_docs(
                dout, q, k, v, o, lse, doc_start, doc_end, ctx.scale,
                _use_permlane())
        return dq, dk, dv, None, None, None, None


def _docs_attention(q, k, v, dropout_p, doc_ids):
    doc_start, doc_end = _as_bounds(doc_ids, q)
    if (_usable(q, k, v) and _docs_kernels_enabled()
            and (dropout_p == 0.0 or _dropout_kernels_enabled())):
        if not hasattr(_load_ext(), "flash_attn_fwd_v3_docs"):
            raise RuntimeError(
                "_hip_ops has no flash_attn_fwd_v3_docs: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        scale = 1.0 / math.sqrt(q.shape[-1])
        return _FlashAttnDocs.apply(q, k, v, doc_start, doc_end, scale,
                                    float(dropout_p))
    return F.scaled_dot_product_attention(
        q, k, v, attn_mask=doc_mask(doc_start), dropout_p=dropout_p)


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    dropout_p: float = 0.0, doc_ids=None) -> torch.Tensor:
    """Causal attention; custom MFMA kernels when usable, SDPA
    otherwise.

    ``dropout_p > 0`` drops attention probabilities (and scales the kept
    ones by ``1/(1-p)``): inside the custom kernels when the call is
    usable and the dropout kernels are enabled (module docstring), else
    through ``F.scaled_dot_product_attention``. Raises ``ValueError``
    for ``dropout_p`` outside ``[0, 1)``.

    ``doc_ids`` (integer [B, T], or the ``doc_bounds`` pair) makes the
    attention causal within each document of a packed row (module
    docstring); ``None`` is the call without it. Raises ``ValueError``
    for ids of the wrong shape or of a floating dtype."""
    _check_p(dropout_p)
    if doc_ids is not None:
        return _docs_attention(q, k, v, dropout_p, doc_ids)
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
