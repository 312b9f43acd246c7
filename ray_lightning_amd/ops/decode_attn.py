"""Single-token attention over a KV cache (generation's decode step).

``decode_attention(qkv, k_cache, v_cache, pos)`` attends the one new
token of every row over what the row has cached and appends the token's
k and v to the caches, in one call:

- ``qkv`` [B, 3*H*hs] is ``c_attn``'s output for the new tokens, taken
  as it is (row ``b``: q, then k, then v, each ``H*hs`` wide);
- ``k_cache`` / ``v_cache`` [B, H, Tmax, hs] are updated in place at
  slot ``pos[b]``;
- ``pos`` int32 [B], on the device, is the number of tokens row ``b``
  has cached. Row ``b`` attends cache slots ``0 .. pos[b]-1`` and the
  new token, which is read from ``qkv``, never from the cache. Rows may
  differ, so prompts of different lengths share a batch. ``pos`` is
  never read on the host;
- ``max_pos`` (host int, default ``Tmax - 1``) is the caller's promise
  that no ``pos[b]`` exceeds it. A row whose ``pos[b]`` lies outside
  ``[0, max_pos]`` is inactive: its cache row stays as it is and its
  output is zero;
- the result is [B, H*hs], ready for ``c_proj``.

On the GPU, for bf16 and head size 64, this is the split-KV HIP kernel
of csrc/decode_attn.hip: a (KV chunks, B*H) grid of streaming reads,
fp32 partials folded in chunk order by a second small kernel, the append
done by the workgroup that owns slot ``pos[b]`` (docs/DESIGN.md §13,
profiles/gpt2_generate.md). The chunk partition depends on the position
alone, so a row's bits do not depend on its batch. Whether the kernel is
the default is ``_DECODE_DEFAULT`` below; ``RLA_DECODE_ATTN=1`` / ``=0``
forces it on / off. Everything else (CPU, other dtypes and head sizes,
the gate off) runs the torch twin with the same semantics: ``scatter_``
into the caches, then a masked softmax in fp32 (on the GPU: SDPA with
the same mask).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import _load_ext

# Set by the measurement in profiles/gpt2_generate.md: the kernel is the
# default iff it beats index_copy_ + SDPA there at all three lengths for
# B = 8.
_DECODE_DEFAULT = True

# the kernel's KV positions per workgroup when the extension is absent
# (cache sizes are rounded to it either way)
_CHUNK_FALLBACK = 128


def decode_attn_chunk() -> int:
    """KV positions per workgroup of the decode kernel."""
    ext = _load_ext()
    if ext is not None and hasattr(ext, "decode_attn_chunk"):
        return int(ext.decode_attn_chunk())
    return _CHUNK_FALLBACK


def _kernel_enabled() -> bool:
    env = os.environ.get("RLA_DECODE_ATTN")
    if env is None:
        return _DECODE_DEFAULT
    return env == "1"


def _kernel_shape(qkv: torch.Tensor, k_cache: torch.Tensor) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16
            and k_cache.dim() == 4 and k_cache.shape[-1] == 64
            and _load_ext() is not None)


def _twin(qkv, k_cache, v_cache, pos, max_pos):
    B, H, Tmax, hs = k_cache.shape
    q, k, v = qkv.view(B, 3, H, hs).unbind(1)
    active = (pos >= 0) & (pos <= max_pos)
    # inactive rows write back what slot they read, bit for bit
    slot = pos.clamp(0, Tmax - 1).to(torch.int64)
    index = slot.view(B, 1, 1, 1).expand(B, H, 1, hs)
    keep = active.view(B, 1, 1, 1)
    for cache, new in ((k_cache, k), (v_cache, v)):
        old = cache.gather(2, index)
        cache.scatter_(2, index, torch.where(keep, new.unsqueeze(2), old))
    t = torch.arange(Tmax, device=pos.device)
    mask = (t[None, :] <= pos[:, None]) & active[:, None]   # [B, Tmax]
    mask = mask[:, None, :, None]                           # [B, 1, Tmax, 1]
    # slots past pos[b] may hold anything, NaN included
    kz = torch.where(mask, k_cache, torch.zeros((), dtype=k_cache.dtype,
                                                device=k_cache.device))
    vz = torch.where(mask, v_cache, torch.zeros((), dtype=v_cache.dtype,
                                                device=v_cache.device))
    if qkv.is_cuda:
        o = F.scaled_dot_product_attention(
            q.unsqueeze(2), kz, vz, attn_mask=mask.transpose(2, 3))
        o = o.squeeze(2)
    else:
        s = torch.einsum("bhd,bhtd->bht", q.float(), kz.float())
        s = (s / math.sqrt(hs)).masked_fill(~mask.squeeze(3), -math.inf)
        o = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1),
                         vz.float())
    # a row with nothing to attend is all -inf: NaN from the softmax
    o = torch.where(active.view(B, 1, 1), o.to(qkv.dtype),
                    torch.zeros((), dtype=qkv.dtype, device=qkv.device))
    return o.reshape(B, H * hs)


def decode_attention(qkv: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, pos: torch.Tensor,
                     max_pos: Optional[int] = None,
                     n_head: Optional[int] = None) -> torch.Tensor:
    """One new token per row against the KV cache, with the append
    (module docstring). ``n_head``, when given, must be the caches' H."""
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError("k_cache and v_cache must share one "
                         "[B, H, Tmax, hs] shape")
    B, H, Tmax, hs = k_cache.shape
    if n_head is not None and n_head != H:
        raise ValueError(f"n_head = {n_head}, the caches hold {H} heads")
    if max_pos is None:
        max_pos = Tmax - 1
    if _kernel_shape(qkv, k_cache) and _kernel_enabled():
        ext = _load_ext()
        if not hasattr(ext, "decode_attn_fwd"):
            raise RuntimeError(
                "_hip_ops has no decode_attn_fwd: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        # the one checked host path: every other operand check is there
        return ext.decode_attn_fwd(qkv, k_cache, v_cache, pos,
                                   int(max_pos), 1.0 / math.sqrt(hs))
    if qkv.dim() != 2 or tuple(qkv.shape) != (B, 3 * H * hs):
        raise ValueError(
            f"qkv must be [B, 3*H*hs] = {[B, 3 * H * hs]}, got "
            f"{list(qkv.shape)}")
    for c in (k_cache, v_cache):
        if c.dtype != qkv.dtype or c.device != qkv.device:
            raise ValueError("the caches must have qkv's dtype and device")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (B,) \
            or pos.device != qkv.device:
        raise ValueError("pos must be int32 [B] on qkv's device")
    if not 0 <= max_pos < Tmax:
        raise ValueError(
            f"max_pos = {max_pos} is outside [0, Tmax) = [0, {Tmax})")
    return _twin(qkv, k_cache, v_cache, pos, int(max_pos))


class KVCache:
    """Per-layer ``k`` / ``v`` caches [B, H, Tmax, hs] and the int32
    ``pos`` [B] that all layers share: the number of tokens each row has
    cached. ``max_pos`` is the host's upper bound on ``pos`` (what sizes
    the decode kernel's grid), kept in step by ``advance`` so the device
    values never have to be read back. ``prefilled`` tells a model's
    forward whether the call is the prefill or a decode step."""

    def __init__(self, n_layer: int, B: int, H: int, Tmax: int, hs: int,
                 dtype: torch.dtype, device) -> None:
        shape = (B, H, Tmax, hs)
        self.k: List[torch.Tensor] = [
            torch.zeros(shape, dtype=dtype, device=device)
            for _ in range(n_layer)]
        self.v: List[torch.Tensor] = [
            torch.zeros(shape, dtype=dtype, device=device)
            for _ in range(n_layer)]
        self.pos = torch.zeros(B, dtype=torch.int32, device=device)
        self.max_pos = 0
        self.Tmax = Tmax
        self.prefilled = False

    def set_lengths(self, lens: torch.Tensor, max_len: int) -> None:
        """After the prefill: row ``b`` holds ``lens[b]`` tokens (int32
        [B] on the cache's device), none more than ``max_len``."""
        self.pos.copy_(lens)
        self.max_pos = int(max_len)
        self.prefilled = True

    def advance(self) -> None:
        """One token appended to every row."""
        self.pos += 1
        self.max_pos += 1
