"""Multi-token attention over a KV cache: extend rows that already have a
cache by ``T`` tokens in one call (the next turn of a conversation, a
slice of a chunked prefill, several drafted tokens to verify).

``append_attention(qkv, k_cache, v_cache, pos)``:

- ``qkv`` [B, T, 3*H*hs] is ``c_attn``'s output for the new tokens, taken
  as it is (token ``(b, t)``: q, then k, then v, each ``H*hs`` wide);
- ``k_cache`` / ``v_cache`` [B, H, Tmax, hs] are updated in place at
  slots ``pos[b] .. pos[b]+T-1``;
- ``pos`` int32 [B], on the device, is the number of tokens row ``b``
  has cached. Query ``t`` of row ``b`` attends cache slots
  ``0 .. pos[b]-1`` and new tokens ``0 .. t``, which are read from
  ``qkv``, never from the cache. ``pos`` is never read on the host;
- ``max_pos`` (host int, default ``Tmax - T``) is the caller's promise
  that no ``pos[b]`` exceeds it; ``max_pos + T <= Tmax``. A row whose
  ``pos[b]`` lies outside ``[0, max_pos]`` is inactive: its cache row
  stays as it is and its output rows are zero;
- the result is [B, T, H*hs], ready for ``c_proj``.

On the GPU, for bf16 and head size 64, this is the MFMA split-KV kernel
pair of csrc/append_attn.hip (docs/DESIGN.md §15,
profiles/append_attn.md): a (KV chunks, query tiles, B*H) grid, fp32
partials folded in chunk order, the append done by the workgroups of
query tile 0. The chunk partition depends on the position alone, so a
row's bits do not depend on its batch. Whether the kernel is the default
is ``_APPEND_DEFAULT`` below; ``RLA_APPEND_ATTN=1`` / ``=0`` forces it on
/ off. Everything else (CPU, other dtypes and head sizes, the gate off)
runs the torch twin with the same semantics: ``scatter_`` into the
caches, then a masked softmax in fp32 (on the GPU: SDPA with the same
mask).

Over an fp8 cache (``k_scale`` / ``v_scale`` given, ops/decode_attn.py) the
contract is ``decode_attention``'s: the ``T`` new rows are quantized as
``quantize_kv`` does and stored as codes and scales, and query ``t``
attends the dequantized cache and the dequantized new rows ``0 .. t``:
attention over the cache as the call leaves it. On the GPU that is the fp8
variant of the same kernel under the same gate (docs/DESIGN.md §21,
profiles/append_attn_fp8.md): codes and scales go from global memory to
registers, ``v_cvt_scalef32_pk_bf16_fp8`` makes them the MFMA's bf16
operands, and the new rows are quantized, stored and attended as stored in
the launch. Its twin (``_fp8``: CPU, other shapes, the gate off) is a torch
composition: ``quantize_kv`` and a byte ``scatter_``, the caches
dequantized into bf16 temporaries, then the bf16 path above on those.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _load_ext

# Set by the rule of profiles/append_attn.md: True iff the kernel beats
# both index_copy_ + SDPA and T decode_attention calls at all nine B = 8
# points by more than the spread of either. It does, by 1.3x to 5.1x and 3.7x
# to 28x.
_APPEND_DEFAULT = True

_CHUNK_FALLBACK = 128


def append_attn_chunk() -> int:
    """KV positions per workgroup of the append kernel."""
    ext = _load_ext()
    if ext is not None and hasattr(ext, "append_attn_chunk"):
        return int(ext.append_attn_chunk())
    return _CHUNK_FALLBACK


def _kernel_enabled() -> bool:
    env = os.environ.get("RLA_APPEND_ATTN")
    if env is None:
        return _APPEND_DEFAULT
    return env == "1"


def _kernel_shape(qkv: torch.Tensor, k_cache: torch.Tensor) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16
            and k_cache.dim() == 4 and k_cache.shape[-1] == 64
            and _load_ext() is not None)


def _twin(qkv, k_cache, v_cache, pos, max_pos):
    B, H, Tmax, hs = k_cache.shape
    T = qkv.shape[1]
    dev = qkv.device
    q, k, v = (x.transpose(1, 2)                      # [B, H, T, hs]
               for x in qkv.view(B, T, 3, H, hs).unbind(2))
    active = (pos >= 0) & (pos <= max_pos)
    steps = torch.arange(T, device=dev)
    # inactive rows write back what slots they read, bit for bit
    slot = pos.clamp(0, Tmax - T).to(torch.int64)[:, None] + steps  # [B, T]
    index = slot.view(B, 1, T, 1).expand(B, H, T, hs)
    keep = active.view(B, 1, 1, 1)
    for cache, new in ((k_cache, k), (v_cache, v)):
        old = cache.gather(2, index)
        cache.scatter_(2, index, torch.where(keep, new, old))
    s_pos = torch.arange(Tmax, device=dev)
    last = pos[:, None] + steps                                  # [B, T]
    mask = (s_pos <= last[:, :, None]) & active[:, None, None]   # [B,T,Tmax]
    mask = mask[:, None]                                         # [B,1,T,Tmax]
    # slots past pos[b] + T - 1 may hold anything, NaN included
    held = ((s_pos < (pos + T)[:, None]) & active[:, None])[:, None, :, None]
    zero = torch.zeros((), dtype=k_cache.dtype, device=dev)
    kz = torch.where(held, k_cache, zero)
    vz = torch.where(held, v_cache, zero)
    if qkv.is_cuda:
        o = F.scaled_dot_product_attention(q, kz, vz, attn_mask=mask)
    else:
        s = torch.einsum("bhtd,bhsd->bhts", q.float(), kz.float())
        s = (s / math.sqrt(hs)).masked_fill(~mask, -math.inf)
        o = torch.einsum("bhts,bhsd->bhtd", torch.softmax(s, dim=-1),
                         vz.float())
    # a row with nothing to attend is all -inf: NaN from the softmax
    o = torch.where(active.view(B, 1, 1, 1), o.to(qkv.dtype),
                    torch.zeros((), dtype=qkv.dtype, device=dev))
    return o.transpose(1, 2).reshape(B, T, H * hs)


def _fp8(qkv, k_cache, v_cache, k_scale, v_scale, pos, max_pos):
    """The fp8 kernel's twin: quantize and store the new rows, then the
    bf16 op on dequantized temporaries (module docstring)."""
    from .decode_attn import dequantize_kv, quantize_kv
    B, H, Tmax, hs = k_cache.shape
    T = qkv.shape[1]
    parts = qkv.view(B, T, 3, H, hs).unbind(2)
    active = (pos >= 0) & (pos <= max_pos)
    slot = pos.clamp(0, Tmax - T).to(torch.int64)[:, None] + \
        torch.arange(T, device=qkv.device)                      # [B, T]
    index = slot.view(B, 1, T).expand(B, H, T)
    idx4 = index.unsqueeze(3).expand(B, H, T, hs)
    keep = active.view(B, 1, 1)
    new = [parts[0]]
    for cache, scale, x in ((k_cache, k_scale, parts[1]),
                            (v_cache, v_scale, parts[2])):
        codes, s = quantize_kv(x.transpose(1, 2))               # [B, H, T, .]
        # inactive rows write back what they read; fp8 moves as bytes
        bytes_ = cache.view(torch.uint8)
        bytes_.scatter_(2, idx4, torch.where(
            keep.unsqueeze(3), codes.view(torch.uint8),
            bytes_.gather(2, idx4)))
        scale.scatter_(2, index, torch.where(keep, s,
                                             scale.gather(2, index)))
        new.append(dequantize_kv(codes, s, qkv.dtype).transpose(1, 2))
    # slots not held yet may carry the NaN code or a NaN scale; the bf16
    # op never attends them, as it never attends NaN in a bf16 cache
    return append_attention(
        torch.stack(new, dim=2).reshape(B, T, 3 * H * hs),
        dequantize_kv(k_cache, k_scale, qkv.dtype),
        dequantize_kv(v_cache, v_scale, qkv.dtype), pos, max_pos)


def append_attention(qkv: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, pos: torch.Tensor,
                     max_pos: Optional[int] = None,
                     n_head: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``T`` new tokens per row against the KV cache, with the append
    (module docstring). ``n_head``, when given, must be the caches' H.
    ``k_scale`` / ``v_scale`` come with float8_e4m3fn caches."""
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError("k_cache and v_cache must share one "
                         "[B, H, Tmax, hs] shape")
    B, H, Tmax, hs = k_cache.shape
    if n_head is not None and n_head != H:
        raise ValueError(f"n_head = {n_head}, the caches hold {H} heads")
    if max_pos is None:
        max_pos = Tmax - (qkv.shape[1] if qkv.dim() == 3 else 1)
    if _kernel_shape(qkv, k_cache) and _kernel_enabled():
        ext = _load_ext()
        if not hasattr(ext, "append_attn_fwd"):
            raise RuntimeError(
                "_hip_ops has no append_attn_fwd: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        # the one checked host path: every other operand check is there
        if k_scale is not None or v_scale is not None:
            return ext.append_attn_fwd(qkv, k_cache, v_cache, pos,
                                       int(max_pos), 1.0 / math.sqrt(hs),
                                       k_scale, v_scale)
        return ext.append_attn_fwd(qkv, k_cache, v_cache, pos,
                                   int(max_pos), 1.0 / math.sqrt(hs))
    from .decode_attn import _check_scales
    _check_scales(k_cache, v_cache, k_scale, v_scale)
    if k_scale is not None:
        if qkv.dim() != 3 or qkv.shape[0] != B or qkv.shape[1] < 1 \
                or qkv.shape[2] != 3 * H * hs:
            raise ValueError(
                f"qkv must be [B, T, 3*H*hs] = [{B}, T >= 1, {3 * H * hs}], "
                f"got {list(qkv.shape)}")
        if pos.dtype != torch.int32 or tuple(pos.shape) != (B,) \
                or pos.device != qkv.device or k_cache.device != qkv.device:
            raise ValueError("pos must be int32 [B] and the caches on "
                             "qkv's device")
        if not (0 <= max_pos and max_pos + qkv.shape[1] <= Tmax):
            raise ValueError(
                f"max_pos = {max_pos} with T = {qkv.shape[1]} new tokens "
                f"does not fit Tmax = {Tmax}")
        return _fp8(qkv.contiguous(), k_cache, v_cache, k_scale, v_scale,
                    pos, int(max_pos))
    if qkv.dim() != 3 or qkv.shape[0] != B or qkv.shape[1] < 1 \
            or qkv.shape[2] != 3 * H * hs:
        raise ValueError(
            f"qkv must be [B, T, 3*H*hs] = [{B}, T >= 1, {3 * H * hs}], "
            f"got {list(qkv.shape)}")
    for c in (k_cache, v_cache):
        if c.dtype != qkv.dtype or c.device != qkv.device:
            raise ValueError("the caches must have qkv's dtype and device")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (B,) \
            or pos.device != qkv.device:
        raise ValueError("pos must be int32 [B] on qkv's device")
    if not (0 <= max_pos and max_pos + qkv.shape[1] <= Tmax):
        raise ValueError(
            f"max_pos = {max_pos} with T = {qkv.shape[1]} new tokens does "
            f"not fit Tmax = {Tmax}")
    return _twin(qkv.contiguous(), k_cache, v_cache, pos, int(max_pos))
