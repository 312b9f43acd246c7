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

fp8 cache. ``quantize_kv(x)`` gives ``(codes, scale)`` for ``x`` [..., 64]
bf16: OCP ``float8_e4m3fn`` codes of the same shape and one fp32
power-of-two scale per row of 64, ``2^ceil(log2(absmax / 448))``; 136 bytes
per head and position where bf16 is 256. With ``k_scale`` / ``v_scale``
[B, H, Tmax] given, ``decode_attention`` takes the caches as codes: the new
token's k and v are quantized first, stored as codes and scales at slot
``pos[b]``, and the query attends their dequantized values, so the result
is attention over the cache as the call leaves it,

    out[b] = softmax(q[b] . dq(K[b, :, 0..pos[b]]) / 8) . dq(V[b, :, 0..pos[b]])

On the GPU that is the fp8 kernel of csrc/decode_attn.hip under the same
gate (docs/DESIGN.md §20, profiles/kv_fp8.md); ``kv_cache_fill`` is the
prefill's quantizing fill, a kernel of the same file. Their torch twins
compute in fp32 on dequantized values, with codes and scales from
``quantize_kv``. The contract covers finite rows; a row with a non-finite
value shows NaN in the output.
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


FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_kv(x: torch.Tensor):
    """``(codes, scale)`` for ``x`` [..., hs]: ``codes`` float8_e4m3fn of
    the same shape and ``scale`` fp32 [...], per row the smallest power of
    two with ``absmax / scale <= 448`` (1 for an all-zero row), so nothing
    saturates. ``dequantize_kv`` of the pair is exact in bf16, and
    quantizing that again gives the same pair."""
    w = x.detach().float()
    # frexp: absmax / 448 = m * 2^e with m in [0.5, 1), so ceil(log2) is e,
    # or e - 1 at m = 0.5; exact, where log2 would round
    m, e = torch.frexp(w.abs().amax(dim=-1) / FP8_MAX)
    e = torch.where(m == 0.5, e - 1, e)
    scale = torch.where(m == 0, torch.ones_like(m),
                        torch.ldexp(torch.ones_like(m), e))
    return (w / scale.unsqueeze(-1)).to(FP8), scale


def dequantize_kv(codes: torch.Tensor, scale: torch.Tensor,
                  dtype=torch.bfloat16) -> torch.Tensor:
    """``codes * scale`` per row in ``dtype`` (exact in bf16 and wider)."""
    return (codes.float() * scale.unsqueeze(-1)).to(dtype)


def _check_scales(k_cache, v_cache, k_scale, v_scale):
    """Both scales or neither; with them, fp8 caches and fp32
    [B, H, Tmax] scales on the caches' device."""
    if (k_scale is None) != (v_scale is None):
        raise ValueError("k_scale and v_scale come together or not at all")
    if (k_scale is not None) != (k_cache.dtype == FP8):
        raise ValueError(
            "float8_e4m3fn caches and k_scale / v_scale come together or "
            "not at all")
    if k_scale is None:
        return
    for s in (k_scale, v_scale):
        if s.dtype != torch.float32 or s.shape != k_cache.shape[:3] \
                or s.device != k_cache.device or v_cache.dtype != FP8:
            raise ValueError(
                "k_scale and v_scale must be fp32 [B, H, Tmax] = "
                f"{list(k_cache.shape[:3])} next to float8_e4m3fn caches")


def kv_cache_fill(qkv: torch.Tensor, k_cache: torch.Tensor,
                  v_cache: torch.Tensor, k_scale: torch.Tensor,
                  v_scale: torch.Tensor) -> None:
    """The prefill's fill of an fp8 cache: k and v of ``qkv`` [B, T, 3*H*hs]
    (``c_attn``'s packed output) quantized per (b, t, h) row into codes and
    scales at ``[:, :, :T]``; slots ``>= T`` stay as they are. On the GPU,
    for bf16 and head size 64, one HIP kernel (``RLA_DECODE_ATTN`` gates it
    with the decode kernel); otherwise ``quantize_kv`` and ``copy_``."""
    _check_scales(k_cache, v_cache, k_scale, v_scale)
    if k_scale is None:
        raise ValueError("kv_cache_fill fills float8_e4m3fn caches")
    if _kernel_shape(qkv, k_cache) and _kernel_enabled():
        ext = _load_ext()
        if not hasattr(ext, "kv_cache_fill"):
            raise RuntimeError(
                "_hip_ops has no kv_cache_fill: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        # the one checked host path: every other operand check is there
        ext.kv_cache_fill(qkv, k_cache, v_cache, k_scale, v_scale)
        return
    B, H, Tmax, hs = k_cache.shape
    if qkv.dim() != 3 or qkv.shape[0] != B or qkv.shape[2] != 3 * H * hs \
            or qkv.shape[1] > Tmax:
        raise ValueError(
            f"qkv must be [B, T <= Tmax, 3*H*hs] = [{B}, <= {Tmax}, "
            f"{3 * H * hs}], got {list(qkv.shape)}")
    T = qkv.shape[1]
    _, k, v = qkv.view(B, T, 3, H, hs).unbind(2)
    for cache, scale, new in ((k_cache, k_scale, k), (v_cache, v_scale, v)):
        codes, s = quantize_kv(new.transpose(1, 2))
        cache[:, :, :T].copy_(codes)
        scale[:, :, :T].copy_(s)


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


def _twin_fp8(qkv, k_cache, v_cache, k_scale, v_scale, pos, max_pos):
    """The bf16 twin on dequantized copies of the caches, with the new row
    replaced by its dequantized quantization; codes and scales of active
    rows are stored at slot ``pos[b]``."""
    B, H, Tmax, hs = k_cache.shape
    _, k, v = qkv.view(B, 3, H, hs).unbind(1)
    (kq, ks), (vq, vs) = quantize_kv(k), quantize_kv(v)
    qkv = torch.stack([qkv.view(B, 3, H, hs)[:, 0],
                       dequantize_kv(kq, ks, qkv.dtype),
                       dequantize_kv(vq, vs, qkv.dtype)], dim=1)
    active = (pos >= 0) & (pos <= max_pos)
    slot = pos.clamp(0, Tmax - 1).to(torch.int64)
    index = slot.view(B, 1, 1).expand(B, H, 1)
    keep = active.view(B, 1, 1)
    for cache, scale, codes, s in ((k_cache, k_scale, kq, ks),
                                   (v_cache, v_scale, vq, vs)):
        # fp8 has no gather / scatter: move the codes as bytes
        bytes_ = cache.view(torch.uint8)
        idx4 = index.unsqueeze(3).expand(B, H, 1, hs)
        old = bytes_.gather(2, idx4)
        bytes_.scatter_(2, idx4, torch.where(
            keep.unsqueeze(3), codes.view(torch.uint8).unsqueeze(2), old))
        scale.scatter_(2, index, torch.where(keep, s.unsqueeze(2),
                                             scale.gather(2, index)))
    # slots past pos[b] may hold the NaN code and NaN scales: the bf16
    # twin masks them as it masks NaN in a bf16 cache
    return _twin(qkv.reshape(B, 3 * H * hs),
                 dequantize_kv(k_cache, k_scale, qkv.dtype),
                 dequantize_kv(v_cache, v_scale, qkv.dtype), pos, max_pos)


def decode_attention(qkv: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, pos: torch.Tensor,
                     max_pos: Optional[int] = None,
                     n_head: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One new token per row against the KV cache, with the append
    (module docstring). ``n_head``, when given, must be the caches' H.
    ``k_scale`` / ``v_scale`` come with float8_e4m3fn caches."""
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
        if k_scale is not None or v_scale is not None:
            return ext.decode_attn_fwd(qkv, k_cache, v_cache, pos,
                                       int(max_pos), 1.0 / math.sqrt(hs),
                                       k_scale, v_scale)
        return ext.decode_attn_fwd(qkv, k_cache, v_cache, pos,
                                   int(max_pos), 1.0 / math.sqrt(hs))
    if qkv.dim() != 2 or tuple(qkv.shape) != (B, 3 * H * hs):
        raise ValueError(
            f"qkv must be [B, 3*H*hs] = {[B, 3 * H * hs]}, got "
            f"{list(qkv.shape)}")
    _check_scales(k_cache, v_cache, k_scale, v_scale)
    for c in (k_cache, v_cache):
        if (k_scale is None and c.dtype != qkv.dtype) \
                or c.device != qkv.device:
            raise ValueError("the caches must have qkv's dtype and device")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (B,) \
            or pos.device != qkv.device:
        raise ValueError("pos must be int32 [B] on qkv's device")
    if not 0 <= max_pos < Tmax:
        raise ValueError(
            f"max_pos = {max_pos} is outside [0, Tmax) = [0, {Tmax})")
    if k_scale is not None:
        return _twin_fp8(qkv, k_cache, v_cache, k_scale, v_scale, pos,
                         int(max_pos))
    return _twin(qkv, k_cache, v_cache, pos, int(max_pos))


class KVCache:
    """Per-layer ``k`` / ``v`` caches [B, H, Tmax, hs] and the int32
    ``pos`` [B] that all layers share: the number of tokens each row has
    cached. ``max_pos`` is the host's upper bound on ``pos`` (what sizes
    the decode kernel's grid), kept in step by ``advance`` so the device
    values never have to be read back. ``prefilled`` tells a model's
    forward whether the call is the prefill or a decode step. With
    ``dtype=torch.float8_e4m3fn`` ``k`` / ``v`` hold ``quantize_kv``'s
    codes and ``k_scale`` / ``v_scale`` are per-layer fp32 [B, H, Tmax]
    (ones at first); for every other dtype they are ``None``."""

    def __init__(self, n_layer: int, B: int, H: int, Tmax: int, hs: int,
                 dtype: torch.dtype, device) -> None:
        shape = (B, H, Tmax, hs)
        self.k: List[torch.Tensor] = [
            torch.zeros(shape, dtype=dtype, device=device)
            for _ in range(n_layer)]
        self.v: List[torch.Tensor] = [
            torch.zeros(shape, dtype=dtype, device=device)
            for _ in range(n_layer)]
        self.k_scale = self.v_scale = None
        if dtype == FP8:
            self.k_scale, self.v_scale = (
                [torch.ones(shape[:3], dtype=torch.float32, device=device)
                 for _ in range(n_layer)] for _ in range(2))
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

    def set_max_pos(self, max_pos: int) -> None:
        """The host's bound on ``pos`` after the device changed ``pos``
        itself (ops/spec_decode.py): what the caller read back."""
        self.max_pos = int(max_pos)

    def advance(self, n: int = 1) -> None:
        """``n`` tokens appended to every row."""
        self.pos += n
        self.max_pos += n
