"""Framework-owned compute ops.

GPU path: hand-written CDNA4 HIP kernels (``csrc/``), built in-tree for
gfx950. The HIP extension is REQUIRED on GPU — ops raise rather than
silently falling back to eager PyTorch on a GPU box (set
``RLA_ALLOW_EAGER_GPU=1`` only for A/B debugging). CPU path: plain torch
(used by the gloo test tier).

Kernels (SURVEY.md N3/N6 hand-tuned halves):
- multi-tensor gradient pack (flatten, optional fp32->bf16 cast)
- bucket unpack + 1/world scale (optional bf16->fp32 cast), fused
- fused SGD(momentum) and Adam/AdamW optimizer steps (multi-tensor)
- sharded fused Adam (bf16 params/grads, fp32 master state)
- global-norm clipping: multi-tensor sum of squares (deterministic, no
  atomics), in-place scale by a device scalar, and an optional gradient
  multiplier inside the fused optimizer kernels
- softmax cross-entropy forward/backward over logits rows with
  ignore_index, label smoothing and z-loss (``chunked_ce.py``)
- single-token attention over a KV cache, split along the KV range, with
  the cache append in the same launch (``decode_attn.py``)
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

_ext = None
_ext_err: Optional[str] = None


def _load_ext():
    global _ext, _ext_err
    if _ext is not None or _ext_err is not None:
        return _ext
    try:
        from . import _hip_ops  # built in-tree by ops/build.py
        _ext = _hip_ops
    except ImportError as e:
        _ext_err = str(e)
    return _ext


def hip_ext_available() -> bool:
    return _load_ext() is not None


def _require_ext():
    ext = _load_ext()
    if ext is None and os.environ.get("RLA_ALLOW_EAGER_GPU") != "1":
        raise RuntimeError(
            "ray_lightning_amd HIP extension (_hip_ops) is not built but a "
            "GPU op was requested. Build it with "
            "`python -m ray_lightning_amd.ops.build` "
            f"(import error: {_ext_err})")
    return ext


def pack_grads(slots: List[torch.Tensor], grads: List[torch.Tensor]) -> None:
    """Copy each grad (any shape) into its flat bucket slot, casting to
    the comm dtype if needed."""
    if not slots:
        return
    if slots[0].is_cuda:
        ext = _require_ext()
        if ext is not None:
            ext.multi_tensor_pack(slots, [g.reshape(-1) for g in grads])
            return
    flat_grads = [g.reshape(-1) for g in grads]
    if slots[0].dtype == flat_grads[0].dtype:
        torch._foreach_copy_(slots, flat_grads)
    else:
        for s, g in zip(slots, flat_grads):
            s.copy_(g)


def _flat_view(t: torch.Tensor) -> Optional[torch.Tensor]:
    """1-D alias of a dense tensor's memory (element order is irrelevant
    to a norm or a scale), or None when the layout has no such view.
    Covers contiguous and channels_last grads."""
    if t.is_contiguous():
        return t.view(-1)
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t.permute(0, 2, 3, 1).reshape(-1)
    if t.dim() == 5 and t.is_contiguous(
            memory_format=torch.channels_last_3d):
        return t.permute(0, 2, 3, 4, 1).reshape(-1)
    return None


def _kernel_dtypes(tensors: List[torch.Tensor]) -> bool:
    """The clip kernels cover the dtypes this project trains in (fp32,
    bf16). Gradients of any other dtype (fp16, fp64) are not a missing
    kernel but outside the kernels' contract: they take the torch math
    below, as they did before the kernels existed."""
    return all(t.dtype in (torch.float32, torch.bfloat16) for t in tensors)


def _wide(t: torch.Tensor) -> torch.dtype:
    """fp32, or the tensor's own dtype where that is wider (fp64)."""
    return torch.promote_types(t.dtype, torch.float32)


def grad_sumsq(tensors: List[torch.Tensor],
               device: Optional[torch.device] = None) -> torch.Tensor:
    """Sum of squares over a list of fp32/bf16 tensors, accumulated in
    fp32, as a 1-element fp32 tensor on the tensors' device (``device``
    only matters for an empty list). Never reads back to the host."""
    if not tensors:
        return torch.zeros(1, dtype=torch.float32, device=device)
    if tensors[0].is_cuda and _kernel_dtypes(tensors):
        ext = _require_ext()
        if ext is not None:
            flat = [_flat_view(t) for t in tensors]
            return ext.grad_sumsq(
                [t.reshape(-1) if f is None else f
                 for t, f in zip(tensors, flat)])
    # same order as the kernel: per-tensor squares summed in fp32
    per = [t.to(_wide(t)).pow(2).sum().float() for t in tensors]
    return torch.stack(per).sum().reshape(1)


def clip_coef(sumsq: torch.Tensor, max_norm: float):
    """``(norm, coef)`` from a sum of squares, by the definition
    ``torch.nn.utils.clip_grad_norm_`` uses (``error_if_nonfinite=False``):
    ``coef = min(1, max_norm / (norm + 1e-6))``; a non-finite norm
    propagates the same way. 1-element device ops, no host read."""
    norm = sumsq.sqrt()
    coef = torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)
    return norm, coef


def scale_grads_(tensors: List[torch.Tensor], coef: torch.Tensor) -> None:
    """In place ``g *= coef`` for every tensor, ``coef`` a 1-element
    tensor that stays on the device."""
    if not tensors:
        return
    if tensors[0].is_cuda and _kernel_dtypes(tensors):
        ext = _require_ext()
        if ext is not None:
            coef = coef.to(torch.float32).reshape(1)
            flat = [_flat_view(t) for t in tensors]
            ext.multi_tensor_scale([f for f in flat if f is not None],
                                   coef)
            for t, f in zip(tensors, flat):
                if f is None:  # exotic strides: no flat alias exists
                    t.mul_(coef)
            return
    for t in tensors:
        # multiply in fp32 and round once, like the kernel
        w = _wide(t)
        t.copy_((t.to(w) * coef.to(device=t.device, dtype=w)).to(t.dtype))


def unpack_scale(bucket, scale: float) -> None:
    """Apply the 1/world_size scale to a reduced bucket; when the comm
    dtype differs from the grad dtype, fuse the upcast with the scale."""
    if bucket.flat.is_cuda:
        ext = _require_ext()
        if ext is not None:
            if bucket.flat_grad is not None:
                ext.scale_cast(bucket.flat_grad, bucket.flat, scale)
            else:
                ext.scale_inplace(bucket.flat, scale)
            return
    if bucket.flat_grad is not None:
        bucket.flat_grad.copy_(bucket.flat)
        if scale != 1.0:
            bucket.flat_grad.mul_(scale)
    elif scale != 1.0:
        bucket.flat.mul_(scale)
