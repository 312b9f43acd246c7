"""Chunked linear + cross-entropy for large-vocab LM heads, with
``ignore_index``, label smoothing and z-loss.

The naive GPT-2 loss path materializes the full logits tensor twice
(bf16 GEMM output + ``.float()`` copy: ~1.6 GB at B=8, T=1024,
V=50257) and keeps it alive for backward. This computes the loss in
row chunks, keeping only O(chunk * V) live, and recomputes the chunk
logits in backward. Per row with logits ``z``, target ``t``, smoothing
``e`` and z-loss weight ``l``:

    lse  = logsumexp(z)
    loss = lse - (1-e) z_t - (e/V) sum_j z_j + l lse^2
    dz_j = g ((1 + 2 l lse) softmax(z)_j - (1-e) [j==t] - e/V)
    dx   = dz @ W
    dW   = sum_chunks dz^T @ x_chunk           (fp32 accumulator)

which is ``F.cross_entropy(logits.float(), t, ignore_index=,
label_smoothing=)`` plus the z-loss term ``l * lse^2``. Rows whose
target is ``ignore_index`` contribute neither loss nor gradient, and
``reduction="mean"`` divides by the number of non-ignored rows counted
over ALL rows (not per chunk), as a device tensor.

One deliberate difference from ``F.cross_entropy``: when every row is
ignored the loss is 0 with zero gradients (the count is clamped to 1)
instead of NaN, so a rank that draws an all-padding micro-batch does
not poison the gradient all-reduce.

Two implementations sit behind ``chunked_cross_entropy``:

- torch: GEMM -> ``.float()`` -> ``logsumexp``/``gather`` forward,
  ``softmax``/``scatter_add_`` backward. The CPU tier and the fallback.
- fused: GEMM -> ``fused_ce_fwd`` straight on the bf16/fp32 GEMM output
  (one pass, no fp32 copy; saves ``lse`` for all N rows), and in
  backward GEMM -> ``fused_ce_bwd`` in place over the recomputed logits
  (one pass) -> the two gradient GEMMs. Kernels: ``csrc/fused_ce.hip``. The gradient
  scale ``gout / count`` stays on the device; nothing reads back to the
  host.

The fused path needs GPU bf16/fp32 inputs and the HIP extension.
``RLA_FUSED_CE=1`` / ``=0`` forces it on / off; unset,
``_FUSED_DEFAULT`` below decides (profiles/fused_ce.md).
"""
from __future__ import annotations

import os

import torch

from . import _require_ext

# Set by the measurement in profiles/fused_ce.md: the fused kernels are
# the default iff they beat the torch path there by more than the
# run-to-run spread and the whole GPT-2 step is not worse.
_FUSED_DEFAULT = True


def _rows_loss(logits, lse, tgt_idx, valid, label_smoothing, z_loss):
    """Per-row loss from fp32 logits; ``tgt_idx`` is already safe to
    gather with. With both options off this is ``lse - z_t``."""
    tgt = logits.gather(1, tgt_idx[:, None]).squeeze(1)
    if label_smoothing > 0.0:
        rows = (lse - (1.0 - label_smoothing) * tgt
                - label_smoothing * logits.mean(dim=-1))
    else:
        rows = lse - tgt
    if z_loss > 0.0:
        rows = rows + z_loss * lse * lse
    return torch.where(valid, rows, torch.zeros_like(rows))


class _ChunkedLinearCE(torch.autograd.Function):
    """The torch path."""

    @staticmethod
    def forward(ctx, x, weight, targets, chunk_rows, ignore_index,
                label_smoothing, z_loss, mean):
        n = x.shape[0]
        valid = targets != ignore_index
        # gather/scatter need an in-range index on ignored rows too
        tgt_idx = torch.where(valid, targets, torch.zeros_like(targets))
        loss_sum = x.new_zeros((), dtype=torch.float32)
        for i in range(0, n, chunk_rows):
            xc = x[i:i + chunk_rows]
            logits = (xc @ weight.t()).float()
            lse = torch.logsumexp(logits, dim=-1)
            loss_sum += _rows_loss(
                logits, lse, tgt_idx[i:i + chunk_rows],
                valid[i:i + chunk_rows], label_smoothing, z_loss).sum()
        if mean:
            denom = valid.sum().to(torch.float32).clamp(min=1)
        else:
            denom = x.new_ones((), dtype=torch.float32)
        ctx.save_for_backward(x, weight, tgt_idx, valid, denom)
        ctx.chunk_rows = chunk_rows
        ctx.label_smoothing, ctx.z_loss = label_smoothing, z_loss
        return loss_sum / denom

    @staticmethod
    def backward(ctx, gout):
        x, weight, tgt_idx, valid, denom = ctx.saved_tensors
        chunk_rows = ctx.chunk_rows
        eps, lam = ctx.label_smoothing, ctx.z_loss
        n = x.shape[0]
        v = weight.shape[0]
        # per-row scale: gout / count, 0 on ignored rows
        scale = (gout.float() / denom) * valid.to(torch.float32)
        dx = torch.empty_like(x)
        dw32 = torch.zeros(weight.shape, dtype=torch.float32,
                           device=weight.device)
        for i in range(0, n, chunk_rows):
            xc = x[i:i + chunk_rows]
            logits = (xc @ weight.t()).float()
            if lam > 0.0:
                lse = torch.logsumexp(logits, dim=-1, keepdim=True)
                probs = torch.softmax(logits, dim=-1)
                probs *= 1.0 + 2.0 * lam * lse
            else:
                probs = torch.softmax(logits, dim=-1)
            probs.scatter_add_(
                1, tgt_idx[i:i + chunk_rows, None],
                torch.full((xc.shape[0], 1), -(1.0 - eps),
                           dtype=torch.float32, device=x.device))
            if eps > 0.0:
                probs -= eps / v
            dlogits = (probs * scale[i:i + chunk_rows, None]).to(x.dtype)
            dx[i:i + chunk_rows] = dlogits @ weight
            dw32 += (dlogits.t() @ xc).float()
        return (dx, dw32.to(weight.dtype), None, None, None, None, None,
                None)


class _FusedLinearCE(torch.autograd.Function):
    """GEMM -> fused_ce_fwd; backward GEMM -> fused_ce_bwd in place."""

    @staticmethod
    def forward(ctx, x, weight, targets, chunk_rows, ignore_index,
                label_smoothing, z_loss, mean):
        ext = _require_ext()
        n = x.shape[0]
        # lse as an fp32 pair [hi; lo] (csrc/fused_ce.hip)
        lse = torch.empty(2, n, dtype=torch.float32, device=x.device)
        loss_sum = x.new_zeros((), dtype=torch.float32)
        for i in range(0, n, chunk_rows):
            logits = x[i:i + chunk_rows] @ weight.t()
            rows, lse_c, lo_c = ext.fused_ce_fwd(
                logits, targets[i:i + chunk_rows], ignore_index,
                label_smoothing, z_loss)
            lse[0, i:i + chunk_rows] = lse_c
            lse[1, i:i + chunk_rows] = lo_c
            loss_sum += rows.sum()
        if mean:
            denom = (targets != ignore_index).sum().to(
                torch.float32).clamp(min=1)
        else:
            denom = x.new_ones((), dtype=torch.float32)
        ctx.save_for_backward(x, weight, targets, lse, denom)
        ctx.chunk_rows = chunk_rows
        ctx.opts = (ignore_index, label_smoothing, z_loss)
        return loss_sum / denom

    @staticmethod
    def backward(ctx, gout):
        ext = _require_ext()
        x, weight, targets, lse, denom = ctx.saved_tensors
        chunk_rows = ctx.chunk_rows
        ignore_index, label_smoothing, z_loss = ctx.opts
        n = x.shape[0]
        # gout / count as a 1-element device tensor, read by the kernel
        gscale = (gout.float() / denom).reshape(1)
        dx = torch.empty_like(x)
        dw32 = torch.zeros(weight.shape, dtype=torch.float32,
                           device=weight.device)
        for i in range(0, n, chunk_rows):
            xc = x[i:i + chunk_rows]
            # backward owns the recomputed logits: dlogits goes over them
            dlogits = ext.fused_ce_bwd(
                xc @ weight.t(), lse[0, i:i + chunk_rows],
                lse[1, i:i + chunk_rows],
                targets[i:i + chunk_rows], gscale, ignore_index,
                label_smoothing, z_loss, True)
            dx[i:i + chunk_rows] = dlogits @ weight
            dw32 += (dlogits.t() @ xc).float()
        return (dx, dw32.to(weight.dtype), None, None, None, None, None,
                None)


def _fused_enabled() -> bool:
    env = os.environ.get("RLA_FUSED_CE")
    if env is None:
        return _FUSED_DEFAULT
    return env == "1"


def _use_fused(x: torch.Tensor, weight: torch.Tensor) -> bool:
    if not _fused_enabled():
        return False
    if not (x.is_cuda and weight.device == x.device
            and weight.dtype == x.dtype
            and x.dtype in (torch.bfloat16, torch.float32)):
        return False
    ext = _require_ext()
    if ext is None:  # RLA_ALLOW_EAGER_GPU=1 without a built extension
        return False
    if not hasattr(ext, "fused_ce_fwd"):
        raise RuntimeError(
            "_hip_ops has no fused_ce_fwd: rebuild with "
            "`python -m ray_lightning_amd.ops.build`")
    return True


def chunked_cross_entropy(x: torch.Tensor, weight: torch.Tensor,
                          targets: torch.Tensor,
                          chunk_rows: int = None, *,
                          ignore_index: int = -100,
                          label_smoothing: float = 0.0,
                          z_loss: float = 0.0,
                          reduction: str = "mean") -> torch.Tensor:
    """Cross-entropy of ``x @ weight.T`` against ``targets`` without
    materializing the full logits. ``x``: [N, C] (bf16/f32),
    ``weight``: [V, C], ``targets``: [N] int64.

    Rows with ``targets == ignore_index`` are left out. ``reduction`` is
    ``"mean"`` (over the non-ignored rows of all N; 0, not NaN, when
    there are none) or ``"sum"`` (for callers that normalise by a token
    count of their own). ``label_smoothing`` in ``[0, 1)`` and
    ``z_loss >= 0`` (weight of ``logsumexp^2``) as in the module
    docstring; anything else raises ``ValueError``."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(
            f"label_smoothing has to be in [0, 1), but got "
            f"{label_smoothing}")
    if z_loss < 0.0:
        raise ValueError(f"z_loss has to be >= 0, but got {z_loss}")
    if reduction not in ("mean", "sum"):
        raise ValueError(
            f"reduction has to be 'mean' or 'sum', but got {reduction!r}")
    if chunk_rows is None:
        chunk_rows = int(os.environ.get("RLA_CE_CHUNK_ROWS", "8192"))
    fn = _ChunkedLinearCE
    if _use_fused(x, weight):
        fn = _FusedLinearCE
        x, targets = x.contiguous(), targets.contiguous()
    return fn.apply(x, weight, targets, chunk_rows, int(ignore_index),
                    float(label_smoothing), float(z_loss),
                    reduction == "mean")
