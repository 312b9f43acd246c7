"""Token sampling for generation: top-k, top-p (nucleus) and a Philox
draw per row, with the decode loop's EOS / padding / output write.

``sample_tokens(logits, seeds, step, ...)`` returns the next token of
every row, int64 [B]. The contract (docs/DESIGN.md §16), for row ``b``
with logits ``l`` (bf16 or fp32; NaN counts as -inf, +inf as the largest
finite float):

1. ``K = {i : l_i >= the top_k-th largest logit}``, ties kept;
2. ``w_i = exp2((l_i - max l) * c)`` in fp32, ``c = fp32(log2 e /
   temperature)``;
3. ``m_i = floor(w_i * 2**40)`` as a 64-bit integer, 0 outside ``K``;
   every sum and comparison of mass from here on is integer arithmetic;
4. ``P = clamp(round_half_even(top_p * M), 1, M)`` with ``M = sum m``;
   ``i`` stays iff the mass of the strictly larger logits is below ``P``;
5. ``x`` is word 0 of ``Philox4x32-10(key=seeds[b], counter=(step_lo,
   step_hi, 0, 0))``, ``r = floor(M_N * x / 2**32)`` with ``M_N`` the kept
   mass; the token is the lowest kept index whose inclusive mass prefix,
   in index order, exceeds ``r``;
6. ``temperature == 0``: the lowest index among the largest logits;
7. a row with nothing above -inf gives token 0;
8. with ``finished`` (bool [B]), ``out`` (int64 [B, L]) and ``col``
   (int64 [B]): a finished row's token becomes ``pad``, ``finished[b] |=
   tok == eos``, and ``out[b, col[b]] = tok`` when ``0 <= col[b] < L``.

Given the fp32 weights the token is exact, so it is repeatable bit for
bit and depends on the row's logits, ``seeds[b]`` and ``step`` only: not
on ``B`` and not on which row it is.

On the GPU, for ``V <= 65536``, this is one launch of csrc/sample.hip
(profiles/fused_sample.md). Whether the kernel is the default is
``_SAMPLE_DEFAULT`` below; ``RLA_FUSED_SAMPLE=1`` / ``=0`` forces it on /
off. Everything else (CPU, larger ``V``, the gate off) runs the torch
twin with the same contract; its ``exp2`` may differ from the kernel's in
the last bit, so twin and kernel agree on the distribution, not on every
token. The twin reads ``seeds`` on the host.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _load_ext

# Set by the rule of profiles/fused_sample.md: True iff the kernel beats
# the ATen chain at all three B = 8, V = 50257 configurations by more than
# the spread of either. It does, by 2.8x, 5.3x and 4.3x.
_SAMPLE_DEFAULT = True

_FLT_MAX = torch.finfo(torch.float32).max
_LOG2E = 1.4426950408889634


def philox_word0(seed: int, step: int) -> int:
    """Word 0 of Philox4x32-10(key=seed, counter=(step_lo, step_hi, 0, 0))."""
    seed &= (1 << 64) - 1
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c = [step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 0, 0]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF,
             (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0]


def _kernel_enabled() -> bool:
    env = os.environ.get("RLA_FUSED_SAMPLE")
    if env is None:
        return _SAMPLE_DEFAULT
    return env == "1"


def _kernel_shape(logits: torch.Tensor) -> bool:
    ext = _load_ext()
    return (logits.is_cuda and ext is not None
            and logits.dtype in (torch.bfloat16, torch.float32)
            and hasattr(ext, "sample_items_per_thread")
            and ext.sample_items_per_thread(logits) != 0)


def _twin(logits, seeds, step, temperature, top_k, top_p):
    """``step`` is one int for all rows or a list of ``B`` ints."""
    B, V = logits.shape
    steps = step if isinstance(step, (list, tuple)) else [step] * B
    dev = logits.device
    l = torch.nan_to_num(logits.float(), nan=-torch.inf, posinf=_FLT_MAX,
                         neginf=-torch.inf)
    mx = l.max(dim=1, keepdim=True).values
    empty = mx[:, 0] == -torch.inf
    zero = torch.zeros(B, dtype=torch.int64, device=dev)
    if temperature == 0:
        # argmax returns the first of several maxima
        return torch.where(empty, zero, (l == mx).to(torch.int8).argmax(1))
    keep = torch.ones_like(l, dtype=torch.bool)
    if top_k is not None and top_k < V:
        keep = l >= l.topk(top_k, dim=1).values[:, -1:]
    c = torch.tensor(_LOG2E / temperature, dtype=torch.float32, device=dev)
    d = l - torch.where(empty[:, None], torch.zeros_like(mx), mx)
    w = torch.where(d == 0, torch.ones_like(d), torch.exp2(d * c))
    m = torch.where(keep, (w.double() * 2.0 ** 40).floor().to(torch.int64),
                    zero[:, None])
    if top_p is not None and top_p < 1.0:
        M = m.sum(1, keepdim=True)
        P = torch.minimum((top_p * M.double()).round().to(torch.int64)
                          .clamp(min=1), M.clamp(min=1))
        ls, order = l.sort(dim=1, descending=True, stable=True)
        ms = m.gather(1, order)
        above = ms.cumsum(1) - ms
        # the mass above a run of equal logits is that above its first
        start = torch.ones_like(keep)
        start[:, 1:] = ls[:, 1:] != ls[:, :-1]
        above = torch.where(start, above, -torch.ones_like(above)) \
            .cummax(dim=1).values
        kept = torch.zeros_like(keep).scatter_(1, order, above < P)
        m = torch.where(kept, m, zero[:, None])
    cum = m.cumsum(1)
    MN = cum[:, -1]
    x = torch.tensor([philox_word0(s, st)
                      for s, st in zip(seeds.tolist(), steps)],
                     dtype=torch.int64, device=dev)
    # floor(MN * x / 2^32) without leaving int64: MN = hi * 2^28 + lo
    hi, lo = MN >> 28, MN & ((1 << 28) - 1)
    r = (hi * x + ((lo * x) >> 28)) >> 4
    tok = torch.searchsorted(cum, r[:, None], right=True)[:, 0]
    return torch.where(empty, zero, tok.clamp(max=V - 1))


def sample_tokens(logits: torch.Tensor, seeds: torch.Tensor, step: int, *,
                  temperature: float = 1.0, top_k: Optional[int] = None,
                  top_p: Optional[float] = None,
                  finished: Optional[torch.Tensor] = None,
                  eos: Optional[int] = None, pad: int = 0,
                  out: Optional[torch.Tensor] = None,
                  col: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The next token of every row, int64 [B] (module docstring).
    ``finished``, ``out`` and ``col`` come together or not at all and are
    updated in place; ``eos=None`` never finishes a row."""
    eos = -1 if eos is None else int(eos)
    if _kernel_shape(logits) and _kernel_enabled():
        ext = _load_ext()
        if not hasattr(ext, "sample_fwd"):
            raise RuntimeError(
                "_hip_ops has no sample_fwd: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        # the one checked host path: every operand check is there
        return ext.sample_fwd(logits, seeds, int(step), float(temperature),
                              top_k, top_p, finished, eos, int(pad), out,
                              col)
    if logits.dim() != 2 or logits.shape[1] < 1 or \
            not logits.is_floating_point():
        raise ValueError("logits must be a floating-point [B, V], V >= 1")
    B = logits.shape[0]
    if seeds.dtype != torch.int64 or tuple(seeds.shape) != (B,):
        raise ValueError("seeds must be int64 [B]")
    if step < 0:
        raise ValueError("step must be >= 0")
    if not temperature >= 0:
        raise ValueError("temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1")
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError("top_p must be in (0, 1]")
    epilogue = finished is not None
    if (out is not None) != epilogue or (col is not None) != epilogue:
        raise ValueError("finished, out and col come together or not at all")
    if epilogue:
        if finished.dtype != torch.bool or tuple(finished.shape) != (B,):
            raise ValueError("finished must be bool [B]")
        if col.dtype != torch.int64 or tuple(col.shape) != (B,):
            raise ValueError("col must be int64 [B]")
        if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != B:
            raise ValueError("out must be int64 [B, L]")
        for t in (finished, col, out):
            if t.device != logits.device:
                raise ValueError("the epilogue tensors must be on logits' "
                                 "device")
    tok = _twin(logits, seeds, int(step), float(temperature), top_k, top_p)
    if epilogue:
        tok = torch.where(finished, tok.new_tensor(int(pad)), tok)
        finished |= tok == eos
        ok = (col >= 0) & (col < out.shape[1])
        at = col.clamp(0, out.shape[1] - 1)[:, None]
        out.scatter_(1, at, torch.where(ok[:, None], tok[:, None],
                                        out.gather(1, at)))
    return tok
