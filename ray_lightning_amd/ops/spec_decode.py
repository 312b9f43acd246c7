"""One step of prompt-lookup speculative decoding after the LM head:
sampling at ``T + 1`` positions per row, acceptance of the drafted
tokens, the EOS / padding / output write, the repair of the KV cache's
lengths and the next draft (docs/DESIGN.md §17).

``spec_step(logits, draft, seeds, emitted, limit, ...)`` takes the logits
[B, T1, V] of a forward over ``[last token, T drafts]`` (``T1 = T + 1``,
``1 <= T1 <= 16``) and returns ``(tok, n_commit, next_idx)``. For row
``b``:

* sampling: ``tok[b, t]`` is the token ``sample_tokens`` (ops/sample.py)
  gives for ``logits[b, t]``, seed ``seeds[b]`` and step ``emitted[b] +
  t``, where ``emitted[b]`` counts the tokens the row has emitted. A
  lookup draft is a point mass, so accepting drafts while the sampled
  token equals the drafted one is exact speculative sampling: from equal
  logits the row emits the tokens the plain seeded loop emits.
* commit: ``a`` is the number of leading ``t < T`` with ``tok[b, t] ==
  draft[b, t]`` (``a = T`` for a row finished on entry); ``n = min(a + 1,
  limit - emitted[b])``, 0 at the limit. For ``j < n`` in order: ``x =
  pad if finished[b] else tok[b, j]``; ``finished[b] |= x == eos``;
  ``out[b, col[b] + j] = x`` where that column exists. Then ``col[b] +=
  n``, ``emitted[b] += n``, ``pos[b] += n - T1`` (the cache advanced by
  ``T1``; the rejected slots are overwritten before they are attended)
  and ``n_commit[b] = n``.
* draft: the history is ``h = out[b, :col[b]]`` (the part inside
  ``out``). Among earlier positions ``s`` with ``s + g <= col - 1`` and
  ``h[s:s+g] == h[col-g:col]`` the longest ``g <= ngram`` wins, then the
  largest ``s``; the drafts continue the match, ``d[j] = e[s + g + j]``
  with ``e`` = ``h`` followed by ``d`` itself, so a match that runs off
  the end continues periodically. No match: ``d[j] = h[col - 1]``.
  ``next_idx[b] = [h[col-1], d[0 .. next_T-1]]`` is the next forward's
  input and ``next_idx[:, 1:]`` its ``draft``, served as the view it is.
  An empty history gives ``pad`` throughout. Tokens are compared by
  their low 32 bits.

``finished`` (bool [B]), ``out`` (int64 [B, L], ``L <= 16384``), ``col``
and ``emitted`` (int64 [B]), ``pos`` (int32 [B]) are updated in place.
``done`` (int32 [B], zero) is the kernel's per-row arrival counter, zero
again when the call returns; ``None`` allocates one.

On the GPU, for ``V <= 65536`` in bf16 or fp32, all of this is one launch
of csrc/spec_decode.hip (profiles/spec_decode.md). Everywhere else, and
with ``RLA_SPEC_DECODE=0``, a torch twin with the same contract runs: the
tokens from the sampler's twin, commit and draft in plain Python on the
host.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _load_ext
from .sample import _twin as _sample_twin

MAX_T1 = 16
MAX_NGRAM = 8
MAX_L = 16384


def _kernel_shape(logits: torch.Tensor) -> bool:
    ext = _load_ext()
    return (logits.is_cuda and ext is not None
            and logits.dtype in (torch.bfloat16, torch.float32)
            and hasattr(ext, "spec_items_per_thread")
            and ext.spec_items_per_thread(logits) != 0)


def draft_lookup(h, ngram: int, n: int, pad: int = 0):
    """``[h[-1], d[0 .. n-1]]`` of the module docstring for a history
    given as a list of ints."""
    if not h:
        return [pad] * (1 + n)
    H = len(h)
    best_g, best_e = 0, -1
    for e in range(H - 1):                  # the earlier occurrence ends at e
        g = 0
        while g < ngram and e - g >= 0 and h[e - g] == h[H - 1 - g]:
            g += 1
        if g and (g, e) > (best_g, best_e):
            best_g, best_e = g, e
    ext = list(h)
    for j in range(n):
        ext.append(ext[best_e + 1 + j] if best_g else h[-1])
    return ext[H - 1:]


def _check(logits, draft, seeds, emitted, limit, temperature, top_k, top_p,
           finished, eos, pad, out, col, pos, done, ngram, next_T):
    if logits.dim() != 3 or not logits.is_floating_point() or \
            not logits.is_contiguous():
        raise ValueError("logits must be a contiguous floating-point "
                         "[B, T1, V]")
    B, T1, V = logits.shape
    if V < 1 or not 1 <= T1 <= MAX_T1:
        raise ValueError(f"V >= 1 and 1 <= T1 <= {MAX_T1}")
    for name, t, ty in (("seeds", seeds, torch.int64),
                        ("emitted", emitted, torch.int64),
                        ("finished", finished, torch.bool),
                        ("col", col, torch.int64), ("pos", pos, torch.int32),
                        ("done", done, torch.int32)):
        if t.dtype != ty or tuple(t.shape) != (B,) or \
                t.device != logits.device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {ty} [B] on "
                             "logits' device")
    if draft.dtype != torch.int64 or tuple(draft.shape) != (B, T1 - 1) or \
            draft.device != logits.device or \
            (T1 > 1 and draft.stride(1) != 1):
        raise ValueError("draft must be int64 [B, T1 - 1] on logits' device "
                         "with unit stride along a row")
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != B or \
            out.device != logits.device or not out.is_contiguous() or \
            not 1 <= out.shape[1] <= MAX_L:
        raise ValueError(f"out must be a contiguous int64 [B, L], L <= "
                         f"{MAX_L}, on logits' device")
    if limit < 0:
        raise ValueError("limit must be >= 0")
    if not 1 <= ngram <= MAX_NGRAM:
        raise ValueError(f"ngram must be in [1, {MAX_NGRAM}]")
    if not 0 <= next_T < MAX_T1:
        raise ValueError(f"next_T must be in [0, {MAX_T1 - 1}]")
    if not -1 <= eos < 2 ** 31 or not 0 <= pad < 2 ** 31:
        raise ValueError("eos must be None or a token id, pad a token id")
    if not temperature >= 0:
        raise ValueError("temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1")
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError("top_p must be in (0, 1]")


def _twin(logits, draft, seeds, emitted, limit, temperature, top_k, top_p,
          finished, eos, pad, out, col, pos, ngram, next_T):
    B, T1, V = logits.shape
    steps = [e + t for e in emitted.tolist() for t in range(T1)]
    tok = _sample_twin(logits.view(B * T1, V), seeds.repeat_interleave(T1),
                       steps, temperature, top_k, top_p).view(B, T1)
    return commit_and_draft(tok, draft, emitted, limit, finished, eos, pad,
                            out, col, pos, ngram, next_T)


def commit_and_draft(tok, draft, emitted, limit, finished, eos, pad, out,
                     col, pos, ngram, next_T):
    """The commit and draft parts on sampled tokens ``tok`` [B, T1], on
    the host."""
    B, T1 = tok.shape
    T, L, dev = T1 - 1, out.shape[1], tok.device
    em, cols = emitted.tolist(), col.tolist()
    toks, drafts, fin = tok.tolist(), draft.tolist(), finished.tolist()
    n_commit, nxt = [], []
    for b in range(B):
        a = T
        if not fin[b]:
            a = 0
            while a < T and toks[b][a] == drafts[b][a]:
                a += 1
        n = max(0, min(a + 1, limit - em[b]))
        for j in range(n):
            x = pad if fin[b] else toks[b][j]
            fin[b] = fin[b] or x == eos
            if 0 <= cols[b] + j < L:
                out[b, cols[b] + j] = x
        cols[b] += n
        em[b] += n
        n_commit.append(n)
        h = out[b, :min(max(cols[b], 0), L)].tolist()
        nxt.append(draft_lookup(h, ngram, next_T, pad))
    col.copy_(torch.tensor(cols, dtype=torch.int64))
    emitted.copy_(torch.tensor(em, dtype=torch.int64))
    finished.copy_(torch.tensor(fin, dtype=torch.bool))
    ncom = torch.tensor(n_commit, dtype=torch.int64, device=dev)
    pos += (ncom - T1).to(torch.int32)
    return tok, ncom, torch.tensor(nxt, dtype=torch.int64, device=dev)


def spec_step(logits: torch.Tensor, draft: torch.Tensor,
              seeds: torch.Tensor, emitted: torch.Tensor, limit: int, *,
              temperature: float = 1.0, top_k: Optional[int] = None,
              top_p: Optional[float] = None, finished: torch.Tensor,
              eos: Optional[int] = None, pad: int = 0, out: torch.Tensor,
              col: torch.Tensor, pos: torch.Tensor, ngram: int = 3,
              next_T: int = 0, done: Optional[torch.Tensor] = None):
    """``(tok [B, T1], n_commit [B], next_idx [B, 1 + next_T])``, all
    int64 (module docstring). ``eos=None`` never finishes a row."""
    eos = -1 if eos is None else int(eos)
    if _kernel_shape(logits) and os.environ.get("RLA_SPEC_DECODE") != "0":
        ext = _load_ext()
        if not hasattr(ext, "spec_step"):
            raise RuntimeError(
                "_hip_ops has no spec_step: rebuild with "
                "`python -m ray_lightning_amd.ops.build`")
        if done is None:
            done = torch.zeros(logits.shape[0], dtype=torch.int32,
                               device=logits.device)
        # the one checked host path: every operand check is there
        return tuple(ext.spec_step(
            logits, draft, seeds, emitted, int(limit), float(temperature),
            top_k, top_p, finished, eos, int(pad), out, col, pos, done,
            int(ngram), int(next_T)))
    if done is None:
        done = torch.zeros(logits.shape[:1], dtype=torch.int32,
                           device=logits.device)
    _check(logits, draft, seeds, emitted, limit, temperature, top_k, top_p,
           finished, eos, pad, out, col, pos, done, ngram, next_T)
    return _twin(logits, draft, seeds, emitted, int(limit),
                 float(temperature), top_k, top_p, finished, eos, int(pad),
                 out, col, pos, int(ngram), int(next_T))
