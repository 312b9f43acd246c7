"""GPT-2 family (bf16-first) — sharded-strategy benchmark model
(BASELINE.json config 4: GPT-2-XL, RayShardedStrategy, 8 workers).

Own implementation sized to the published GPT-2 configs. Attention uses
torch SDPA (AOTriton flash path on ROCm); matmuls hit hipBLASLt via
PyTorch-ROCm. The framework-owned hot path on this model is the sharded
gradient engine + the sharded fused-Adam HIP kernel.

The training loss is the chunked LM-head cross-entropy of
ops/chunked_ce.py: targets equal to ``cfg.ignore_index`` (-100: padding,
masked prompts, document boundaries) are left out of the mean, and
``cfg.label_smoothing`` / ``cfg.z_loss`` add the two usual LM loss
regularisers. Its softmax runs in the fused_ce HIP kernels when that
path is enabled (``RLA_FUSED_CE``, docs/CONFIG.md).

Packed rows: ``GPT2.forward(idx, targets, doc_ids=...)`` keeps attention
and positions within each document (``document_ids`` derives the ids
from an EOS token; ops/flash_attn.py has the kernels). Masking the
target that follows an EOS stays with the data pipeline, through
``ignore_index``.

Generation: ``GPT2.generate`` samples from the model with a KV cache
(ops/decode_attn.py): one prefill forward over the prompts on the flash
kernels, then one token per row per step through the split-KV decode
attention kernel, which also appends to the cache. ``forward(idx,
cache=...)`` is the same machinery one call at a time, and
``forward(idx, cache=..., extend=True)`` appends ``T`` tokens per row to
a filled cache through the MFMA append kernel (ops/append_attn.py): the
next turn of a conversation, a slice of a chunked prefill
(``generate(prefill_chunk=)``), drafted tokens to verify. With
``RLA_SKINNY_LINEAR`` on (docs/CONFIG.md), a decode step of a bf16 model
with at most 64 rows runs every block as one ``decode_layer`` call and
the final LayerNorm with the LM head as one ``skinny_linear`` call
(ops/skinny_linear.py). After ``GPT2.quantize_weights_fp8()`` those decode
steps stream the blocks' linear weights as fp8 (``RLA_SKINNY_FP8``), and
after ``quantize_weights_fp8(drop_bf16=True)`` the blocks keep the fp8
pairs only: prefill, ``extend`` and decode apply them through
``fp8_linear`` (ops/fp8_linear.py, docs/DESIGN.md §22).
``generate(kv_fp8=True)`` keeps the KV cache in fp8 (ops/decode_attn.py,
docs/DESIGN.md §20).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.fused_ln import FusedLayerNorm


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    # dropout (published GPT-2: 0.1 on all three). embd/resid run inside
    # the fused add+LayerNorm kernels, attn_pdrop inside the flash
    # attention kernels (ops/flash_attn.py); no mask is stored.
    embd_pdrop: float = 0.0
    resid_pdrop: float = 0.0
    attn_pdrop: float = 0.0
    # loss (ops/chunked_ce.py): targets equal to ignore_index are left
    # out of the mean; label smoothing and the z-loss weight
    # (z_loss * logsumexp^2) are off by default.
    ignore_index: int = -100
    label_smoothing: float = 0.0
    z_loss: float = 0.0

    @classmethod
    def gpt2(cls):
        return cls()

    @classmethod
    def gpt2_medium(cls):
        return cls(n_embd=1024, n_layer=24, n_head=16)

    @classmethod
    def gpt2_large(cls):
        return cls(n_embd=1280, n_layer=36, n_head=20)

    @classmethod
    def gpt2_xl(cls):
        return cls(n_embd=1600, n_layer=48, n_head=25)


def linear_dropped(lin: nn.Linear) -> bool:
    """Whether ``quantize_weights_fp8(drop_bf16=True)`` left ``lin`` with
    its fp8 pair only: an empty ``weight`` next to ``weight_fp8``."""
    return lin.weight.numel() == 0 and \
        getattr(lin, "weight_fp8", None) is not None


def _apply_linear(lin: nn.Linear, x, gelu: bool = False):
    """``lin(x)``, through ``fp8_linear`` (ops/fp8_linear.py) when the bf16
    weight was dropped; ``gelu`` is for dropped linears only."""
    if linear_dropped(lin):
        from ..ops.fp8_linear import fp8_linear
        return fp8_linear(x, lin.weight_fp8, lin.weight_scale, lin.bias,
                          gelu=gelu)
    return lin(x)


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.n_head = cfg.n_head
        self.attn_pdrop = cfg.attn_pdrop
        self.c_attn = nn.Linear(cfg.n_embd, 3 * cfg.n_embd)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd)

    def forward(self, x, doc_ids=None, cache=None, extend=False):
        """``cache`` is this layer's ``(k_cache, v_cache, kv)`` of a
        ``KVCache`` ``kv``. Before the prefill the call attends as it
        does without a cache and copies its k and v into the caches at
        ``[:, :, :T]``; after it, ``x`` is one new token per row and
        attention is ``decode_attention`` over the cache, or, with
        ``extend``, ``T`` new tokens per row and ``append_attention``. An
        fp8 cache's layer is ``(k_cache, v_cache, kv, k_scale, v_scale)``
        and is filled by ``kv_cache_fill``."""
        B, T, C = x.shape
        qkv = _apply_linear(self.c_attn, x)
        scales = {}
        if cache is not None and len(cache) == 5:
            scales = dict(k_scale=cache[3], v_scale=cache[4])
            cache = cache[:3]
        if extend:
            from ..ops.append_attn import append_attention
            k_cache, v_cache, kv = cache
            y = append_attention(qkv, k_cache, v_cache, kv.pos, kv.max_pos,
                                 self.n_head, **scales)
            return _apply_linear(self.c_proj, y)
        if cache is not None and cache[2].prefilled:
            from ..ops.decode_attn import decode_attention
            k_cache, v_cache, kv = cache
            y = decode_attention(qkv.view(B, 3 * C), k_cache, v_cache,
                                 kv.pos, kv.max_pos, self.n_head, **scales)
            return _apply_linear(self.c_proj, y.view(B, 1, C))
        if scales:
            from ..ops.decode_attn import kv_cache_fill
            kv_cache_fill(qkv, cache[0], cache[1], **scales)
        elif cache is not None:
            # the prefill's cache fill, from the strided k and v views
            hs = C // self.n_head
            _, k, v = qkv.split(C, dim=2)
            cache[0][:, :, :T].copy_(
                k.view(B, T, self.n_head, hs).transpose(1, 2))
            cache[1][:, :, :T].copy_(
                v.view(B, T, self.n_head, hs).transpose(1, 2))
        # hand-written MFMA flash kernels when the shape qualifies
        # (causal bf16 hs=64), dropout included, SDPA otherwise. Without
        # doc_ids the packed kernels take qkv as c_attn wrote it and
        # return y as c_proj reads it; with doc_ids (ids [B, T] or the
        # doc_bounds pair) the call still goes through flash_attention
        # on [B, H, T, 64] views.
        from ..ops.flash_attn import (flash_attention,
                                      flash_attention_qkvpacked)
        p = self.attn_pdrop if self.training else 0.0
        if doc_ids is None:
            return _apply_linear(
                self.c_proj,
                flash_attention_qkvpacked(qkv, self.n_head, dropout_p=p))
        hs = C // self.n_head
        q, k, v = (t.view(B, T, self.n_head, hs).transpose(1, 2)
                   for t in qkv.split(C, dim=2))
        y = flash_attention(q, k, v, dropout_p=p, doc_ids=doc_ids)
        return _apply_linear(
            self.c_proj, y.transpose(1, 2).contiguous().view(B, T, C))


class MLP(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.c_fc = nn.Linear(cfg.n_embd, 4 * cfg.n_embd)
        self.c_proj = nn.Linear(4 * cfg.n_embd, cfg.n_embd)

    def forward(self, x):
        # hand-written fused dGELU+bias-grad backward (ops/mlp.py);
        # the hipBLASLt-epilogue variant stays opt-in via RLA_LT_MLP=1
        # (measured slower on this library build — ops/lt_mlp.py)
        import os
        if linear_dropped(self.c_fc):
            # fp8 weights only (inference): GELU in the first call's
            # epilogue, not the training-only fused_mlp
            return _apply_linear(self.c_proj,
                                 _apply_linear(self.c_fc, x, gelu=True))
        if os.environ.get("RLA_LT_MLP", "0") == "1":
            from ..ops.lt_mlp import fused_mlp as lt_fused
            return lt_fused(x, self.c_fc.weight, self.c_fc.bias,
                            self.c_proj.weight, self.c_proj.bias)
        from ..ops.mlp import fused_mlp
        return fused_mlp(x, self.c_fc.weight, self.c_fc.bias,
                         self.c_proj.weight, self.c_proj.bias)


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln_1 = FusedLayerNorm(cfg.n_embd)
        self.attn = CausalSelfAttention(cfg)
        self.ln_2 = FusedLayerNorm(cfg.n_embd)
        self.mlp = MLP(cfg)
        self.resid_pdrop = cfg.resid_pdrop

    def forward(self, x, doc_ids=None):
        # standalone (unfused) path; GPT2.forward drives the fused
        # residual+LN chain across block boundaries instead
        p, tr = self.resid_pdrop, self.training
        x = x + F.dropout(self.attn(self.ln_1(x), doc_ids), p, tr)
        x = x + F.dropout(self.mlp(self.ln_2(x)), p, tr)
        return x


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = nn.Embedding(cfg.n_positions, cfg.n_embd)
        self.h = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layer))
        self.ln_f = FusedLayerNorm(cfg.n_embd)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # weight tying

        self.apply(self._init)
        for name, p in self.named_parameters():
            if name.endswith("c_proj.weight"):
                nn.init.normal_(p, std=0.02 / math.sqrt(2 * cfg.n_layer))

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=0.02)

    def forward(self, idx: torch.Tensor,
                targets: Optional[torch.Tensor] = None,
                doc_ids: Optional[torch.Tensor] = None,
                cache=None, extend: bool = False):
        """``doc_ids`` (integer [B, T], e.g. from ``document_ids``) marks
        the documents of packed rows: attention stays within a document
        and positions restart at each document's first token, so a
        packed document computes what it would compute alone.

        ``cache`` (a ``KVCache``, inference only): the first call with
        it is the prefill, an ordinary forward over ``idx`` [B, T] that
        also fills the cache and sets every row's length to ``T``; each
        later call takes one new token per row, ``idx`` [B, 1], at the
        rows' own positions ``cache.pos`` and returns its logits
        [B, 1, V].

        ``extend=True`` (needs a filled cache) appends ``idx`` [B, T],
        ``T >= 1``, to every row instead: token ``t`` of row ``b`` sits
        at position ``cache.pos[b] + t`` and attends the row's cache and
        the new tokens up to itself (ops/append_attn.py). The cache
        advances by ``T`` and the logits are [B, T, V]. Raises
        ``ValueError`` when ``cache.max_pos + T`` exceeds ``cache.Tmax``
        or ``n_positions``.

        Multi-turn recipe, for rows that append fewer than ``T`` real
        tokens: right-pad them to ``T``, call with ``extend=True``, read
        row ``b``'s logits at ``[:n_b]``, then ``cache.set_lengths(old_pos
        + n, max(old_pos + n))`` with the true counts ``n`` [B]. As in
        the prefill, the pad tokens sit after the real ones, so no real
        token attends them, and their cache slots lie at or above the
        row's new length: they are overwritten before they are ever
        attended.

        A model whose bf16 block weights were dropped
        (``quantize_weights_fp8(drop_bf16=True)``) is for inference only:
        in training mode the call raises ``RuntimeError``."""
        if self.training and self.weights_dropped():
            raise RuntimeError(
                "the blocks' bf16 weights were dropped "
                "(quantize_weights_fp8(drop_bf16=True)): the model runs in "
                "eval mode only")
        if targets is None and doc_ids is None and \
                self._fused_decode(idx, cache, extend):
            return self._decode_logits(idx, cache)[:, None], None
        x = self._hidden(idx, doc_ids, cache, extend)
        if targets is not None:
            # chunked LM-head + CE: never materializes the [B*T, V]
            # logits (ops/chunked_ce.py); identical numerics to
            # F.cross_entropy(logits.float(), t, ignore_index=,
            # label_smoothing=) + z_loss * mean(logsumexp^2)
            from ..ops.chunked_ce import chunked_cross_entropy
            loss = chunked_cross_entropy(
                x.reshape(-1, x.size(-1)), self.lm_head.weight,
                targets.reshape(-1),
                ignore_index=self.cfg.ignore_index,
                label_smoothing=self.cfg.label_smoothing,
                z_loss=self.cfg.z_loss)
            return None, loss
        return self.lm_head(x), None

    def _hidden(self, idx, doc_ids=None, cache=None, extend=False):
        """``ln_f`` of the last block's output, [B, T, C]: forward
        without the LM head."""
        B, T = idx.shape
        if extend:
            if cache is None or not cache.prefilled:
                raise ValueError("extend=True needs a filled cache")
            if T < 1:
                raise ValueError("extend=True needs T >= 1 tokens per row")
            if cache.max_pos + T > min(cache.Tmax, self.cfg.n_positions):
                raise ValueError(
                    f"{cache.max_pos} cached + {T} new tokens exceed the "
                    f"cache's {cache.Tmax} or the model's "
                    f"{self.cfg.n_positions} positions")
        decode = cache is not None and cache.prefilled and not extend
        if cache is not None:
            if doc_ids is not None:
                raise ValueError("doc_ids and cache do not combine")
            if decode and T != 1:
                raise ValueError(
                    f"a decode step takes one token per row, got T = {T}")
            # a decode step writes slot max_pos at the furthest, the
            # prefill slots 0 .. T-1
            if not extend and \
                    (cache.max_pos + 1 if decode else T) > cache.Tmax:
                raise ValueError(
                    f"the cache holds {cache.Tmax} positions per row")
        if extend:
            pos = cache.pos.to(torch.int64)[:, None] + \
                torch.arange(T, device=idx.device)
        elif decode:
            pos = cache.pos.to(torch.int64)[:, None]
        else:
            pos = torch.arange(T, device=idx.device)
        bounds = None
        if doc_ids is not None:
            # once per batch; every layer gets the pair
            from ..ops.flash_attn import doc_bounds
            if tuple(doc_ids.shape) != (B, T):
                raise ValueError(
                    f"doc_ids must have idx's shape {[B, T]}, got "
                    f"{list(doc_ids.shape)}")
            bounds = doc_bounds(doc_ids.to(idx.device))
            pos = pos[None, :] - bounds[0]
        x = self.wte(idx) + self.wpe(pos)
        # fused pre-norm chain: each residual add is folded into the
        # NEXT LayerNorm's forward (ops/fused_ln.py), crossing block
        # boundaries; h is always ln(x) of the current position.
        # Dropout rides in the same kernels: embedding dropout in the
        # first LayerNorm (its x_new becomes the residual stream),
        # residual dropout on each sublayer output as it is added.
        pe, pr = self.cfg.embd_pdrop, self.cfg.resid_pdrop
        if pe > 0.0:
            x, h = self.h[0].ln_1(x, dropout_p=pe)
        else:
            h = self.h[0].ln_1(x)
        for i, block in enumerate(self.h):
            if cache is None:
                attn_out = block.attn(h, bounds)
            else:
                attn_out = block.attn(
                    h, None, self._layer_cache(cache, i), extend)
            x, h = block.ln_2(attn_out, residual=x, dropout_p=pr)
            mlp_out = block.mlp(h)
            next_ln = (self.h[i + 1].ln_1 if i + 1 < len(self.h)
                       else self.ln_f)
            x, h = next_ln(mlp_out, residual=x, dropout_p=pr)
        if extend:
            cache.advance(T)
        elif decode:
            cache.advance()
        elif cache is not None:
            cache.set_lengths(
                torch.full((B,), T, dtype=torch.int32, device=idx.device),
                T)
        return h  # = ln_f(x)

    @staticmethod
    def _layer_cache(cache, i):
        """Layer ``i`` of ``cache`` as ``CausalSelfAttention.forward``
        takes it: with the scales when the cache is fp8."""
        if cache.k_scale is None:
            return (cache.k[i], cache.v[i], cache)
        return (cache.k[i], cache.v[i], cache, cache.k_scale[i],
                cache.v_scale[i])

    def _block_linears(self):
        for block in self.h:
            yield from (block.attn.c_attn, block.attn.c_proj,
                        block.mlp.c_fc, block.mlp.c_proj)

    def weights_dropped(self) -> bool:
        """Whether the blocks hold their linears as fp8 pairs only
        (``quantize_weights_fp8`` drops all of them or none, so the first
        block tells)."""
        return len(self.h) > 0 and linear_dropped(self.h[0].attn.c_attn)

    @torch.no_grad()
    def quantize_weights_fp8(self, drop_bf16: bool = False) -> "GPT2":
        """Weight-only fp8 for the four linears of every block, on a bf16
        model in eval mode: each bf16 ``weight`` is overwritten with its
        dequantized e4m3 values (exact in bf16), and the codes and row
        scales are kept next to it as non-persistent buffers
        ``weight_fp8`` / ``weight_scale``, so state dicts do not change.
        ``decode_layer`` streams the fp8 copy; the bf16 copy stays and
        serves prefill, ``extend`` and every other path, which compute the
        same function, so the blocks' weight memory grows by half. The
        embeddings and the LM head stay bf16. Call it again after the
        weights change; returns ``self``.

        ``drop_bf16=True`` frees the bf16 copies instead: each of those
        ``weight`` parameters becomes an empty bf16 [0, K], the pair
        becomes persistent buffers (a state dict still holds the model and
        loads strictly into another dropped model), and every path applies
        the linear through ``fp8_linear`` (ops/fp8_linear.py): ``N * K +
        4 * N`` bytes per linear where bf16 takes ``2 * N * K``. The model
        is then for inference only, and a second call raises
        ``RuntimeError``, the bf16 values being gone."""
        from ..ops.skinny_linear import dequantize_weight, quantize_weight
        if self.training or self.wte.weight.dtype != torch.bfloat16:
            raise RuntimeError(
                "quantize_weights_fp8 takes a bf16 model in eval mode")
        if self.weights_dropped():
            raise RuntimeError(
                "the blocks' bf16 weights were dropped: there is nothing "
                "to quantize again")
        for lin in self._block_linears():
            q, scale = quantize_weight(lin.weight)
            if drop_bf16:
                lin.weight = nn.Parameter(
                    lin.weight.new_empty(0, lin.weight.shape[1]),
                    requires_grad=False)
            else:
                lin.weight.copy_(dequantize_weight(q, scale))
            lin.register_buffer("weight_fp8", q, persistent=drop_bf16)
            lin.register_buffer("weight_scale", scale, persistent=drop_bf16)
        return self

    def _fused_decode(self, idx, cache, extend=False) -> bool:
        """Whether this call is a decode step that runs through
        ``decode_layer`` (ops/skinny_linear.py): one token per row over a
        filled cache, at most 64 rows, a bf16 model in eval mode, the
        gate on. On the GPU also only where the kernels take the model's
        linears (fp32 LayerNorm parameters, widths in 32s, the extension
        loaded): there the torch twin, which widens every weight matrix
        per call, would be slower than the composed path."""
        if cache is None or not cache.prefilled or extend or self.training \
                or len(self.h) == 0:
            return False
        if idx.dim() != 2 or idx.shape[1] != 1 or not 1 <= idx.shape[0] <= 64:
            return False
        from ..ops.skinny_linear import (fp8_enabled, kernel_enabled,
                                         kernel_serves)
        w = self.wte.weight
        if w.dtype != torch.bfloat16 or not kernel_enabled():
            return False
        b0 = self.h[0]
        # a dropped linear is judged by its fp8 matrix, the only one it
        # has; with RLA_SKINNY_FP8=0 such a model takes the composed route
        dropped = self.weights_dropped()
        if dropped and not fp8_enabled():
            return False

        def mat(lin):
            return lin.weight_fp8 if dropped else lin.weight

        return not w.is_cuda or (
            kernel_serves(mat(b0.attn.c_attn), b0.ln_1.weight)
            and kernel_serves(mat(b0.mlp.c_fc), b0.ln_2.weight)
            and kernel_serves(mat(b0.mlp.c_proj))
            and kernel_serves(self.lm_head.weight, self.ln_f.weight))

    def _decode_logits(self, idx, cache):
        """The logits [B, V] of one decode step over ``idx`` [B, 1]. On
        the fused path every block is one ``decode_layer`` call and the
        last residual add, ``ln_f`` and the LM head are one
        ``skinny_linear`` call; otherwise ``_hidden`` and the LM head."""
        if not self._fused_decode(idx, cache):
            return self.lm_head(self._hidden(idx, None, cache)[:, 0])
        from ..ops.skinny_linear import decode_layer, skinny_linear
        if cache.max_pos + 1 > cache.Tmax:
            raise ValueError(
                f"the cache holds {cache.Tmax} positions per row")
        x = self.wte(idx[:, 0]) + self.wpe(cache.pos.to(torch.int64))
        res = None
        ks, vs = cache.k_scale, cache.v_scale
        for i, block in enumerate(self.h):
            res, x = decode_layer(
                x, res, block.ln_1, block.attn.c_attn, cache.k[i],
                cache.v[i], cache.pos, cache.max_pos, block.attn.c_proj,
                block.ln_2, block.mlp.c_fc, block.mlp.c_proj,
                *(() if ks is None else (ks[i], vs[i])))
        logits, _ = skinny_linear(
            x, self.lm_head.weight, None, residual=res,
            ln_weight=self.ln_f.weight, ln_bias=self.ln_f.bias,
            eps=self.ln_f.eps)
        cache.advance()
        return logits

    @staticmethod
    def _sample(logits, temperature, top_k, generator):
        if temperature == 0:
            return logits.argmax(dim=-1)
        logits = logits / temperature
        if top_k is not None:
            kth = logits.topk(min(top_k, logits.size(-1)), dim=-1).values
            logits = logits.masked_fill(logits < kth[:, -1:], -math.inf)
        probs = torch.softmax(logits, dim=-1)
        return torch.multinomial(probs, 1, generator=generator)[:, 0]

    def _prefill_in_slices(self, prompt, c, cache, lens_dev, max_len,
                           pad_token_id):
        """The prompts into ``cache`` ``c`` positions at a time: the first
        slice through the prefill (padded up to the flash tile of 64, as
        the whole prompt is without slices), the others through
        ``extend``. After each slice the rows' lengths are put to what
        they really hold, so a row whose prompt has ended keeps its
        length while the others grow; what the slice wrote above it is
        overwritten before it is attended. Returns ``ln_f``'s output at
        each row's last prompt token, [B, C]."""
        B = prompt.shape[0]
        rows = torch.arange(B, device=prompt.device)
        last = lens_dev - 1

        def settle(done):
            cache.set_lengths(lens_dev.clamp(max=done).to(torch.int32),
                              min(max_len, done))

        c0 = min(c, max_len)
        c0_pad = min(-(-c0 // 64) * 64, prompt.shape[1])
        first = prompt[:, :c0_pad].clone()
        first[:, c0:] = pad_token_id
        h = self._hidden(first, None, cache)
        settle(c0)
        out = h[rows, last.clamp(max=c0 - 1)]
        for s in range(c0, max_len, c):
            n = min(c, max_len - s)
            h = self._hidden(prompt[:, s:s + n], None, cache, extend=True)
            settle(s + n)
            here = (last >= s) & (last < s + n)
            out = torch.where(here[:, None],
                              h[rows, (last - s).clamp(0, n - 1)], out)
        return out

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int, *,
                 prompt_lens=None, temperature: float = 1.0,
                 top_k: Optional[int] = None,
                 eos_token_id: Optional[int] = None,
                 pad_token_id: int = 0,
                 generator: Optional[torch.Generator] = None,
                 return_logits: bool = False,
                 prefill_chunk: Optional[int] = None,
                 top_p: Optional[float] = None, seed=None,
                 draft_tokens: int = 0, draft_ngram: int = 3,
                 return_stats: bool = False, kv_fp8: bool = False):
        """Sample ``max_new_tokens`` tokens per row after the prompts.

        ``idx`` [B, P] holds the prompts, right-padded; ``prompt_lens``
        (list or CPU tensor, default all ``P``) their true lengths.
        Returns tokens [B, P + max_new_tokens]: row ``b`` is its prompt,
        its new tokens from position ``prompt_lens[b]`` on, then
        ``pad_token_id``. Raises ``ValueError`` for a length outside
        ``[1, P]`` or when ``max(prompt_lens) + max_new_tokens`` exceeds
        ``n_positions``.

        ``temperature == 0`` is greedy; otherwise the logits are divided
        by ``temperature``, cut to the ``top_k`` largest when given, and
        sampled with ``torch.multinomial`` on ``generator``. A row that
        has emitted ``eos_token_id`` emits ``pad_token_id`` from then on.

        With ``seed`` or ``top_p`` given, every step's sampling, EOS
        handling and write into the result is one ``sample_tokens`` call
        (ops/sample.py: one HIP kernel on the GPU) on the LM head's
        logits as they are. ``top_p`` in (0, 1] keeps the nucleus of the
        ``top_k`` set. ``seed`` is an int (row ``b`` draws from the
        Philox stream ``seed + b``) or a sequence of ``B`` ints; step
        ``s`` of a row is counter ``s`` of its stream, so from equal
        logits a row draws the same tokens alone as in any batch.
        ``top_p`` without ``seed`` draws one seed from ``generator`` (or
        torch's default) at the start of the call.

        One prefill forward over the prompts (padded up to a multiple of
        64 positions so the flash kernels take it; the LM head runs on
        the ``B`` rows at ``prompt_lens - 1`` only) fills a KV cache;
        every later token costs one decode step over [B, 1]. Nothing is
        read back from the device per token: whether every row has
        finished is looked at once in 16 steps.

        ``return_logits=True`` also returns the fp32 logits every step
        sampled from, [B, max_new_tokens, V] (zero for steps after an
        early stop). That tensor is for tests and small vocabularies: at
        GPT-2's vocabulary it is 200 KB per row and step.

        ``prefill_chunk=c`` bounds the prefill's activation memory: the
        first ``c`` prompt positions go through the flash prefill, the
        rest in slices of ``c`` through ``extend`` over the cache. The LM
        head still runs on the ``B`` rows at ``prompt_lens - 1`` only.
        The default (``None``) is the single prefill forward.

        ``draft_tokens=T`` (1 to 15) is prompt-lookup speculative
        decoding: every step drafts ``T`` tokens per row by looking the
        row's last ``draft_ngram`` (1 to 8) tokens up in its own history,
        runs one ``extend`` forward over ``[last token, T drafts]`` and
        commits the accepted drafts plus one more token, all after the LM
        head in one ``spec_step`` call (ops/spec_decode.py: one HIP kernel
        on the GPU). Sampling is the seeded rule above with the number of
        tokens the row has emitted as the counter, so from equal logits
        the call returns what it returns with ``draft_tokens=0`` and the
        same ``seed``; a seed is drawn as for ``top_p`` when none is
        given. Three small integers per row (cache length, tokens
        emitted, finished) are read back per step, for the cache's bound
        and the end of the loop. Near the position limit
        the drafts shorten, down to none. ``return_logits`` does not
        combine with it. ``return_stats=True`` also returns ``{"forwards":
        extend forwards run, "committed": tokens they committed over all
        rows}`` (both 0 without drafts).

        ``kv_fp8=True`` keeps the KV cache as float8_e4m3fn codes with one
        power-of-two scale per head and position (ops/decode_attn.py): 136
        bytes where bf16 takes 256, read by the fp8 decode-attention kernel
        and filled by ``kv_cache_fill`` after the prefill. Every token
        attends the dequantized values, its own included. It needs a bf16
        model with head size 64 (``ValueError`` otherwise); ``prefill_chunk``
        and ``draft_tokens`` run the append kernel's fp8 variant over it
        (ops/append_attn.py).

        Runs without gradients, in eval mode; the module's mode is put
        back afterwards."""
        from ..ops.decode_attn import KVCache, decode_attn_chunk
        cfg = self.cfg
        if kv_fp8 and (self.wte.weight.dtype != torch.bfloat16
                       or cfg.n_embd // cfg.n_head != 64):
            raise ValueError(
                "kv_fp8 needs a bf16 model with head size 64")
        if idx.dim() != 2:
            raise ValueError("idx must be [B, P]")
        B, P = idx.shape
        if max_new_tokens < 0:
            raise ValueError("max_new_tokens must be >= 0")
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError("prefill_chunk must be >= 1")
        spec = draft_tokens != 0
        if spec:
            if not 1 <= draft_tokens <= 15:
                raise ValueError("draft_tokens must be in [0, 15]")
            if not 1 <= draft_ngram <= 8:
                raise ValueError("draft_ngram must be in [1, 8]")
            if return_logits:
                raise ValueError(
                    "draft_tokens and return_logits do not combine")
        fused = spec or seed is not None or top_p is not None
        if top_p is not None and not 0 < top_p <= 1:
            raise ValueError("top_p must be in (0, 1]")
        if fused:
            if seed is None:
                seed = int(torch.randint(
                    0, 2 ** 62, (1,), generator=generator,
                    device=None if generator is None else generator.device))
            row_seeds = [seed + b for b in range(B)] \
                if isinstance(seed, int) else [int(s) for s in seed]
            if len(row_seeds) != B:
                raise ValueError(f"seed must be an int or {B} ints")
            # into int64, as two's complement
            row_seeds = [(s + 2 ** 63) % 2 ** 64 - 2 ** 63
                         for s in row_seeds]
        if prompt_lens is None:
            lens = [P] * B
        else:
            lens = [int(n) for n in (prompt_lens.tolist() if isinstance(
                prompt_lens, torch.Tensor) else prompt_lens)]
        if len(lens) != B or not all(1 <= n <= P for n in lens):
            raise ValueError(
                f"prompt_lens must hold {B} lengths in [1, {P}], got {lens}")
        max_len = max(lens)
        if max_len + max_new_tokens > cfg.n_positions:
            raise ValueError(
                f"max(prompt_lens) + max_new_tokens = "
                f"{max_len + max_new_tokens} exceeds n_positions = "
                f"{cfg.n_positions}")
        dev = idx.device
        lens_dev = torch.tensor(lens, dtype=torch.int64, device=dev)
        out = torch.full((B, P + max_new_tokens), pad_token_id,
                         dtype=torch.int64 if fused else idx.dtype,
                         device=dev)
        in_prompt = torch.arange(P, device=dev)[None, :] < lens_dev[:, None]
        out[:, :P] = torch.where(in_prompt, idx, out[:, :P])
        V = cfg.vocab_size
        all_logits = torch.zeros(B, max_new_tokens, V, dtype=torch.float32,
                                 device=dev) if return_logits else None
        stats = {"forwards": 0, "committed": 0}
        if max_new_tokens == 0:
            out = out.to(idx.dtype)
            if return_stats:
                return (out, all_logits, stats) if return_logits \
                    else (out, stats)
            return (out, all_logits) if return_logits else out

        was_training = self.training
        self.eval()
        try:
            # prefill: padding sits after the real tokens, so under
            # causal attention it cannot reach them
            P_pad = min(-(-P // 64) * 64, max(cfg.n_positions, P))
            prompt = out.new_full((B, P_pad), pad_token_id)
            prompt[:, :P] = out[:, :P]
            cache = None
            if max_new_tokens > 1 or prefill_chunk is not None:
                chunk = decode_attn_chunk()
                Tmax = -(-(max_len + max_new_tokens) // chunk) * chunk
                Tmax = max(min(Tmax, cfg.n_positions), P_pad)
                p0 = self.wte.weight
                cache = KVCache(cfg.n_layer, B, cfg.n_head, Tmax,
                                cfg.n_embd // cfg.n_head,
                                torch.float8_e4m3fn if kv_fp8 else p0.dtype,
                                dev)
            rows = torch.arange(B, device=dev)
            if prefill_chunk is None:
                h = self._hidden(prompt, None, cache)
                if cache is not None:
                    # pad positions in the cache are overwritten as the
                    # row grows, and never attended before that
                    cache.set_lengths(lens_dev.to(torch.int32), max_len)
                h = h[rows, lens_dev - 1]
            else:
                h = self._prefill_in_slices(prompt, prefill_chunk, cache,
                                            lens_dev, max_len, pad_token_id)
            logits = self.lm_head(h)
            if not fused:
                logits = logits.float()

            finished = torch.zeros(B, dtype=torch.bool, device=dev)
            if fused:
                from ..ops.sample import sample_tokens
                seeds = torch.tensor(row_seeds, dtype=torch.int64,
                                     device=dev)
                col = lens_dev.clone()
            if spec:
                self._generate_drafted(
                    logits, cache, seeds, col, finished, out,
                    max_new_tokens, draft_tokens, draft_ngram, stats,
                    dict(temperature=temperature, top_k=top_k, top_p=top_p,
                         eos=eos_token_id, pad=pad_token_id))
            for step in range(0 if spec else max_new_tokens):
                if return_logits:
                    all_logits[:, step] = logits
                if fused:
                    tok = sample_tokens(
                        logits.contiguous(), seeds, step,
                        temperature=temperature, top_k=top_k, top_p=top_p,
                        finished=finished, eos=eos_token_id,
                        pad=pad_token_id, out=out, col=col)
                    col += 1
                else:
                    tok = self._sample(logits, temperature, top_k,
                                       generator)
                    if eos_token_id is not None:
                        tok = torch.where(finished,
                                          tok.new_tensor(pad_token_id), tok)
                        finished = finished | (tok == eos_token_id)
                    out.scatter_(1, (lens_dev + step)[:, None],
                                 tok[:, None].to(out.dtype))
                if step + 1 == max_new_tokens:
                    break
                if (eos_token_id is not None and step % 16 == 15
                        and bool(finished.all())):
                    break
                logits = self._decode_logits(tok[:, None], cache)
                if not fused:
                    logits = logits.float()
        finally:
            self.train(was_training)
        out = out.to(idx.dtype)
        if return_stats:
            return (out, all_logits, stats) if return_logits \
                else (out, stats)
        return (out, all_logits) if return_logits else out

    def _generate_drafted(self, logits, cache, seeds, col, finished, out,
                          limit, T, ngram, stats, kw):
        """The loop of ``generate(draft_tokens=T)`` after the prefill.
        ``logits`` [B, V] are the prefill's; ``col`` [B] is where each
        row's next token goes in ``out``. After every ``spec_step`` a
        row's cache holds all its tokens but the last one committed:
        ``pos == col - 1``. The first call has ``T1 = 1`` and follows no
        ``advance``; its ``pos += n - T1`` adds 0, since ``limit >= 1``
        gives ``n = 1``, and the prefill left ``pos = col``."""
        from ..ops.spec_decode import spec_step
        B, dev = logits.shape[0], logits.device
        emitted = torch.zeros(B, dtype=torch.int64, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev)
        # max_new_tokens == 1 runs without a cache
        pos = cache.pos if cache is not None else \
            torch.zeros(B, dtype=torch.int32, device=dev)
        room = 0 if cache is None else \
            min(cache.Tmax, self.cfg.n_positions)
        state = dict(finished=finished, out=out, col=col, pos=pos, done=done,
                     ngram=ngram, **kw)
        _, _, next_idx = spec_step(
            logits[:, None].contiguous(), out.new_empty(B, 0), seeds,
            emitted, limit, next_T=T if limit > 1 else 0, **state)
        while True:
            host = torch.stack((pos.to(torch.int64), emitted,
                                finished.to(torch.int64))).tolist()
            stats["committed"] = sum(host[1]) - B
            if all(e == limit or f for e, f in zip(host[1], host[2])):
                return
            cache.set_max_pos(max(host[0]))
            Tn = min(T, room - cache.max_pos - 1)
            h = self._hidden(next_idx[:, :1 + Tn], None, cache, extend=True)
            _, _, next_idx = spec_step(
                self.lm_head(h), next_idx[:, 1:1 + Tn], seeds, emitted,
                limit, next_T=T, **state)
            stats["forwards"] += 1

def document_ids(idx: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """Document ids [B, T] of a packed token stream: the number of EOS
    tokens strictly before each position, so an EOS token belongs to the
    document it ends and the next token opens a new one."""
    eos = (idx == eos_token_id).to(torch.int64)
    return eos.cumsum(dim=1) - eos


def to_bf16_training(model: nn.Module) -> nn.Module:
    """bf16 weights with fp32 normalization params: the fused LN/BN
    kernels keep their statistics math and affine params in fp32 (the
    numerically sane split, and what engages the fused HIP path)."""
    model = model.to(torch.bfloat16)
    for m in model.modules():
        if isinstance(m, (nn.LayerNorm,)):
            m.float()
    return model


def gpt2_xl() -> GPT2:
    return GPT2(GPT2Config.gpt2_xl())
