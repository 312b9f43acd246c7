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
cache=...)`` is the same machinery one call at a time.
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


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.n_head = cfg.n_head
        self.attn_pdrop = cfg.attn_pdrop
        self.c_attn = nn.Linear(cfg.n_embd, 3 * cfg.n_embd)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd)

    def forward(self, x, doc_ids=None, cache=None):
        """``cache`` is this layer's ``(k_cache, v_cache, kv)`` of a
        ``KVCache`` ``kv``. Before the prefill the call attends as it
        does without a cache and copies its k and v into the caches at
        ``[:, :, :T]``; after it, ``x`` is one new token per row and
        attention is ``decode_attention`` over the cache."""
        B, T, C = x.shape
        qkv = self.c_attn(x)
        if cache is not None and cache[2].prefilled:
            from ..ops.decode_attn import decode_attention
            k_cache, v_cache, kv = cache
            y = decode_attention(qkv.view(B, 3 * C), k_cache, v_cache,
                                 kv.pos, kv.max_pos, self.n_head)
            return self.c_proj(y.view(B, 1, C))
        q, k, v = qkv.split(C, dim=2)
        hs = C // self.n_head
        q = q.view(B, T, self.n_head, hs).transpose(1, 2)
        k = k.view(B, T, self.n_head, hs).transpose(1, 2)
        v = v.view(B, T, self.n_head, hs).transpose(1, 2)
        if cache is not None:
            cache[0][:, :, :T].copy_(k)
            cache[1][:, :, :T].copy_(v)
        # hand-written MFMA flash kernels when the shape qualifies
        # (causal bf16 hs=64), attention dropout and document masking
        # (doc_ids: ids [B, T] or the doc_bounds pair) included; SDPA
        # (AOTriton) otherwise
        from ..ops.flash_attn import flash_attention
        y = flash_attention(
            q, k, v, dropout_p=self.attn_pdrop if self.training else 0.0,
            doc_ids=doc_ids)
        y = y.transpose(1, 2).contiguous().view(B, T, C)
        return self.c_proj(y)


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
                cache=None):
        """``doc_ids`` (integer [B, T], e.g. from ``document_ids``) marks
        the documents of packed rows: attention stays within a document
        and positions restart at each document's first token, so a
        packed document computes what it would compute alone.

        ``cache`` (a ``KVCache``, inference only): the first call with
        it is the prefill, an ordinary forward over ``idx`` [B, T] that
        also fills the cache and sets every row's length to ``T``; each
        later call takes one new token per row, ``idx`` [B, 1], at the
        rows' own positions ``cache.pos`` and returns its logits
        [B, 1, V]."""
        x = self._hidden(idx, doc_ids, cache)
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

    def _hidden(self, idx, doc_ids=None, cache=None):
        """``ln_f`` of the last block's output, [B, T, C]: forward
        without the LM head."""
        B, T = idx.shape
        decode = cache is not None and cache.prefilled
        if cache is not None:
            if doc_ids is not None:
                raise ValueError("doc_ids and cache do not combine")
            if decode and T != 1:
                raise ValueError(
                    f"a decode step takes one token per row, got T = {T}")
            # a decode step writes slot max_pos at the furthest, the
            # prefill slots 0 .. T-1
            if (cache.max_pos + 1 if decode else T) > cache.Tmax:
                raise ValueError(
                    f"the cache holds {cache.Tmax} positions per row")
        if decode:
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
                    h, None, (cache.k[i], cache.v[i], cache))
            x, h = block.ln_2(attn_out, residual=x, dropout_p=pr)
            mlp_out = block.mlp(h)
            next_ln = (self.h[i + 1].ln_1 if i + 1 < len(self.h)
                       else self.ln_f)
            x, h = next_ln(mlp_out, residual=x, dropout_p=pr)
        if decode:
            cache.advance()
        elif cache is not None:
            cache.set_lengths(
                torch.full((B,), T, dtype=torch.int32, device=idx.device),
                T)
        return h  # = ln_f(x)

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

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int, *,
                 prompt_lens=None, temperature: float = 1.0,
                 top_k: Optional[int] = None,
                 eos_token_id: Optional[int] = None,
                 pad_token_id: int = 0,
                 generator: Optional[torch.Generator] = None,
                 return_logits: bool = False):
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

        Runs without gradients, in eval mode; the module's mode is put
        back afterwards."""
        from ..ops.decode_attn import KVCache, decode_attn_chunk
        cfg = self.cfg
        if idx.dim() != 2:
            raise ValueError("idx must be [B, P]")
        B, P = idx.shape
        if max_new_tokens < 0:
            raise ValueError("max_new_tokens must be >= 0")
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
                         dtype=idx.dtype, device=dev)
        in_prompt = torch.arange(P, device=dev)[None, :] < lens_dev[:, None]
        out[:, :P] = torch.where(in_prompt, idx, out[:, :P])
        V = cfg.vocab_size
        all_logits = torch.zeros(B, max_new_tokens, V, dtype=torch.float32,
                                 device=dev) if return_logits else None
        if max_new_tokens == 0:
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
            if max_new_tokens > 1:
                chunk = decode_attn_chunk()
                Tmax = -(-(max_len + max_new_tokens) // chunk) * chunk
                Tmax = max(min(Tmax, cfg.n_positions), P_pad)
                p0 = self.wte.weight
                cache = KVCache(cfg.n_layer, B, cfg.n_head, Tmax,
                                cfg.n_embd // cfg.n_head, p0.dtype, dev)
            h = self._hidden(prompt, None, cache)
            if cache is not None:
                # pad positions in the cache are overwritten as the row
                # grows, and never attended before that
                cache.set_lengths(lens_dev.to(torch.int32), max_len)
            h = h[torch.arange(B, device=dev), lens_dev - 1]
            logits = self.lm_head(h).float()

            finished = torch.zeros(B, dtype=torch.bool, device=dev)
            for step in range(max_new_tokens):
                if return_logits:
                    all_logits[:, step] = logits
                tok = self._sample(logits, temperature, top_k, generator)
                if eos_token_id is not None:
                    tok = torch.where(finished, tok.new_tensor(pad_token_id),
                                      tok)
                    finished = finished | (tok == eos_token_id)
                out.scatter_(1, (lens_dev + step)[:, None],
                             tok[:, None].to(out.dtype))
                if step + 1 == max_new_tokens:
                    break
                if (eos_token_id is not None and step % 16 == 15
                        and bool(finished.all())):
                    break
                h = self._hidden(tok[:, None], None, cache)
                logits = self.lm_head(h[:, 0]).float()
        finally:
            self.train(was_training)
        return (out, all_logits) if return_logits else out

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
