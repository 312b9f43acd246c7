"""Prompt-lookup speculative decoding (ops/spec_decode.py) measured three
ways; profiles/spec_decode.md holds the results. One process, contestants
alternating, five samples each, median with min-max, host clock around a
device synchronise.

(a) op: spec_step (one launch) against sample_tokens on the B * T1 rows
    plus the commit and draft twin on the host. B = 8, V = 50257, bf16.
(b) step: GPT-2-XL (random init), B = 8, about 256 cached tokens: one
    speculative step (extend forward, LM head, spec_step, read-back) for
    T in {3, 7, 15} against the plain decode step (forward, LM head,
    sample_tokens). The break-even is the ratio of the two: the mean
    number of tokens a speculative step must commit to pay for itself.
(c) end to end: generate() with and without drafts on a periodic and on
    a random prompt, greedy. Random weights make acceptance
    unrepresentative: these are the two extremes, (b) is what transfers.

    python scripts/bench_spec_decode.py [--parts abc] [--model xl|tiny]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,  # noqa: E402
                                           to_bf16_training)
from ray_lightning_amd.ops import spec_decode as sd  # noqa: E402
from ray_lightning_amd.ops.decode_attn import KVCache  # noqa: E402
from ray_lightning_amd.ops.sample import sample_tokens  # noqa: E402

B = 8
DEV = "cuda"
KW = dict(temperature=1.0, top_k=50, top_p=0.9)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def contest(fns, calls, unit=1e6):
    """{name: (median, min, max)} of five alternating samples."""
    for fn in fns.values():
        timed(fn, max(2, calls // 4))
    got = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            got[k].append(timed(fn, calls) * unit)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def show(tag, res, unit):
    print(tag + ": " + "  ".join(
        f"{k} {m:.1f} {unit} [{lo:.1f}, {hi:.1f}]"
        for k, (m, lo, hi) in res.items()), flush=True)


def state(T1, L, hist):
    i64 = dict(dtype=torch.int64, device=DEV)
    out = torch.randint(0, 50, (B, L), **i64)
    return dict(finished=torch.zeros(B, dtype=torch.bool, device=DEV),
                out=out, col=torch.full((B,), hist, **i64),
                pos=torch.full((B,), hist, dtype=torch.int32, device=DEV),
                done=torch.zeros(B, dtype=torch.int32, device=DEV))


def part_a(calls):
    V, L, hist = 50257, 1024, 300
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    for T1 in (4, 8, 16):
        logits = (4 * torch.randn(B, T1, V, device=DEV)).to(torch.bfloat16)
        draft = torch.randint(0, V, (B, T1 - 1), device=DEV)
        st = [state(T1, L, hist) for _ in range(2)]
        em = [torch.zeros(B, dtype=torch.int64, device=DEV)
              for _ in range(2)]
        rep = seeds.repeat_interleave(T1)

        def reset(s, e):  # the history stays at hist tokens
            s["col"].fill_(hist)
            e.zero_()

        def kernel(i):
            reset(st[0], em[0])
            sd.spec_step(logits, draft, seeds, em[0], 1 << 40, ngram=3,
                         next_T=T1 - 1, **st[0], **KW)

        def chain(i):
            reset(st[1], em[1])
            tok = sample_tokens(logits.view(B * T1, V), rep, i, **KW)
            s = {k: v for k, v in st[1].items() if k != "done"}
            sd.commit_and_draft(tok.view(B, T1), draft, em[1], 1 << 40,
                                eos=-1, pad=0, ngram=3, next_T=T1 - 1, **s)

        show(f"(a) T1={T1}", contest(dict(spec_step=kernel,
                                          sample_plus_twin=chain), calls),
             "us")


def build(model):
    cfg = GPT2Config.gpt2_xl() if model == "xl" else GPT2Config(
        n_layer=2, n_embd=128, n_head=2, vocab_size=256, n_positions=512)
    torch.manual_seed(0)
    return to_bf16_training(GPT2(cfg)).to(DEV).eval()


@torch.no_grad()
def part_b(m, calls):
    cfg, hist = m.cfg, 256
    V = cfg.vocab_size
    cache = KVCache(cfg.n_layer, B, cfg.n_head, 512,
                    cfg.n_embd // cfg.n_head, m.wte.weight.dtype, DEV)
    m._hidden(torch.randint(0, V, (B, hist), device=DEV), None, cache)
    lens = torch.full((B,), hist, dtype=torch.int32, device=DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    tok = torch.randint(0, V, (B, 1), device=DEV)
    fns = {}

    # every step of either kind leaves one more token in the cache, so a
    # window of `calls` steps runs at hist .. hist + calls cached tokens
    def plain(i):
        if i == 0:
            cache.set_lengths(lens, hist)
        h = m._hidden(tok, None, cache)
        sample_tokens(m.lm_head(h[:, 0]).contiguous(), seeds, i, **KW)

    fns["plain"] = plain
    for T in (3, 7, 15):
        st = state(T + 1, 1024, hist)
        st["pos"] = cache.pos
        em = torch.zeros(B, dtype=torch.int64, device=DEV)
        nxt = [torch.randint(0, V, (B, T + 1), device=DEV)]

        def spec(i, T=T, st=st, em=em, nxt=nxt):
            if i == 0:
                cache.set_lengths(lens, hist)
                st["col"].fill_(hist + 1)
            h = m._hidden(nxt[0], None, cache, extend=True)
            _, _, nxt[0] = sd.spec_step(
                m.lm_head(h), nxt[0][:, 1:], seeds, em, 1 << 40, ngram=3,
                next_T=T, **st, **KW)
            host = torch.stack((cache.pos.to(torch.int64), em,
                                st["finished"].to(torch.int64))).tolist()
            cache.set_max_pos(max(host[0]))

        fns[f"T={T}"] = spec
    with torch.no_grad():
        res = contest(fns, calls, unit=1e3)
    show("(b) step", res, "ms")
    for k, v in res.items():
        if k != "plain":
            print(f"(b) break-even {k}: {v[0] / res['plain'][0]:.2f} "
                  "committed tokens per step", flush=True)


def part_c(m, new):
    V = m.cfg.vocab_size
    g = torch.Generator().manual_seed(0)
    prompts = dict(
        periodic=torch.randint(0, V, (B, 8), generator=g).repeat(1, 8),
        random=torch.randint(0, V, (B, 64), generator=g))
    for name, idx in prompts.items():
        idx = idx.to(DEV)
        stats = {}

        def run(T):
            def fn(i):
                out = m.generate(idx, new, temperature=0.0, seed=1,
                                 draft_tokens=T, return_stats=True)
                stats[T] = out[1]
            return fn

        res = contest({"plain": run(0), "T=7": run(7)}, 1, unit=1.0)
        res = {k: tuple(B * new / x for x in (m_, hi, lo))
               for k, (m_, lo, hi) in res.items()}
        show(f"(c) {name} prompt", res, "tok/s")
        s = stats[7]
        print(f"(c) {name}: {s['forwards']} forwards, "
              f"{s['committed'] / max(1, s['forwards']) / B:.2f} committed "
              "tokens per row and step", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--model", default="xl", choices=["xl", "tiny"])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--new", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if "a" in args.parts:
        part_a(args.calls)
    if "b" in args.parts or "c" in args.parts:
        m = build(args.model)
        if "b" in args.parts:
            part_b(m, args.steps)
        if "c" in args.parts:
            part_c(m, args.new)


if __name__ == "__main__":
    main()
