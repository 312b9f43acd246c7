"""Measure the MFMA split-KV append attention kernel and
GPT2.forward(extend=True) on one GPU. Fails without a GPU and the built
extension.

(a) Kernel against its two incumbents, B=8, H=25, hs=64, bf16,
    Tmax=1024, pos in {128, 512, 960} (every row at the same pos),
    T in {4, 16, 64}:

      kernel   append_attention's HIP path: partial kernel with the
               append of the T rows, and the combine kernel
      sdpa     index_copy_ of the T new k and v rows into the caches,
               then F.scaled_dot_product_attention(q[B,H,T,64],
               k[:, :, :pos+T], v[:, :, :pos+T]) with the boolean mask
      decode   T successive decode_attention kernel calls, token t at
               pos + t (its inputs sliced and its pos tensors made
               outside the timed loop)

    All run on the same caches. A model step visits one cache per layer,
    so the timed loop walks a ring of 48 cache pairs (GPT-2-XL's layer
    count) rather than re-reading one pair that would sit in the
    Infinity Cache. Contestants alternate in one process; each sample is
    device-event time over enough calls to fill --window seconds; median
    of --rounds, and the spread is max - min of those samples.

    Rule, fixed before the run: _APPEND_DEFAULT = True iff at all nine
    points the kernel's median is below each incumbent's by more than
    the larger of the two spreads.

(b) End to end: gpt2-xl, bf16, B=8, 512 cached tokens, a 64-token turn.
    Time to the last token's logits by extend (kernel, and the twin),
    by re-running the 576-token prefill into a fresh cache, and by 64
    decode steps.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402

LAYERS = 48


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def med(t):
    return {"median_us": 1e3 * statistics.median(t), "min_us": 1e3 * min(t),
            "max_us": 1e3 * max(t), "spread_us": 1e3 * (max(t) - min(t))}


def kernel_point(ext, B, H, Tmax, pos, T, window, rounds):
    hs = 64
    scale = 1.0 / math.sqrt(hs)
    g = torch.Generator(device="cuda").manual_seed(pos + T)
    qkv = torch.randn(B, T, 3 * H * hs, device="cuda",
                      generator=g).bfloat16()
    ring = [(torch.randn(B, H, Tmax, hs, device="cuda",
                         generator=g).bfloat16(),
             torch.randn(B, H, Tmax, hs, device="cuda",
                         generator=g).bfloat16()) for _ in range(LAYERS)]
    pos_t = torch.full((B,), pos, dtype=torch.int32, device="cuda")
    slots = torch.arange(pos, pos + T, device="cuda")
    q, k, v = (x.transpose(1, 2)
               for x in qkv.view(B, T, 3, H, hs).unbind(2))
    mask = torch.arange(pos + T, device="cuda")[None, :] <= slots[:, None]
    step_qkv = [qkv[:, t].contiguous() for t in range(T)]
    step_pos = [pos_t + t for t in range(T)]

    def kernel(i):
        kc, vc = ring[i % LAYERS]
        return ext.append_attn_fwd(qkv, kc, vc, pos_t, pos, scale)

    def sdpa(i):
        kc, vc = ring[i % LAYERS]
        kc.index_copy_(2, slots, k)
        vc.index_copy_(2, slots, v)
        o = F.scaled_dot_product_attention(
            q, kc[:, :, :pos + T], vc[:, :, :pos + T], attn_mask=mask)
        return o.transpose(1, 2).reshape(B, T, H * hs)

    def decode(i):
        kc, vc = ring[i % LAYERS]
        return torch.stack(
            [ext.decode_attn_fwd(step_qkv[t], kc, vc, step_pos[t], pos + t,
                                 scale) for t in range(T)], dim=1)

    fns = {"kernel": kernel, "sdpa": sdpa, "decode": decode}
    ref = sdpa(0).float()
    diffs = {n: (fns[n](0).float() - ref).abs().max().item()
             for n in ("kernel", "decode")}
    iters = {}
    for name, fn in fns.items():
        for i in range(LAYERS):
            fn(i)
        torch.cuda.synchronize()
        per_ms = timed(fn, LAYERS)
        n = int(window * 1e3 / per_ms) + 1
        iters[name] = -(-n // LAYERS) * LAYERS
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, iters[name]))
    res = {"B": B, "pos": pos, "T": T, "max_abs_diff_vs_sdpa": diffs,
           "iters": iters}
    for name, t in times.items():
        res[name] = med(t)
    res["kernel_wins"] = all(
        res[n]["median_us"] - res["kernel"]["median_us"] >
        max(res[n]["spread_us"], res["kernel"]["spread_us"])
        for n in ("sdpa", "decode"))
    return res


def end_to_end(rounds):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    from ray_lightning_amd.ops.decode_attn import KVCache
    B, P, TURN = 8, 512, 64
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = GPT2(GPT2Config.gpt2_xl())
    model = to_bf16_training(model).eval()
    cfg = model.cfg
    idx = torch.randint(0, cfg.vocab_size, (B, P + TURN), device="cuda")
    full = torch.full((B,), P, dtype=torch.int32, device="cuda")

    def new_cache():
        return KVCache(cfg.n_layer, B, cfg.n_head, 1024,
                       cfg.n_embd // cfg.n_head, torch.bfloat16, "cuda")

    cache = new_cache()
    scratch = new_cache()
    with torch.no_grad():
        model._hidden(idx[:, :P], None, cache)

    def last_logits(h):
        return model.lm_head(h[:, -1]).float()

    def extend(gate):
        def run():
            os.environ["RLA_APPEND_ATTN"] = gate
            cache.set_lengths(full, P)
            return last_logits(model._hidden(idx[:, P:], None, cache, True))
        return run

    def prefill_again():
        scratch.prefilled = False
        return last_logits(model._hidden(idx, None, scratch))

    def decode_steps():
        cache.set_lengths(full, P)
        for t in range(TURN):
            h = model._hidden(idx[:, P + t:P + t + 1], None, cache)
        return last_logits(h)

    runs = {"extend_kernel": extend("1"), "extend_twin": extend("0"),
            "prefill_576": prefill_again, "decode_64_steps": decode_steps}
    outs, times = {}, {name: [] for name in runs}
    with torch.no_grad():
        for name, fn in runs.items():      # warm-up, every shape
            outs[name] = fn()
        for _ in range(rounds):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    res = {"B": B, "cached": P, "turn": TURN, "model": "gpt2-xl"}
    for name, t in times.items():
        res[name] = {"median_ms": 1e3 * statistics.median(t),
                     "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                     "last_logits_max_abs_diff_vs_prefill": (
                         outs[name] - outs["prefill_576"]).abs().max().item()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25,
                    help="seconds of device time per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-end-to-end", action="store_true")
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "append_attn_fwd"):
        sys.exit("bench_append_attn needs a GPU and the built HIP extension")

    points = []
    for pos in (128, 512, 960):
        for T in (4, 16, 64):
            r = kernel_point(ext, 8, 25, 1024, pos, T, args.window,
                             args.rounds)
            points.append(r)
            print(f"# pos={pos} T={T}: " + "  ".join(
                f"{n} {r[n]['median_us']:.1f}us (+-{r[n]['spread_us']:.1f})"
                for n in ("kernel", "sdpa", "decode"))
                + f"  wins={r['kernel_wins']}", flush=True)
    out = {"chunk": int(ext.append_attn_chunk()), "kernel": points,
           "default_on": all(r["kernel_wins"] for r in points),
           "rounds": args.rounds, "window_s": args.window,
           "hip": torch.version.hip}
    if not args.skip_end_to_end:
        out["end_to_end"] = end_to_end(args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
