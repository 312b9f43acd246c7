"""Measure the split-KV decode attention kernel and generation with the
KV cache on one GPU. Fails without a GPU and the built extension.

(a) Kernel against its incumbent, H=25, hs=64, bf16, Tmax=1024,
    B in {1, 8}, pos in {127, 511, 1023} (every row at the same pos):

      kernel   decode_attention's HIP path, append and combine included,
               at the built-in CHUNK and, through the measurement entry
               point, at 64 / 128 / 256
      sdpa     index_copy_ of the new k and v into the caches, then
               F.scaled_dot_product_attention(q[B,H,1,64],
               k[:, :, :pos+1], v[:, :, :pos+1])

    Both run on the same caches. A generation step visits one cache per
    layer, so the timed loop walks a ring of 48 cache pairs (GPT-2-XL's
    layer count) rather than re-reading one pair that would sit in the
    Infinity Cache. The bytes of a call are 2*(pos+1)*64*2 per (b, h);
    bytes/s is given as a share of the 6.29 TB/s measured and the 8 TB/s
    peak HBM figures. Where the ring's read footprint (in the output) is
    under 256 MiB the reads may be served by the Infinity Cache, as they
    would be in a real generation of that size.

    Contestants alternate in one process; each sample is device-event
    time over enough calls to fill --window seconds; median of 5.

    Rule, fixed before the run: _DECODE_DEFAULT = True iff the kernel's
    median beats sdpa's at all three lengths for B=8.

(b) End to end: gpt2-xl, bf16, B=8, prompt 128, 128 new tokens, greedy.
    tokens/s with cache + kernel, cache + SDPA twin, and a full forward
    per token over the growing sequence (the only way before the cache);
    prefill time (generate with one new token) and decode time per token.
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

HBM_MEASURED = 6.29e12
HBM_PEAK = 8.0e12
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
            "max_us": 1e3 * max(t)}


def kernel_point(ext, B, H, Tmax, pos, window, rounds):
    hs = 64
    scale = 1.0 / math.sqrt(hs)
    g = torch.Generator(device="cuda").manual_seed(pos + B)
    qkv = torch.randn(B, 3 * H * hs, device="cuda", generator=g).bfloat16()
    ring = [(torch.randn(B, H, Tmax, hs, device="cuda",
                         generator=g).bfloat16(),
             torch.randn(B, H, Tmax, hs, device="cuda",
                         generator=g).bfloat16()) for _ in range(LAYERS)]
    pos_t = torch.full((B,), pos, dtype=torch.int32, device="cuda")
    slot = torch.tensor([pos], device="cuda")
    q4 = qkv.view(B, 3, H, hs)

    def kernel(i):
        kc, vc = ring[i % LAYERS]
        return ext.decode_attn_fwd(qkv, kc, vc, pos_t, pos, scale)

    def at_chunk(chunk):
        def run(i):
            kc, vc = ring[i % LAYERS]
            return ext.decode_attn_fwd_at_chunk(qkv, kc, vc, pos_t, pos,
                                                scale, chunk)
        return run

    def sdpa(i):
        kc, vc = ring[i % LAYERS]
        kc.index_copy_(2, slot, q4[:, 1].unsqueeze(2))
        vc.index_copy_(2, slot, q4[:, 2].unsqueeze(2))
        o = F.scaled_dot_product_attention(
            q4[:, 0].unsqueeze(2), kc[:, :, :pos + 1], vc[:, :, :pos + 1])
        return o.transpose(1, 2).reshape(B, H * hs)

    fns = {"kernel": kernel, "sdpa": sdpa, "chunk64": at_chunk(64),
           "chunk128": at_chunk(128), "chunk256": at_chunk(256)}
    diff = (kernel(0).float() - sdpa(0).float()).abs().max().item()
    iters = {}
    for name, fn in fns.items():
        for i in range(2 * LAYERS):
            fn(i)
        torch.cuda.synchronize()
        per_ms = timed(fn, 4 * LAYERS)
        n = int(window * 1e3 / per_ms) + 1
        iters[name] = -(-n // LAYERS) * LAYERS
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, iters[name]))
    nbytes = 2 * (pos + 1) * hs * 2 * B * H
    res = {"B": B, "pos": pos, "bytes": nbytes,
           "ring_read_footprint_MiB": LAYERS * nbytes / 2 ** 20,
           "kernel_vs_sdpa_max_abs_diff": diff, "iters": iters}
    for name, t in times.items():
        r = med(t)
        rate = nbytes / (r["median_us"] * 1e-6)
        r["TB_per_s"] = rate / 1e12
        r["share_of_measured_hbm"] = rate / HBM_MEASURED
        r["share_of_peak_hbm"] = rate / HBM_PEAK
        res[name] = r
    res["kernel_wins"] = (res["kernel"]["median_us"] <
                          res["sdpa"]["median_us"])
    return res


def end_to_end(rounds):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    B, P, NEW = 8, 128, 128
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = GPT2(GPT2Config.gpt2_xl())
    model = to_bf16_training(model).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, P), device="cuda")

    def cached(new, gate):
        os.environ["RLA_DECODE_ATTN"] = gate
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(idx, new, temperature=0.0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def full_forward_per_token():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = idx
        with torch.no_grad():
            for _ in range(NEW):
                logits, _ = model(seq)
                tok = logits[:, -1].float().argmax(dim=-1, keepdim=True)
                seq = torch.cat([seq, tok], dim=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, seq

    runs = {
        "cache_kernel": lambda: cached(NEW, "1"),
        "cache_sdpa": lambda: cached(NEW, "0"),
        "prefill_only": lambda: cached(1, "1"),
        "full_forward_per_token": full_forward_per_token,
    }
    outs = {}
    for name, fn in runs.items():      # warm-up, every shape of the loop
        outs[name] = fn()[1]
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(fn()[0])
    res = {"B": B, "prompt": P, "new_tokens": NEW, "model": "gpt2-xl",
           "tokens_agree_kernel_vs_sdpa": float(
               (outs["cache_kernel"] == outs["cache_sdpa"]).float().mean()),
           "tokens_agree_kernel_vs_full": float(
               (outs["cache_kernel"] == outs["full_forward_per_token"])
               .float().mean())}
    prefill = statistics.median(times["prefill_only"])
    res["prefill_s"] = prefill
    for name in ("cache_kernel", "cache_sdpa", "full_forward_per_token"):
        t = statistics.median(times[name])
        res[name] = {"median_s": t, "min_s": min(times[name]),
                     "max_s": max(times[name]),
                     "tokens_per_s": B * NEW / t}
        if name != "full_forward_per_token":
            res[name]["decode_ms_per_token_step"] = \
                1e3 * (t - prefill) / (NEW - 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25,
                    help="seconds of device time per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-end-to-end", action="store_true")
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "decode_attn_fwd"):
        sys.exit("bench_decode_attn needs a GPU and the built HIP extension")

    points = []
    for B in (1, 8):
        for pos in (127, 511, 1023):
            r = kernel_point(ext, B, 25, 1024, pos, args.window, args.rounds)
            points.append(r)
            print(f"# B={B} pos={pos}: " + "  ".join(
                f"{n} {r[n]['median_us']:.1f}us" for n in
                ("kernel", "sdpa", "chunk64", "chunk128", "chunk256"))
                + f"  kernel {100 * r['kernel']['share_of_measured_hbm']:.1f}"
                "% of 6.29 TB/s", flush=True)
    default_on = all(r["kernel_wins"] for r in points if r["B"] == 8)
    out = {"chunk": int(ext.decode_attn_chunk()), "kernel": points,
           "default_on": default_on, "rounds": args.rounds,
           "window_s": args.window, "hip": torch.version.hip}
    if not args.skip_end_to_end:
        out["end_to_end"] = end_to_end(args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
