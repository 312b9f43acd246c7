"""Measure the fp8 KV cache on one GPU (profiles/kv_fp8.md). Fails without
a GPU and the built extension.

(a) Decode attention, fp8 cache against bf16 cache: H=25, hs=64,
    Tmax=1024, B in {8, 64}, pos in {128, 512, 1023}, every row at the
    same pos. Contestants: the bf16 kernel, the fp8 kernel as built, and
    the fp8 kernel at 2 and 4 waves through the measurement entry point.
    As in bench_decode_attn.py the timed loop walks a ring of 48 cache
    sets (one per GPT-2-XL layer), contestants alternate in one process,
    each sample is device-event time over --window seconds of calls, and
    the median, min and max of --rounds samples are reported. Bytes read
    are 2 * pos * 128 per (b, h) for bf16 and 2 * pos * (64 + 4) for fp8;
    the rate is given as a share of the 6.29 TB/s measured HBM figure.
(b) kv_cache_fill against the two strided copy_ calls of the bf16 fill,
    B=8, H=25, T in {128, 1024}.
(c) GPT-2-XL decode step, RLA_SKINNY_LINEAR=1, bf16 and fp8 weights,
    B in {8, 64}, 512 prompt + 128 new tokens, greedy: fp8 cache against
    bf16 cache, ms per step as (t(128 new) - t(2 new)) / 126, and peak
    memory; once more at B=8 on the composed path (RLA_SKINNY_LINEAR=0).
(d) The largest logit difference between an fp8-cache and a bf16-cache
    greedy run of the test model (2 layers, 2 heads, n_embd 128) on random
    weights, over the steps before their tokens first differ.
(e) Append attention over an fp8 cache (profiles/append_attn_fp8.md), at
    the points of profiles/append_attn.md: B=8, H=25, Tmax=1024, pos in
    {128, 512, 960}, T in {4, 16, 64}. Contestants: the fp8 append kernel,
    the ``_fp8`` torch composition it replaces (quantize and scatter with
    ATen, dequantize both caches, the bf16 append kernel on the copies),
    and the bf16 append kernel on a bf16 cache. Rule, fixed before the run:
    the kernel is the default over an fp8 cache iff at all nine points its
    median is below the composition's by more than the larger of the two
    spreads.
(f) GPT-2-XL, fp8 weights, RLA_SKINNY_LINEAR=1, fp8 cache: one extend
    forward to the last token's logits, with the kernel and with the
    composition: a 64-token turn on 512 cached tokens at B=8, and a
    spec-decode step's forward (T = 7) on 256 cached tokens at B=8 and
    B=64; peak allocated memory of the call.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops import append_attn as aa  # noqa: E402
from ray_lightning_amd.ops import decode_attn as da  # noqa: E402

HBM_MEASURED = 6.29e12
LAYERS = 48
HS = 64


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(fns, window, rounds, ring=LAYERS):
    """{name: {median_us, min_us, max_us}} of contestants run in turn."""
    iters = {}
    for name, fn in fns.items():
        for i in range(2 * ring):
            fn(i)
        torch.cuda.synchronize()
        n = int(window * 1e3 / timed(fn, 2 * ring)) + 1
        iters[name] = -(-n // ring) * ring
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, iters[name]))
    return {name: {"median_us": 1e3 * statistics.median(t),
                   "min_us": 1e3 * min(t), "max_us": 1e3 * max(t)}
            for name, t in times.items()}


def kernel_point(ext, B, H, Tmax, pos, window, rounds):
    scale = 1.0 / math.sqrt(HS)
    g = torch.Generator(device="cuda").manual_seed(pos + B)
    qkv = torch.randn(B, 3 * H * HS, device="cuda", generator=g).bfloat16()
    ring = []
    for _ in range(LAYERS):
        k = torch.randn(B, H, Tmax, HS, device="cuda", generator=g).bfloat16()
        v = torch.randn(B, H, Tmax, HS, device="cuda", generator=g).bfloat16()
        ring.append((k, v) + da.quantize_kv(k) + da.quantize_kv(v))
    pos_t = torch.full((B,), pos, dtype=torch.int32, device="cuda")

    def bf16(i):
        k, v = ring[i % LAYERS][:2]
        return ext.decode_attn_fwd(qkv, k, v, pos_t, pos, scale)

    def fp8(i):
        _, _, k8, ks, v8, vs = ring[i % LAYERS]
        return ext.decode_attn_fwd(qkv, k8, v8, pos_t, pos, scale, ks, vs)

    def at_waves(waves):
        def run(i):
            _, _, k8, ks, v8, vs = ring[i % LAYERS]
            return ext.decode_attn_fp8_fwd_at(qkv, k8, v8, ks, vs, pos_t,
                                              pos, scale, waves)
        return run

    fns = {"bf16": bf16, "fp8": fp8, "fp8_2waves": at_waves(2),
           "fp8_4waves": at_waves(4)}
    res = {"B": B, "pos": pos,
           "fp8_vs_bf16_max_abs_diff":
               (fp8(0).float() - bf16(0).float()).abs().max().item()}
    res.update(alternate(fns, window, rounds))
    for name, r in res.items():
        if isinstance(r, dict):
            per_pos = 2 * 2 * HS if name == "bf16" else 2 * (HS + 4)
            r["bytes"] = pos * per_pos * B * H
            r["share_of_measured_hbm"] = \
                r["bytes"] / (r["median_us"] * 1e-6) / HBM_MEASURED
    return res


def fill_point(B, H, T, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(T)
    C = H * HS
    qkv = torch.randn(B, T, 3 * C, device="cuda", generator=g).bfloat16()
    ring = [(torch.zeros(B, H, T, HS, device="cuda", dtype=torch.bfloat16),
             torch.zeros(B, H, T, HS, device="cuda", dtype=torch.bfloat16),
             da.KVCache(1, B, H, T, HS, da.FP8, "cuda")) for _ in range(8)]

    def copies(i):
        kc, vc, _ = ring[i % 8]
        _, k, v = qkv.split(C, dim=2)
        kc.copy_(k.view(B, T, H, HS).transpose(1, 2))
        vc.copy_(v.view(B, T, H, HS).transpose(1, 2))

    def fill(i):
        c = ring[i % 8][2]
        da.kv_cache_fill(qkv, c.k[0], c.v[0], c.k_scale[0], c.v_scale[0])

    res = {"B": B, "T": T}
    res.update(alternate({"copy_x2": copies, "kv_cache_fill": fill}, window,
                         rounds, ring=8))
    return res


def xl_steps(rounds):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = GPT2(GPT2Config.gpt2_xl())
    model = to_bf16_training(model).eval()
    P, NEW = 512, 128
    out = []

    def run(idx, new, kv_fp8):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        model.generate(idx, new, temperature=0.0, kv_fp8=kv_fp8)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated()

    def point(weights, skinny, B):
        os.environ["RLA_SKINNY_LINEAR"] = skinny
        idx = torch.randint(0, model.cfg.vocab_size, (B, P), device="cuda")
        res = {"weights": weights, "skinny": skinny, "B": B}
        for kv in (False, True):     # warm-up, both lengths
            run(idx, 2, kv), run(idx, NEW, kv)
        t = {(kv, n): [] for kv in (False, True) for n in (2, NEW)}
        peak = {}
        for _ in range(rounds):
            for kv in (False, True):
                for n in (2, NEW):
                    s, peak[kv] = run(idx, n, kv)
                    t[kv, n].append(s)
        for kv in (False, True):
            steps = [1e3 * (a - b) / (NEW - 2)
                     for a, b in zip(t[kv, NEW], t[kv, 2])]
            res["fp8_cache" if kv else "bf16_cache"] = {
                "step_ms_median": statistics.median(steps),
                "step_ms_min": min(steps), "step_ms_max": max(steps),
                "peak_GiB": peak[kv] / 2 ** 30}
        print("#", json.dumps(res), flush=True)
        out.append(res)

    for B in (8, 64):
        point("bf16", "1", B)
    point("bf16", "0", 8)
    model.quantize_weights_fp8()
    for B in (8, 64):
        point("fp8", "1", B)
    return out


def logit_difference():
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    torch.manual_seed(0)
    m = to_bf16_training(GPT2(GPT2Config(
        n_layer=2, n_embd=128, n_head=2, vocab_size=256,
        n_positions=128)).cuda()).eval()
    idx = torch.randint(0, 256, (8, 32), device="cuda")
    runs = [m.generate(idx, 64, temperature=0.0, return_logits=True,
                       kv_fp8=kv) for kv in (False, True)]
    same = (runs[0][0] == runs[1][0])[:, 32:].int().cumprod(dim=1)
    # step s of a row counts while tokens 0 .. s-1 agreed
    counted = torch.cat([torch.ones_like(same[:, :1]), same[:, :-1]], dim=1)
    diff = (runs[0][1] - runs[1][1]).abs().amax(dim=2) * counted
    return {"max_abs_logit_diff": diff.max().item(),
            "max_abs_logit": runs[0][1].abs().max().item(),
            "steps_counted": int(counted.sum()), "steps": counted.numel(),
            "tokens_agree": float(same.float().mean())}


_APPEND = aa.append_attention


def composition(qkv, k8, v8, pos, max_pos, n_head=None, k_scale=None,
                v_scale=None):
    """append_attention as it was before the fp8 append kernel: fp8 calls
    go to the ``_fp8`` composition, whose bf16 call comes back here."""
    if k_scale is None:
        return _APPEND(qkv, k8, v8, pos, max_pos, n_head)
    return aa._fp8(qkv.contiguous(), k8, v8, k_scale, v_scale, pos,
                   int(max_pos))


def append_point(B, H, Tmax, pos, T, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(pos + T)
    qkv = torch.randn(B, T, 3 * H * HS, device="cuda", generator=g).bfloat16()
    ring = []
    for _ in range(LAYERS):
        k = torch.randn(B, H, Tmax, HS, device="cuda", generator=g).bfloat16()
        v = torch.randn(B, H, Tmax, HS, device="cuda", generator=g).bfloat16()
        ring.append((k, v) + da.quantize_kv(k) + da.quantize_kv(v))
    pos_t = torch.full((B,), pos, dtype=torch.int32, device="cuda")

    def bf16(i):
        k, v = ring[i % LAYERS][:2]
        return aa.append_attention(qkv, k, v, pos_t, pos)

    def fp8(i):
        _, _, k8, ks, v8, vs = ring[i % LAYERS]
        return aa.append_attention(qkv, k8, v8, pos_t, pos, k_scale=ks,
                                   v_scale=vs)

    def composed(i):
        _, _, k8, ks, v8, vs = ring[i % LAYERS]
        return composition(qkv, k8, v8, pos_t, pos, None, ks, vs)

    fns = {"fp8_kernel": fp8, "fp8_composition": composed, "bf16_kernel": bf16}
    res = {"B": B, "pos": pos, "T": T,
           "kernel_vs_composition_max_abs_diff":
               (fp8(0).float() - composed(0).float()).abs().max().item()}
    res.update(alternate(fns, window, rounds))
    spread = lambda r: r["max_us"] - r["min_us"]
    k, c = res["fp8_kernel"], res["fp8_composition"]
    res["kernel_wins"] = c["median_us"] - k["median_us"] > \
        max(spread(k), spread(c))
    return res


def xl_append(rounds):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    os.environ["RLA_SKINNY_LINEAR"] = "1"
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = GPT2(GPT2Config.gpt2_xl())
    model = to_bf16_training(model).eval()
    model.quantize_weights_fp8()
    cfg = model.cfg
    out = []
    for B, P, T in ((8, 512, 64), (8, 256, 7), (64, 256, 7)):
        idx = torch.randint(0, cfg.vocab_size, (B, P + T), device="cuda")
        full = torch.full((B,), P, dtype=torch.int32, device="cuda")
        cache = da.KVCache(cfg.n_layer, B, cfg.n_head, 1024, HS, da.FP8,
                           "cuda")
        with torch.no_grad():
            model._hidden(idx[:, :P], None, cache)

        def run(op):
            aa.append_attention = op
            cache.set_lengths(full, P)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            with torch.no_grad():
                h = model._hidden(idx[:, P:], None, cache, True)
                logits = model.lm_head(h[:, -1]).float()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0, torch.cuda.max_memory_allocated(),
                    logits)

        ops_ = {"kernel": _APPEND, "composition": composition}
        res = {"B": B, "cached": P, "T": T}
        try:
            last = {n: run(op)[2] for n, op in ops_.items()}   # warm-up
            t = {n: [] for n in ops_}
            peak = {}
            for _ in range(rounds):
                for n, op in ops_.items():
                    s, peak[n], _ = run(op)
                    t[n].append(s)
        finally:
            aa.append_attention = _APPEND
        for n in ops_:
            res[n] = {"median_ms": 1e3 * statistics.median(t[n]),
                      "min_ms": 1e3 * min(t[n]), "max_ms": 1e3 * max(t[n]),
                      "peak_GiB": peak[n] / 2 ** 30}
        res["last_logits_max_abs_diff"] = \
            (last["kernel"] - last["composition"]).abs().max().item()
        print("#", json.dumps(res), flush=True)
        out.append(res)
        del cache
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25,
                    help="seconds of device time per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--append-only", action="store_true",
                    help="sections (e) and (f) only")
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "decode_attn_fp8_fwd_at"):
        sys.exit("bench_kv_fp8 needs a GPU and the built HIP extension")
    os.environ["RLA_DECODE_ATTN"] = "1"
    out = {"kernel": [], "fill": [], "hip": torch.version.hip,
           "rounds": args.rounds, "window_s": args.window}
    out["append"] = []
    for pos in (128, 512, 960):
        for T in (4, 16, 64):
            r = append_point(8, 25, 1024, pos, T, args.window, args.rounds)
            out["append"].append(r)
            print("#", json.dumps(r), flush=True)
    out["append_default_on"] = all(r["kernel_wins"] for r in out["append"])
    if not args.skip_model:
        out["xl_append"] = xl_append(args.rounds)
    if args.append_only:
        print(json.dumps(out))
        return
    for B in (8, 64):
        for pos in (128, 512, 1023):
            r = kernel_point(ext, B, 25, 1024, pos, args.window, args.rounds)
            out["kernel"].append(r)
            print("#", json.dumps(r), flush=True)
    for T in (128, 1024):
        r = fill_point(8, 25, T, args.window, args.rounds)
        out["fill"].append(r)
        print("#", json.dumps(r), flush=True)
    out["logits"] = logit_difference()
    print("#", json.dumps(out["logits"]), flush=True)
    if not args.skip_model:
        out["xl"] = xl_steps(3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
