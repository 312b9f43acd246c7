"""Measure the skinny-linear kernel and GPT-2-XL's decode step with it on
one GPU. Fails without a GPU and the built extension.

(a) Kernel against the composed path at GPT-2-XL's five decode linears,
    each with the neighbours the model fuses into it, M in {1, 8, 16, 64}:

      c_attn    4800 x 1600   add + LN prologue, bias
      attn_proj 1600 x 1600   bias
      c_fc      6400 x 1600   add + LN prologue, bias, GELU
      mlp_proj  1600 x 6400   bias
      lm_head  50257 x 1600   add + LN prologue

      w4r1 / w8r1 / w8r2   skinny_linear_fwd_at with 4 or 8 K-splitting
                           waves and 16 or 32 weight rows per workgroup
      composed             fused add + LayerNorm kernel, F.linear
                           (hipBLASLt), F.gelu: the model's path
      f8{n,w}r{1,2}u{8,16}
                           skinny_linear_fp8_fwd_at on the quantized ring
                           (not the LM head, which stays bf16): narrow
                           (8-byte) or wide (16-byte) weight loads, 16 or
                           32 weight rows per workgroup, 8 or 16
                           k-steps in flight; its share of 6.29 TB/s is
                           on the fp8 weight bytes

    A decode step visits every layer's weights once, so the timed loop
    walks a ring of 48 weight matrices (8 for the LM head, 1.3 GB) and
    the stream comes from HBM, not from the Infinity Cache. Times are
    call times (device events over a loop, launch cost included); the
    share of 6.29 TB/s is weight bytes over that time, so it understates
    the kernel's own rate. Contestants alternate in one process; each
    sample is enough calls to fill --window seconds; median of 5.

(b) End to end: gpt2-xl, bf16, prompt 128, 128 new tokens, greedy, B = 8
    and B = 1, RLA_SKINNY_LINEAR=1 against =0 (the composed path):
    seconds, tokens/s, ms per decode step (prefill taken off).

    Rule, fixed before the run: _SKINNY_DEFAULT = True iff the decode
    step is faster with the gate on at both B by more than the larger of
    the two contestants' min-max spreads.

(c) The same end to end on a model after quantize_weights_fp8(), with
    RLA_SKINNY_LINEAR=1: RLA_SKINNY_FP8=1 against =0 (the bf16 kernels on
    the dequantized weights, the same function). The same rule decides
    _FP8_DEFAULT.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops.fused_ln import dropout_add_layer_norm  # noqa: E402

HBM_MEASURED = 6.29e12
EPS = 1e-5
SHAPES = [  # name, N, K, add + LN, GELU, bias, ring
    ("c_attn", 4800, 1600, True, False, True, 48),
    ("attn_proj", 1600, 1600, False, False, True, 48),
    ("c_fc", 6400, 1600, True, True, True, 48),
    ("mlp_proj", 1600, 6400, False, False, True, 48),
    ("lm_head", 50257, 1600, True, False, False, 8),
]
CONFIGS = {"w4r1": (4, 1), "w8r1": (8, 1), "w8r2": (8, 2)}
FP8_CONFIGS = {  # row_tiles, wide, uk
    f"f8{'w' if wide else 'n'}r{rt}u{uk}": (rt, wide, uk)
    for uk in (16, 8) for wide in (False, True) for rt in (1, 2)}


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def kernel_point(ext, name, N, K, ln, gelu, bias, ring_n, M, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(N + K + M)

    def rand(*shape, std=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * std)

    x = rand(M, K).bfloat16()
    res = rand(M, K).bfloat16() if ln else None
    gamma = 1 + 0.1 * rand(K) if ln else None
    beta = 0.1 * rand(K) if ln else None
    b = rand(N, std=0.02).bfloat16() if bias else None
    ring = [rand(N, K, std=0.02).bfloat16() for _ in range(ring_n)]

    def at(waves, rows):
        def run(i):
            return ext.skinny_linear_fwd_at(x, ring[i % ring_n], b, res,
                                            gamma, beta, EPS, gelu, waves,
                                            rows)[0]
        return run

    def composed(i):
        h = x
        if ln:
            _, h = dropout_add_layer_norm(x, res, gamma, beta, EPS, 0.0)
        y = F.linear(h, ring[i % ring_n], b)
        return F.gelu(y, approximate="tanh") if gelu else y

    fns = {k: at(*v) for k, v in CONFIGS.items()}
    fns["composed"] = composed
    fp8_bytes = {}
    if name != "lm_head":
        from ray_lightning_amd.ops.skinny_linear import quantize_weight
        ring8 = [quantize_weight(w) for w in ring]

        def at8(rows, wide, uk):
            def run(i):
                q, s = ring8[i % ring_n]
                return ext.skinny_linear_fp8_fwd_at(
                    x, q, s, b, res, gamma, beta, EPS, gelu, rows, wide,
                    uk)[0]
            return run

        for k, v in FP8_CONFIGS.items():
            fns[k] = at8(*v)
            fp8_bytes[k] = N * K
    diff = (fns["w8r1"](0).float() - composed(0).float()).abs().max().item()
    iters = {}
    for k, fn in fns.items():
        for i in range(2 * ring_n):
            fn(i)
        torch.cuda.synchronize()
        per_ms = timed(fn, 2 * ring_n)
        iters[k] = -(-(int(window * 1e3 / per_ms) + 1) // ring_n) * ring_n
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters[k]))
    out = {"shape": name, "N": N, "K": K, "M": M, "weight_bytes": 2 * N * K,
           "max_abs_diff_w8r1_vs_composed": diff}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"median_us": 1e3 * med, "min_us": 1e3 * min(t),
                  "max_us": 1e3 * max(t),
                  "share_of_measured_hbm": fp8_bytes.get(k, 2 * N * K) /
                  (med * 1e-3) / HBM_MEASURED}
    return out


def end_to_end(rounds, var="RLA_SKINNY_LINEAR", fp8=False):
    """The gate `var` on against off; `fp8`: on a quantized model with
    the skinny kernels on."""
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    P, NEW = 128, 128
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = GPT2(GPT2Config.gpt2_xl())
    model = to_bf16_training(model).eval()
    if fp8:
        model.quantize_weights_fp8()
        os.environ["RLA_SKINNY_LINEAR"] = "1"
    results = []
    for B in (8, 1):
        idx = torch.randint(0, model.cfg.vocab_size, (B, P), device="cuda")

        def run(new, gate):
            os.environ[var] = gate
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(idx, new, temperature=0.0)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        outs = {gate: run(NEW, gate)[1] for gate in "10"}   # warm-up
        run(1, "1")
        total = {"1": [], "0": []}
        prefill = []
        for _ in range(rounds):
            for gate in "10":
                total[gate].append(run(NEW, gate)[0])
            prefill.append(run(1, "1")[0])
        pre = statistics.median(prefill)
        r = {"B": B, "prompt": P, "new_tokens": NEW, "prefill_s": pre,
             "tokens_agree_on_vs_off": float(
                 (outs["1"] == outs["0"]).float().mean())}
        for gate, key in (("1", "gate_on"), ("0", "gate_off")):
            step = [1e3 * (t - pre) / (NEW - 1) for t in total[gate]]
            med = statistics.median(total[gate])
            r[key] = {"median_s": med, "min_s": min(total[gate]),
                      "max_s": max(total[gate]),
                      "tokens_per_s": B * NEW / med,
                      "decode_ms_per_step": statistics.median(step),
                      "decode_ms_min": min(step), "decode_ms_max": max(step)}
        on, off = r["gate_on"], r["gate_off"]
        spread = max(on["decode_ms_max"] - on["decode_ms_min"],
                     off["decode_ms_max"] - off["decode_ms_min"])
        r["spread_ms"] = spread
        r["gate_on_wins"] = (off["decode_ms_per_step"] -
                             on["decode_ms_per_step"]) > spread
        results.append(r)
        print(f"# {var} B={B}: on {on['decode_ms_per_step']:.3f} ms/step, off "
              f"{off['decode_ms_per_step']:.3f} ms/step, spread "
              f"{spread:.3f}", flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of device time per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--skip-fp8-end-to-end", action="store_true")
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "skinny_linear_fwd"):
        sys.exit("bench_skinny_linear needs a GPU and the built HIP "
                 "extension")
    out = {"rounds": args.rounds, "window_s": args.window,
           "hip": torch.version.hip, "kernel": []}
    for name, N, K, ln, gelu, bias, ring_n in SHAPES:
        for M in (1, 8, 16, 64):
            if args.skip_kernel:
                continue
            r = kernel_point(ext, name, N, K, ln, gelu, bias, ring_n, M,
                             args.window, args.rounds)
            out["kernel"].append(r)
            print(f"# {name} M={M}: " + "  ".join(
                f"{k} {r[k]['median_us']:.1f}us" for k in
                (*CONFIGS, "composed", *FP8_CONFIGS) if k in r) +
                f"  w8r1 {100 * r['w8r1']['share_of_measured_hbm']:.1f}% of "
                "6.29 TB/s", flush=True)
    if not args.skip_end_to_end:
        out["end_to_end"] = end_to_end(args.rounds)
        out["default_on"] = all(r["gate_on_wins"]
                                for r in out["end_to_end"])
    if not args.skip_fp8_end_to_end:
        out["end_to_end_fp8"] = end_to_end(args.rounds, "RLA_SKINNY_FP8",
                                           fp8=True)
        out["fp8_default_on"] = all(r["gate_on_wins"]
                                    for r in out["end_to_end_fp8"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
