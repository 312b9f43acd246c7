"""Measure fp8_linear and GPT-2-XL without its bf16 block weights on one
GPU. Fails without a GPU and the built extension.

(a) Call time at GPT-2-XL's four block linears (N x K: c_attn 4800 x 1600,
    attn_proj 1600 x 1600, c_fc 6400 x 1600 with GELU, mlp_proj 1600 x
    6400; all with bias), M in {8, 16, 32, 64, 128, 512, 1024, 8192}:

      t64 / t128   fp8_linear_fwd_at at the 64 x 64 / 128 x 128 tile
      skinny       skinny_linear_fwd on the fp8 pair (M <= 64 only)
      composed     F.linear (hipBLASLt) on the dequantized bf16 weight,
                   then F.gelu for c_fc: a kept model's path

    Device events around a loop that fills --window seconds, warm-up per
    shape and contestant, contestants alternated in one process, median and
    min / max of --rounds samples. FLOP/s is 2 M N K over the call time,
    against 2.5 PFLOP/s, the published dense bf16 matrix rate.

(b) End to end, gpt2-xl, a kept model (quantize_weights_fp8()) against a
    dropped one (drop_bf16=True) from the same seed: prefill of 8 x 512,
    a 64-token extend on 512 cached, one decode step at B = 8 (ms each,
    host clock around a synchronise), the bytes the block linears hold and
    the peak memory of generate(8 x 512, 64 new tokens).
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
from ray_lightning_amd.ops.skinny_linear import (dequantize_weight,  # noqa: E402
                                                 quantize_weight)

BF16_PEAK = 2.5e15
SHAPES = [("c_attn", 4800, 1600, False), ("attn_proj", 1600, 1600, False),
          ("c_fc", 6400, 1600, True), ("mlp_proj", 1600, 6400, False)]
ROWS = (8, 16, 32, 64, 128, 512, 1024, 8192)


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def kernel_point(ext, name, N, K, gelu, M, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(N + K + M)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    b = (torch.randn(N, device="cuda", generator=g) * 0.02).bfloat16()
    q, s = quantize_weight(
        torch.randn(N, K, device="cuda", generator=g) * 0.02)
    w = dequantize_weight(q, s)

    def composed():
        y = F.linear(x, w, b)
        return F.gelu(y, approximate="tanh") if gelu else y

    fns = {"t64": lambda: ext.fp8_linear_fwd_at(x, q, s, b, gelu, 64),
           "t128": lambda: ext.fp8_linear_fwd_at(x, q, s, b, gelu, 128),
           "composed": composed}
    if M <= 64:
        fns["skinny"] = lambda: ext.skinny_linear_fwd(
            x, q, b, None, None, None, 0.0, gelu, s)[0]
    diff = (fns["t64"]().float() - composed().float()).abs().max().item()
    iters = {}
    for k, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        iters[k] = int(window * 1e3 / timed(fn, 20)) + 1
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters[k]))
    out = {"shape": name, "N": N, "K": K, "M": M,
           "max_abs_diff_t64_vs_composed": diff}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"median_us": 1e3 * med, "min_us": 1e3 * min(t),
                  "max_us": 1e3 * max(t),
                  "tflops": 2 * M * N * K / (med * 1e-3) / 1e12,
                  "share_of_bf16_peak": 2 * M * N * K / (med * 1e-3) /
                  BF16_PEAK}
    return out


def end_to_end(rounds):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    from ray_lightning_amd.ops.decode_attn import KVCache
    B, P, T = 8, 512, 64
    results = {}
    for name, drop in (("kept", False), ("dropped", True)):
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = GPT2(GPT2Config.gpt2_xl())
        model = to_bf16_training(model).eval()
        model.quantize_weights_fp8(drop_bf16=drop)
        torch.cuda.empty_cache()
        cfg = model.cfg
        held = sum(t.numel() * t.element_size()
                   for lin in model._block_linears()
                   for t in (lin.weight, lin.weight_fp8, lin.weight_scale))
        idx = torch.randint(0, cfg.vocab_size, (B, P + T), device="cuda",
                            generator=torch.Generator("cuda").manual_seed(1))

        def phases():
            cache = KVCache(cfg.n_layer, B, cfg.n_head, 1024,
                            cfg.n_embd // cfg.n_head, torch.bfloat16, "cuda")
            ts = []
            with torch.no_grad():
                for args in ((idx[:, :P], False), (idx[:, P:], True),
                             (idx[:, :1], False)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model(args[0], cache=cache, extend=args[1])
                    torch.cuda.synchronize()
                    ts.append(1e3 * (time.perf_counter() - t0))
            return ts

        phases()  # warm-up
        runs = [phases() for _ in range(rounds)]
        r = {"block_linear_bytes": held}
        for i, key in enumerate(("prefill_8x512_ms", "extend_64_on_512_ms",
                                 "decode_step_B8_ms")):
            v = [run[i] for run in runs]
            r[key] = {"median": statistics.median(v), "min": min(v),
                      "max": max(v)}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        model.generate(idx[:, :P], T, temperature=0.0)
        torch.cuda.synchronize()
        r["generate_peak_mib"] = torch.cuda.max_memory_allocated() / 2 ** 20
        results[name] = r
        print(f"# {name}: " + json.dumps(r), flush=True)
        del model
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2,
                    help="seconds of device time per sample")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--once", nargs=3, type=int, metavar=("M", "SHAPE", "N"),
                    help="no timing: N calls of the host's pick at M rows "
                    "of shape number SHAPE, for a kernel trace")
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "fp8_linear_fwd"):
        sys.exit("bench_fp8_linear needs a GPU and the built HIP extension")
    if args.once:
        M, shape, n = args.once
        _, N, K, gelu = SHAPES[shape]
        x = torch.randn(M, K, device="cuda").bfloat16()
        q, s = quantize_weight(torch.randn(N, K, device="cuda") * 0.02)
        b = torch.zeros(N, device="cuda").bfloat16()
        for _ in range(n):
            ext.fp8_linear_fwd(x, q, s, b, gelu)
        torch.cuda.synchronize()
        return
    out = {"rounds": args.rounds, "window_s": args.window,
           "hip": torch.version.hip, "kernel": []}
    for name, N, K, gelu in SHAPES:
        for M in ROWS:
            if args.skip_kernel:
                continue
            r = kernel_point(ext, name, N, K, gelu, M, args.window,
                             args.rounds)
            out["kernel"].append(r)
            print(f"# {name} M={M}: " + "  ".join(
                f"{k} {r[k]['median_us']:.1f}us "
                f"[{r[k]['min_us']:.1f}, {r[k]['max_us']:.1f}]"
                for k in ("t64", "t128", "skinny", "composed") if k in r) +
                f"  t128 {r['t128']['tflops']:.0f} TFLOP/s", flush=True)
    if not args.skip_end_to_end:
        out["end_to_end"] = end_to_end(args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
