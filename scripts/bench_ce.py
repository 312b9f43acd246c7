"""Time the GPT-2 LM-head loss, forward + backward, at the shape it has
in the GPT-2-XL benchmark (N = 16*1024 rows, C = 1600, V = 50257, bf16,
chunk_rows = 8192):

  (a) a baseline ``chunked_ce.py`` given with ``--baseline-file`` (the
      file of an earlier commit), when given
  (b) the torch path   (``RLA_FUSED_CE=0``)
  (c) the fused path   (``RLA_FUSED_CE=1``, csrc/fused_ce.hip)

The paths alternate in rounds on the same tensors; times are
device-event times per iteration, and each path's peak memory is the
allocator's high-water mark over one forward + backward above what the
inputs hold. The two kernels are also timed alone on one chunk of
logits, against the bytes they must move (forward reads the chunk once;
backward reads and writes it once).
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops import chunked_ce  # noqa: E402

HBM_ACHIEVABLE_GBPS = 6300.0  # MI355X streaming figure, of 8000 peak


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def load_baseline(path):
    spec = importlib.util.spec_from_file_location(
        "ray_lightning_amd.ops._baseline_chunked_ce", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.chunked_cross_entropy


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t),
            "max_ms": max(t), "spread_ms": max(t) - min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16 * 1024)
    ap.add_argument("--cols", type=int, default=1600)
    ap.add_argument("--vocab", type=int, default=50257)
    ap.add_argument("--chunk-rows", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--baseline-file", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops._load_ext() is None:
        sys.exit("bench_ce needs a GPU and the built HIP extension")

    N, C, V = args.rows, args.cols, args.vocab
    torch.manual_seed(0)
    dev, bf = "cuda", torch.bfloat16
    x = (torch.randn(N, C, device=dev) * 0.5).to(bf).requires_grad_(True)
    w = (torch.randn(V, C, device=dev) * 0.02).to(bf).requires_grad_(True)
    t = torch.randint(0, V, (N,), device=dev)

    def fwd_bwd(loss_fn, env):
        def run():
            if env is None:
                os.environ.pop("RLA_FUSED_CE", None)
            else:
                os.environ["RLA_FUSED_CE"] = env
            loss = loss_fn(x, w, t, args.chunk_rows)
            return (loss,) + torch.autograd.grad(loss, [x, w])
        return run

    paths = {}
    if args.baseline_file:
        paths["a_baseline"] = fwd_bwd(load_baseline(args.baseline_file),
                                      None)
    paths["b_torch"] = fwd_bwd(chunked_ce.chunked_cross_entropy, "0")
    paths["c_fused"] = fwd_bwd(chunked_ce.chunked_cross_entropy, "1")

    # same loss and gradients on every path, and the memory each needs
    ref = None
    check, peak = {}, {}
    for name, fn in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        if ref is None:
            ref = out
        check[name] = {
            "loss": float(out[0]),
            "max_abs_dx_vs_first": float(
                (out[1].float() - ref[1].float()).abs().max()),
            "max_abs_dw_vs_first": float(
                (out[2].float() - ref[2].float()).abs().max()),
            "max_abs_dx": float(out[1].float().abs().max()),
            "max_abs_dw": float(out[2].float().abs().max()),
        }
        del out
    del ref

    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, fn in paths.items():
            times[name].append(timed(fn, args.iters))
    result = {name: dict(stats(ts), peak_GiB=peak[name])
              for name, ts in times.items()}

    # the two kernels alone on one chunk of logits
    ext = ops._load_ext()
    R = min(args.chunk_rows, N)
    logits = (torch.randn(R, V, device=dev) * 2).to(bf)
    one = torch.ones(1, device=dev)
    _, lse, lse_lo = ext.fused_ce_fwd(logits, t[:R], -100, 0.0, 0.0)
    kern = {
        "fused_ce_fwd": (lambda: ext.fused_ce_fwd(
            logits, t[:R], -100, 0.0, 0.0), R * V * 2),
        "fused_ce_bwd": (lambda: ext.fused_ce_bwd(
            logits, lse, lse_lo, t[:R], one, -100, 0.0, 0.0),
            2 * R * V * 2),
    }
    kernels = {}
    for name, (fn, nbytes) in kern.items():
        for _ in range(5):
            fn()
        ts = [timed(fn, args.iters) for _ in range(args.rounds)]
        s = stats(ts)
        gbps = nbytes / (s["median_ms"] * 1e-3) / 1e9
        kernels[name] = dict(s, bytes=nbytes, GBps=gbps,
                             of_achievable_hbm=gbps / HBM_ACHIEVABLE_GBPS)

    first = next(iter(paths))
    b, c = result[first], result["c_fused"]
    print(json.dumps({
        "rows": N, "cols": C, "vocab": V, "chunk_rows": args.chunk_rows,
        "dtype": "bf16", "paths": result, "kernels": kernels,
        "compared_with": first,
        "fused_over_compared": c["median_ms"] / b["median_ms"],
        "fused_faster_by_more_than_spread":
            b["median_ms"] - c["median_ms"] > max(
                r["spread_ms"] for r in result.values()),
        "check": check, "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
