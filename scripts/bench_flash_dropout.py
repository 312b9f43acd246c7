"""Time causal attention with dropout on the probabilities at the
GPT-2-XL shape (B=8, H=25, T=1024, hs=64, bf16, p=0.1):

  (a) the v3 flash kernels, p = 0                        (the floor)
  (b) F.scaled_dot_product_attention(dropout_p=p, is_causal=True)
      (what flash_attention(..., dropout_p > 0) did before the kernels
      had dropout)
  (c) the v3 flash kernels' DROPOUT instantiations (ops/flash_attn.py)

The three alternate in rounds on the same tensors, in one process;
times are device-event times per iteration, forward only and forward +
backward (torch.autograd.grad, so no .grad accumulation is timed).

The dropped share of (b) and (c) is read off the output: with q = k = 0
the probabilities are uniform over the causal row, and with V zero
except V[:64] = identity, o[b,h,q,d] != 0 iff (q, d) was kept.

The decision the note records: (c) is the default iff its forward +
backward median beats (b)'s by more than the larger of the two spreads.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops import flash_attn as fa  # noqa: E402


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t),
            "max_ms": max(t), "spread_ms": max(t) - min(t)}


def dropped_share(attn, B, H, T, hs):
    z = torch.zeros(B, H, T, hs, device="cuda", dtype=torch.bfloat16)
    v = z.clone()
    v[:, :, :hs] = torch.eye(hs, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        o = attn(z, z, v)
    causal = torch.tril(torch.ones(T, hs, device="cuda", dtype=torch.bool))
    kept = ((o != 0) & causal).sum().item()
    return 1.0 - kept / (B * H * causal.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=25)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "flash_attn_fwd_v3_dropout"):
        sys.exit("bench_flash_dropout needs a GPU and the built HIP "
                 "extension")

    B, H, T, hs, p = args.batch, args.heads, args.seq, 64, args.p
    scale = 1.0 / math.sqrt(hs)
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, T, hs, device="cuda").to(
        torch.bfloat16).requires_grad_(True) for _ in range(3))
    dy = torch.randn(B, H, T, hs, device="cuda").to(torch.bfloat16)
    leaves = [q, k, v]

    def attn_a(q, k, v):
        return fa._FlashAttn.apply(q, k, v, scale)

    def attn_b(q, k, v):
        return F.scaled_dot_product_attention(q, k, v, dropout_p=p,
                                              is_causal=True)

    def attn_c(q, k, v):
        return fa._FlashAttnDropout.apply(q, k, v, scale, p)

    paths = {"a_flash_p0": attn_a, "b_sdpa_dropout": attn_b,
             "c_flash_dropout": attn_c}

    def fwd(attn):
        def run():
            with torch.no_grad():
                attn(q, k, v)
        return run

    def fwd_bwd(attn):
        def run():
            torch.autograd.grad(attn(q, k, v), leaves, dy)
        return run

    check = {name + "_dropped_share": dropped_share(fn, B, H, T, hs)
             for name, fn in paths.items()}

    out = {}
    for kind, wrap in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
        fns = {name: wrap(fn) for name, fn in paths.items()}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, args.iters))
        out[kind] = {name: stats(t) for name, t in times.items()}
        a, b, c = (out[kind][n]["median_ms"] for n in paths)
        out[kind]["c_over_a"] = c / a
        out[kind]["c_over_b"] = c / b
        out[kind]["c_beats_b_by_more_than_spread"] = (
            b - c > max(out[kind]["b_sdpa_dropout"]["spread_ms"],
                        out[kind]["c_flash_dropout"]["spread_ms"]))

    print(json.dumps({
        "B": B, "H": H, "T": T, "hs": hs, "p": p, "dtype": "bf16",
        **out, "check": check,
        "default_on": out["fwd_bwd"]["c_beats_b_by_more_than_spread"],
        "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
