"""Time causal attention from c_attn's output to c_proj's input at the
GPT-2-XL bench shape (B=16, H=25, T=1024, hs=64, bf16, p=0), forward +
backward, from ``qkv`` [B, T, 3C] and a ``dout`` [B, T, C] to ``o`` and
``dqkv``, on two paths:

  composed  what CausalSelfAttention did before the packed kernels:
            split, transpose and .contiguous() on q, k, v, the unpacked
            v3 kernels, transpose + .contiguous() of y, and autograd's
            mirror image in backward (the strided copy of dout, the
            copies that make dq, dk, dv contiguous, the cat into dqkv)
  packed    the PACKED instantiations of the same kernels: no copies

The two alternate in rounds on the same tensors, in one process, after a
warm-up of both; times are device-event times per iteration
(torch.autograd.grad, so no .grad accumulation is timed). Also reports
whether o and dqkv of the two paths are the same bits.

Rule, fixed before the run (profiles/flash_attn_packed.md):
_PACKED_DEFAULT = True iff the packed median is below the composed
median by more than the larger of the two ranges AND the GPT-2 step of
bench.py is not slower with the packed kernels than without.
"""
import argparse
import json
import os
import statistics
import sys

import torch

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
            "max_ms": max(t), "range_ms": max(t) - min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--heads", type=int, default=25)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "flash_attn_fwd_v3_packed"):
        sys.exit("bench_flash_packed needs a GPU and the built HIP "
                 "extension")

    B, H, T, hs = args.batch, args.heads, args.seq, 64
    C = H * hs
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3 * C, device="cuda").to(
        torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, T, C, device="cuda").to(torch.bfloat16)

    def composed():
        q, k, v = qkv.split(C, dim=2)
        q = q.view(B, T, H, hs).transpose(1, 2)
        k = k.view(B, T, H, hs).transpose(1, 2)
        v = v.view(B, T, H, hs).transpose(1, 2)
        y = fa.flash_attention(q, k, v)
        return y.transpose(1, 2).contiguous().view(B, T, C)

    def packed():
        return fa._FlashAttnPacked.apply(qkv, H, hs ** -0.5, 0.0, None,
                                         None)

    paths = {"composed": composed, "packed": packed}

    def fwd_bwd(attn):
        def run():
            o = attn()
            return o, torch.autograd.grad(o, qkv, dout)[0]
        return run

    fns = {name: fwd_bwd(fn) for name, fn in paths.items()}
    outs = {name: fn() for name, fn in fns.items()}
    same = {"o": torch.equal(outs["composed"][0], outs["packed"][0]),
            "dqkv": torch.equal(outs["composed"][1], outs["packed"][1])}
    del outs
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, args.iters))
    res = {name: stats(t) for name, t in times.items()}
    gain = res["composed"]["median_ms"] - res["packed"]["median_ms"]
    print(json.dumps({
        "B": B, "H": H, "T": T, "hs": hs, "p": 0.0, "dtype": "bf16",
        "fwd_bwd": res, "same_bits": same,
        "packed_over_composed":
            res["packed"]["median_ms"] / res["composed"]["median_ms"],
        "packed_wins_by_more_than_range":
            gain > max(res["composed"]["range_ms"],
                       res["packed"]["range_ms"]),
        "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
