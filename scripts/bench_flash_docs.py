"""Time document-masked causal attention for packed rows at the
GPT-2-XL shape (B=8, H=25, T=1024, hs=64, bf16, p=0), for three layouts
of every row:

  one    one document (the mask is the plain causal one)
  4x256  four documents of 256
  mixed  a fixed seeded mix of lengths that are no multiples of 64

and three paths:

  (a) the plain causal v3 flash kernels (they ignore the documents: the
      floor, and the wrong answer for the last two layouts)
  (b) F.scaled_dot_product_attention with the boolean [B,1,T,T] mask,
      what flash_attention(..., doc_ids=) falls back to; timed with the
      mask built once outside the loop (b_sdpa_mask) and, as the
      fallback does it, built from the bounds in every call
      (b_sdpa_mask_built)
  (c) the DOCS instantiations of the v3 flash kernels

The paths alternate in rounds on the same tensors, in one process; times
are device-event times per iteration, forward only and forward +
backward (torch.autograd.grad, so no .grad accumulation is timed).

Rules, fixed before the run (profiles/flash_attn_docs.md):
- _DOCS_DEFAULT = True iff the forward+backward median of (c) beats that
  of (b) on the mixed layout by more than the larger of the two spreads;
  (b) is the faster variant, the one with the mask built outside.
- cost of the flag: (c) on one document against (a).
- gain from skipping: (c) on 4x256 against (c) on one document; if it is
  not faster by more than the spread the skipping does not work.
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


def mixed_lengths(T, seed):
    """Document lengths of one row: seeded, none a multiple of 64."""
    g = torch.Generator().manual_seed(seed)
    out, left = [], T
    while left > 0:
        n = int(torch.randint(17, 400, (1,), generator=g))
        if n % 64 == 0:
            n += 1
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def ids_of(rows, T):
    return torch.stack([
        torch.cat([torch.full((n,), i) for i, n in enumerate(row)])
        for row in rows]).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=25)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ext = ops._load_ext() if torch.cuda.is_available() else None
    if ext is None or not hasattr(ext, "flash_attn_fwd_v3_docs"):
        sys.exit("bench_flash_docs needs a GPU and the built HIP extension")

    B, H, T, hs = args.batch, args.heads, args.seq, 64
    scale = 1.0 / math.sqrt(hs)
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, T, hs, device="cuda").to(
        torch.bfloat16).requires_grad_(True) for _ in range(3))
    dy = torch.randn(B, H, T, hs, device="cuda").to(torch.bfloat16)
    leaves = [q, k, v]

    layouts = {
        "one": [[T]] * B,
        "4x256": [[T // 4] * 4] * B,
        "mixed": [mixed_lengths(T, 1000 + b) for b in range(B)],
    }
    out = {"layouts": {"mixed": layouts["mixed"]}}
    for lname, rows in layouts.items():
        start, end = fa.doc_bounds(ids_of(rows, T))
        mask = fa.doc_mask(start)
        allowed_share = mask.float().mean().item()

        def attn_a():
            return fa._FlashAttn.apply(q, k, v, scale)

        def attn_b():
            return F.scaled_dot_product_attention(q, k, v, attn_mask=mask)

        def attn_b_built():
            return F.scaled_dot_product_attention(
                q, k, v, attn_mask=fa.doc_mask(start))

        def attn_c():
            return fa._FlashAttnDocs.apply(q, k, v, start, end, scale, 0.0)

        paths = {"a_flash_causal": attn_a, "b_sdpa_mask": attn_b,
                 "b_sdpa_mask_built": attn_b_built, "c_flash_docs": attn_c}

        with torch.no_grad():
            err = (attn_c().float() - attn_b().float()).abs().max().item()

        def fwd(attn):
            def run():
                with torch.no_grad():
                    attn()
            return run

        def fwd_bwd(attn):
            def run():
                torch.autograd.grad(attn(), leaves, dy)
            return run

        res = {"allowed_share_of_TxT": allowed_share,
               "c_vs_b_max_abs_diff": err}
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
            res[kind] = {name: stats(t) for name, t in times.items()}
            r = res[kind]
            r["c_over_a"] = (r["c_flash_docs"]["median_ms"] /
                             r["a_flash_causal"]["median_ms"])
            r["c_over_b"] = (r["c_flash_docs"]["median_ms"] /
                             r["b_sdpa_mask"]["median_ms"])
            r["c_beats_b_by_more_than_spread"] = (
                r["b_sdpa_mask"]["median_ms"] -
                r["c_flash_docs"]["median_ms"] >
                max(r["b_sdpa_mask"]["spread_ms"],
                    r["c_flash_docs"]["spread_ms"]))
        out[lname] = res

    skip = {}
    for kind in ("fwd", "fwd_bwd"):
        one = out["one"][kind]["c_flash_docs"]
        four = out["4x256"][kind]["c_flash_docs"]
        skip[kind] = {
            "c_4x256_over_c_one": four["median_ms"] / one["median_ms"],
            "faster_by_more_than_spread":
                one["median_ms"] - four["median_ms"] >
                max(one["spread_ms"], four["spread_ms"])}
    print(json.dumps({
        "B": B, "H": H, "T": T, "hs": hs, "p": 0.0, "dtype": "bf16",
        **out, "skipping": skip,
        "default_on":
            out["mixed"]["fwd_bwd"]["c_beats_b_by_more_than_spread"],
        "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
