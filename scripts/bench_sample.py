"""sample_tokens (csrc/sample.hip, one launch) against the ATen chain the
decode loop runs without it: GPT2._sample plus the four EOS / scatter
calls of generate. B = 8, V = 50257, bf16 logits, temperature 1, at
top_k = 50, top_p = 0.9 (ATen: sort + cumsum + mask, below) and both.
Five alternating samples per side; prints median and range in
microseconds per call, host clock around a device synchronise.

    python scripts/bench_sample.py [--calls 300]
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["RLA_FUSED_SAMPLE"] = "1"

from ray_lightning_amd.models.gpt2 import GPT2  # noqa: E402
from ray_lightning_amd.ops.sample import sample_tokens  # noqa: E402

B, V, L = 8, 50257, 256


def aten_step(logits, top_k, top_p, gen, finished, out, col, eos, pad):
    logits = logits.float()
    if top_p is None:
        tok = GPT2._sample(logits, 1.0, top_k, gen)
    else:
        if top_k is not None:
            kth = logits.topk(top_k, dim=-1).values
            logits = logits.masked_fill(logits < kth[:, -1:], -math.inf)
        probs = torch.softmax(logits, dim=-1)
        ps, order = probs.sort(dim=-1, descending=True)
        drop = (ps.cumsum(-1) - ps) >= top_p
        probs = probs.masked_fill(
            torch.zeros_like(drop).scatter_(1, order, drop), 0.0)
        tok = torch.multinomial(probs, 1, generator=gen)[:, 0]
    tok = torch.where(finished, tok.new_tensor(pad), tok)
    finished = finished | (tok == eos)
    out.scatter_(1, col[:, None], tok[:, None])
    return tok, finished


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = "cuda"
    torch.manual_seed(0)
    logits = (4 * torch.randn(B, V, device=dev)).to(torch.bfloat16)
    seeds = torch.arange(B, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    out = torch.zeros(B, L, dtype=torch.int64, device=dev)
    col = torch.full((B,), 5, dtype=torch.int64, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.calls):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e6

    for top_k, top_p in ((50, None), (None, 0.9), (50, 0.9)):
        fin_k = torch.zeros(B, dtype=torch.bool, device=dev)
        fin_a = [torch.zeros(B, dtype=torch.bool, device=dev)]

        def kernel(i):
            sample_tokens(logits, seeds, i, top_k=top_k, top_p=top_p,
                          finished=fin_k, eos=V, pad=0, out=out, col=col)

        def aten(i):
            _, fin_a[0] = aten_step(logits, top_k, top_p, gen, fin_a[0],
                                    out, col, V, 0)

        for fn in (kernel, aten):  # warm-up
            timed(fn)
        ks, as_ = [], []
        for _ in range(5):
            ks.append(timed(kernel))
            as_.append(timed(aten))
        print(f"top_k={top_k} top_p={top_p}: "
              f"kernel {statistics.median(ks):.1f} us "
              f"[{min(ks):.1f}, {max(ks):.1f}]  "
              f"aten {statistics.median(as_):.1f} us "
              f"[{min(as_):.1f}, {max(as_):.1f}]", flush=True)


if __name__ == "__main__":
    main()
