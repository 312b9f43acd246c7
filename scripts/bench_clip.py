"""Time global-norm clipping + optimizer step over GPT-2-XL's actual
parameter list (bf16 weights, fp32 norms, as ``to_bf16_training`` makes
them):

  (a) torch.nn.utils.clip_grad_norm_ then ShardedFusedAdam.step()
  (b) HIP sum of squares -> device coefficient -> ShardedFusedAdam.step()
      with the coefficient as a multiplier inside the kernel
  (c) the sum-of-squares kernels alone, as GB/s of gradient bytes read

(a) and (b) alternate in rounds on the same parameters, grads and
optimizer state; times are device-event times per iteration. (a) clips
the shared grads in place, so they are restored after each of its
blocks.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,  # noqa: E402
                                           to_bf16_training)
from ray_lightning_amd.optim import ShardedFusedAdam  # noqa: E402


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-xl",
                    choices=["gpt2", "gpt2-xl"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops._load_ext() is None:
        sys.exit("bench_clip needs a GPU and the built HIP extension")

    cfg = (GPT2Config.gpt2_xl() if args.model == "gpt2-xl"
           else GPT2Config.gpt2())
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = to_bf16_training(GPT2(cfg))
    params = list(model.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    grads = [p.grad for p in params]
    pristine = [g.clone() for g in grads]
    n_elem = sum(g.numel() for g in grads)
    n_bytes = sum(g.numel() * g.element_size() for g in grads)
    opt = ShardedFusedAdam(params, lr=1e-5, betas=(0.9, 0.95),
                           weight_decay=0.1)

    def path_a():
        torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        opt.step()

    def path_b():
        _, coef = ops.clip_coef(ops.grad_sumsq(grads), args.max_norm)
        opt.set_grad_scale(coef)
        opt.step()

    def path_c():
        ops.grad_sumsq(grads)

    # same inputs, same answer: compare the norms before timing
    ref = torch.stack(
        [g.double().pow(2).sum() for g in grads]).sum().sqrt()
    ours = ops.grad_sumsq(grads).sqrt()
    same = torch.equal(ops.grad_sumsq(grads), ops.grad_sumsq(grads))

    for fn in (path_a, path_b, path_c):  # warm up every path
        for _ in range(3):
            fn()
    torch._foreach_copy_(grads, pristine)
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.rounds):
        # (a) scales the shared grads in place: only its first iteration
        # of a round sees a norm above max_norm, later ones a coefficient
        # just under 1 (neither path branches on it, so the work is the
        # same). Put the grads back so (b) and (c) always see the
        # original norm, ~395x max_norm.
        ta.append(timed(path_a, args.iters))
        torch._foreach_copy_(grads, pristine)
        tb.append(timed(path_b, args.iters))
        tc.append(timed(path_c, args.iters))
    med = statistics.median
    print(json.dumps({
        "model": args.model, "tensors": len(grads), "grad_elems": n_elem,
        "grad_bytes": n_bytes,
        "norm_fp64": float(ref), "norm_hip": float(ours),
        "sumsq_bitwise_repeatable": same,
        "a_torch_clip_plus_step_ms": {"median": med(ta), "min": min(ta),
                                      "max": max(ta)},
        "b_hip_deferred_plus_step_ms": {"median": med(tb), "min": min(tb),
                                        "max": max(tb)},
        "c_sumsq_ms": {"median": med(tc), "min": min(tc), "max": max(tc)},
        "c_sumsq_GBps": n_bytes / (med(tc) * 1e-3) / 1e9,
        "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
