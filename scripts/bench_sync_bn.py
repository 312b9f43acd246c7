"""Time what the split (synchronized) BN path costs over the plain fused
BN kernels of the same build, per ResNet-50 layer shape, forward +
backward, with communication taken out:

  (a) FusedBatchNorm2d       fused_bn_fwd / fused_bn_bwd
  (b) FusedSyncBatchNorm2d   stats -> [all-reduce] -> apply,
                             reduce -> [all-reduce] -> dx
      bound to a communicator of world size 2 whose all_reduce_ does
      nothing

(b) runs the same two passes over the activation per direction as (a);
it adds two per-channel kernels (the fold to [2C(+1)] and the
coefficient kernel now separate) and one [2C] clone per backward. The
table shows whether that is all it adds. The cost of a real all-reduce
across GPUs is NOT in these numbers.

The two alternate in rounds on the same tensors; times are device-event
times per iteration. One JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops.fused_bn import (FusedBatchNorm2d,  # noqa: E402
                                            FusedSyncBatchNorm2d)

# (C, H=W, relu, residual): the BN sites of ResNet-50 at 224x224
SHAPES = [
    (64, 112, True, False),    # stem
    (64, 56, True, False),     # layer1 bn1/bn2
    (256, 56, False, False),   # layer1 downsample
    (256, 56, True, True),     # layer1 bn3
    (128, 28, True, False),    # layer2 bn2
    (512, 28, True, True),     # layer2 bn3
    (256, 14, True, False),    # layer3 bn2
    (1024, 14, True, True),    # layer3 bn3
    (512, 7, True, False),     # layer4 bn2
    (2048, 7, True, True),     # layer4 bn3
]


class NoopComm:
    world_size = 2
    rank = 0

    def all_reduce_(self, tensor, op="sum", async_op=False):
        pass


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
    ap.add_argument("--batch", type=int, default=768,
                    help="per-GPU batch of bench.py's ResNet run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops._load_ext() is None:
        sys.exit("bench_sync_bn needs a GPU and the built HIP extension")

    dev, bf = "cuda", torch.bfloat16
    for c, hw, relu, with_res in SHAPES:
        torch.manual_seed(0)

        def _t():
            return torch.randn(args.batch, c, hw, hw, device=dev,
                               dtype=bf).contiguous(
                memory_format=torch.channels_last)

        x = _t().requires_grad_(True)
        res = _t().requires_grad_(True) if with_res else None
        dy = _t()
        plain = FusedBatchNorm2d(c, relu=relu).to(dev).train()
        sync = FusedSyncBatchNorm2d(c, relu=relu,
                                    comm=NoopComm()).to(dev).train()

        def fwd_bwd(bn):
            leaves = [x, bn.weight, bn.bias] + ([res] if with_res else [])

            def run():
                return torch.autograd.grad(bn(x, res), leaves, dy)
            return run

        path_a, path_b = fwd_bwd(plain), fwd_bwd(sync)
        ga, gb = path_a(), path_b()
        max_dx_diff = float((ga[0].float() - gb[0].float()).abs().max())
        del ga, gb
        for fn in (path_a, path_b):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(path_a, args.iters))
            tb.append(timed(path_b, args.iters))

        def stats(t):
            return {"median_ms": statistics.median(t), "min_ms": min(t),
                    "max_ms": max(t)}

        a, b = stats(ta), stats(tb)
        print(json.dumps({
            "C": c, "HW": hw, "batch": args.batch, "relu": relu,
            "residual": with_res, "dtype": "bf16",
            "a_plain": a, "b_split_noop_comm": b,
            "b_over_a": b["median_ms"] / a["median_ms"],
            "b_minus_a_us": 1e3 * (b["median_ms"] - a["median_ms"]),
            "max_dx_diff": max_dx_diff,
            "rounds": args.rounds, "iters": args.iters,
            "hip": torch.version.hip,
        }), flush=True)
        del x, res, dy


if __name__ == "__main__":
    main()
