"""Time one residual-dropout site of GPT-2-XL, forward + backward, at
the shape it has in training (R = 16*1024 rows, C = 1600, bf16):

  (a) fused add+LayerNorm, no dropout               (the floor)
  (b) eager F.dropout(sub) then fused add+LayerNorm (without the new op)
  (c) fused dropout+add+LayerNorm                   (ops/fused_ln.py)

The three alternate in rounds on the same tensors; times are
device-event times per iteration. Bytes are what each path's kernels
must move by their own structure (N = R*C elements of 2 bytes):
forward reads sub, residual and writes x_new, y (4N); the dx kernel
reads dy, x_new, d_ext and writes dx (4N), plus d_sub for (c) (5N);
the dgamma/dbeta kernel reads dy and x_new again (2N). Eager dropout
adds read+write of sub and a 1-byte mask each way.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402
from ray_lightning_amd.ops.fused_ln import FusedLayerNorm  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16 * 1024)
    ap.add_argument("--cols", type=int, default=1600)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops._load_ext() is None:
        sys.exit("bench_dropout_ln needs a GPU and the built HIP extension")

    R, C, p = args.rows, args.cols, args.p
    torch.manual_seed(0)
    dev, bf = "cuda", torch.bfloat16
    ln = FusedLayerNorm(C).to(dev).float()
    sub = torch.randn(R, C, device=dev).to(bf).requires_grad_(True)
    res = torch.randn(R, C, device=dev).to(bf).requires_grad_(True)
    dy = torch.randn(R, C, device=dev).to(bf)
    dxn = torch.randn(R, C, device=dev).to(bf)
    leaves = [sub, res, ln.weight, ln.bias]

    def fwd_bwd(make):
        def run():
            x_new, y = make()
            return torch.autograd.grad([x_new, y], leaves, [dxn, dy])
        return run

    path_a = fwd_bwd(lambda: ln(sub, residual=res))
    path_b = fwd_bwd(lambda: ln(F.dropout(sub, p, True), residual=res))
    path_c = fwd_bwd(lambda: ln(sub, residual=res, dropout_p=p))

    # (c) drops what (b) drops: a fraction p of sub's gradient is zero
    check = {
        "b_d_sub_zero_fraction": float((path_b()[0] == 0).float().mean()),
        "c_d_sub_zero_fraction": float((path_c()[0] == 0).float().mean()),
    }

    for fn in (path_a, path_b, path_c):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.rounds):
        ta.append(timed(path_a, args.iters))
        tb.append(timed(path_b, args.iters))
        tc.append(timed(path_c, args.iters))

    n2 = R * C * 2
    bytes_a = 10 * n2
    bytes_c = 11 * n2
    # eager dropout: fwd r/w sub + 1-byte mask, bwd r/w grad + mask
    bytes_b = bytes_a + 4 * n2 + 2 * R * C

    def stats(t, nbytes):
        m = statistics.median(t)
        gbps = nbytes / (m * 1e-3) / 1e9
        return {"median_ms": m, "min_ms": min(t), "max_ms": max(t),
                "spread_ms": max(t) - min(t), "bytes": nbytes,
                "GBps": gbps,
                "of_achievable_hbm": gbps / HBM_ACHIEVABLE_GBPS}

    a, b, c = stats(ta, bytes_a), stats(tb, bytes_b), stats(tc, bytes_c)
    print(json.dumps({
        "rows": R, "cols": C, "p": p, "dtype": "bf16",
        "a_fused_add_ln": a, "b_eager_dropout_then_fused": b,
        "c_fused_dropout_add_ln": c,
        "c_over_b": c["median_ms"] / b["median_ms"],
        "c_over_a": c["median_ms"] / a["median_ms"],
        "c_over_a_expected_from_bytes": bytes_c / bytes_a,
        "c_beats_b_by_more_than_spread":
            b["median_ms"] - c["median_ms"] > max(b["spread_ms"],
                                                  c["spread_ms"]),
        "check": check,
        "rounds": args.rounds, "iters": args.iters,
        "hip": torch.version.hip,
    }))


if __name__ == "__main__":
    main()
