"""Bit fingerprint of the ten fused-BN entry points of this build.

Fixed inputs are drawn on the CPU under ``torch.manual_seed``, moved to
the GPU and sent through every entry point; one line per returned tensor
(running stats included) carries the sha256 of its bytes. Two builds
whose outputs are equal line by line compute the same bits on these
cases: run the script once in a checkout of each and ``diff`` the two
outputs.

  a-e      the shapes of tests/test_sync_bn_gpu.py::CASES, first chunk:
           fused_bn_fwd / fused_bn_bwd in the three (relu, residual)
           fusions and in eval mode, and the four sync entry points as
           one rank
  pool     fused_bn_relu_pool_fwd / _bwd
  dual     fused_bn_dual_fwd / _bwd
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops  # noqa: E402

BF16, FP32 = torch.bfloat16, torch.float32
MOMENTUM, EPS = 0.1, 1e-5
FUSIONS = [("plain", False, False), ("relu", True, False),
           ("res_relu", True, True)]
# name: (dtype, N, C, H, W)
PLAIN = {"a": (BF16, 3, 8, 3, 3), "b": (BF16, 3, 64, 7, 7),
         "c": (BF16, 1, 2048, 2, 2), "d": (BF16, 1, 2048, 23, 23),
         "e": (FP32, 2, 4, 5, 5)}
POOL = [(dt, shape) for shape in ((2, 64, 10, 10), (2, 16, 9, 11))
        for dt in (BF16, FP32)]
DUAL = [(BF16, (4, 64, 7, 7)), (BF16, (2, 2048, 7, 7))]


def _nhwc(shape, dtype, scale=1.0, shift=0.0):
    t = torch.randn(*shape) * scale + shift
    return t.to(dtype).contiguous(memory_format=torch.channels_last).cuda()


def _affine(c):
    return ((0.5 + torch.rand(c)).cuda(), (0.1 * torch.randn(c)).cuda())


def _running(c):
    return torch.zeros(c).cuda(), torch.ones(c).cuda()


def emit(case, names, tensors):
    torch.cuda.synchronize()
    assert len(names) == len(tensors), (case, names, len(tensors))
    for name, t in zip(names, tensors):
        raw = t.detach().contiguous().view(torch.uint8).cpu().numpy()
        print(f"{case} {name} {tuple(t.shape)} "
              f"{hashlib.sha256(raw.tobytes()).hexdigest()}", flush=True)


def plain_and_sync(ext, name, dtype, shape):
    c = shape[1]
    x = _nhwc(shape, dtype, 1.5, 0.5)
    res = _nhwc(shape, dtype)
    dy = _nhwc(shape, dtype)
    w, b = _affine(c)
    for tag, relu, with_res in FUSIONS:
        r = res if with_res else None
        rm, rv = _running(c)
        y, mean, invstd, mask = ext.fused_bn_fwd(
            x, w, b, rm, rv, r, relu, True, MOMENTUM, EPS)
        emit(f"{name}.{tag}.fwd",
             ["y", "mean", "invstd", "mask", "running_mean", "running_var"],
             [y, mean, invstd, mask, rm, rv])
        outs = ext.fused_bn_bwd(dy, mask, x, mean, invstd, w, relu,
                                with_res)
        emit(f"{name}.{tag}.bwd",
             ["dx", "dgamma", "dbeta", "dres"][:len(outs)], outs)

        rm, rv = _running(c)
        sums = ext.fused_bn_sync_stats(x)
        y, mean, invstd, mask = ext.fused_bn_sync_apply(
            x, sums, w, b, rm, rv, r, relu, MOMENTUM, EPS)
        emit(f"{name}.{tag}.sync_fwd",
             ["sums", "y", "mean", "invstd", "mask", "running_mean",
              "running_var"], [sums, y, mean, invstd, mask, rm, rv])
        bsums = ext.fused_bn_sync_bwd_reduce(dy, mask, x, mean, invstd,
                                             relu)
        outs = ext.fused_bn_sync_bwd_dx(dy, mask, x, mean, invstd, w,
                                        bsums, sums[2 * c:], relu, with_res)
        emit(f"{name}.{tag}.sync_bwd", ["bsums", "dx", "dres"][:1 + len(outs)],
             [bsums] + list(outs))
    rm = torch.randn(c).cuda()
    rv = (0.5 + torch.rand(c)).cuda()
    y = ext.fused_bn_fwd(x, w, b, rm, rv, None, True, False, 0.0, EPS)[0]
    emit(f"{name}.eval", ["y", "running_mean", "running_var"], [y, rm, rv])


def pool(ext, dtype, shape):
    c = shape[1]
    case = f"pool.{'bf16' if dtype == BF16 else 'fp32'}.{shape}"
    x = _nhwc(shape, dtype, 1.5, 0.5)
    w, b = _affine(c)
    rm, rv = _running(c)
    pooled, mean, invstd, code = ext.fused_bn_relu_pool_fwd(
        x, w, b, rm, rv, MOMENTUM, EPS)
    emit(case + ".fwd",
         ["pooled", "mean", "invstd", "code", "running_mean", "running_var"],
         [pooled, mean, invstd, code, rm, rv])
    dpool = _nhwc(tuple(pooled.shape), dtype)
    outs = ext.fused_bn_relu_pool_bwd(dpool, code, x, mean, invstd, w)
    emit(case + ".bwd", ["dx", "dgamma", "dbeta"], outs)


def dual(ext, dtype, shape):
    c = shape[1]
    case = f"dual.bf16.{shape}"
    x3 = _nhwc(shape, dtype, 1.5, 0.5)
    xd = _nhwc(shape, dtype, 0.7, -0.3)
    dy = _nhwc(shape, dtype)
    w3, b3 = _affine(c)
    wd, bd = _affine(c)
    rm3, rv3 = _running(c)
    rmd, rvd = _running(c)
    y, mean3, invstd3, meand, invstdd, mask = ext.fused_bn_dual_fwd(
        x3, xd, w3, b3, rm3, rv3, wd, bd, rmd, rvd, MOMENTUM, 0.2, EPS,
        1e-3)
    emit(case + ".fwd",
         ["y", "mean3", "invstd3", "meand", "invstdd", "mask",
          "running_mean3", "running_var3", "running_meand", "running_vard"],
         [y, mean3, invstd3, meand, invstdd, mask, rm3, rv3, rmd, rvd])
    outs = ext.fused_bn_dual_bwd(dy, mask, x3, xd, mean3, invstd3, w3,
                                 meand, invstdd, wd)
    emit(case + ".bwd",
         ["dx3", "dxd", "dgamma3", "dbeta3", "dgammad", "dbetad"], outs)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    ext = ops._load_ext()
    assert ext is not None, "HIP extension not built"
    torch.manual_seed(20)
    for name, (dtype, *shape) in PLAIN.items():
        plain_and_sync(ext, name, dtype, tuple(shape))
    for dtype, shape in POOL:
        pool(ext, dtype, shape)
    for dtype, shape in DUAL:
        dual(ext, dtype, shape)


if __name__ == "__main__":
    main()
