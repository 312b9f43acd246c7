"""Shared pieces of the synchronized-BN tests (CPU and GPU tiers).

The reference everywhere is ONE process running ``F.batch_norm`` on the
concatenation of the ranks' batches, with loss = sum of the per-rank
losses: each rank's ``dx`` is the reference's slice, the sum of the
ranks' local ``dgamma``/``dbeta`` is the reference's, and the running
stats after one step are the reference's.

``run_fake_ranks`` drives the four phases (stats, apply, bwd_reduce,
bwd_dx) by hand over several chunks on one device and adds the chunks'
sums in Python where the communicator would all-reduce them.
"""
from __future__ import annotations

import multiprocessing as mp

import torch
import torch.nn.functional as F

from ray_lightning_amd.ops import fused_bn

EPS = 1e-5
MOMENTUM = 0.1

# (relu, with_residual): plain, ReLU, residual+ReLU
FUSIONS = [(False, False), (True, False), (True, True)]
FUSION_IDS = ["plain", "relu", "res_relu"]


class TwinBackend:
    """The torch twins of the four phases."""

    stats = staticmethod(fused_bn._twin_stats)
    apply = staticmethod(fused_bn._twin_apply)
    bwd_reduce = staticmethod(fused_bn._twin_bwd_reduce)

    @staticmethod
    def bwd_dx(dy, mask, x, mean, invstd, weight, bsums, count, relu,
               has_res):
        dx, d = fused_bn._twin_bwd_dx(dy, mask, x, mean, invstd, weight,
                                      bsums, count, relu)
        return (dx, d.to(x.dtype)) if has_res else (dx,)


class ExtBackend:
    """The HIP entry points of the four phases."""

    def __init__(self):
        self.ext = fused_bn._load_ext()
        assert self.ext is not None, "HIP extension not built"

    def stats(self, x):
        return self.ext.fused_bn_sync_stats(x)

    def apply(self, x, sums, weight, bias, rm, rv, res, relu, momentum,
              eps):
        return self.ext.fused_bn_sync_apply(x, sums, weight, bias, rm, rv,
                                            res, relu, momentum, eps)

    def bwd_reduce(self, dy, mask, x, mean, invstd, relu):
        return self.ext.fused_bn_sync_bwd_reduce(dy, mask, x, mean,
                                                 invstd, relu)

    def bwd_dx(self, *args):
        return tuple(self.ext.fused_bn_sync_bwd_dx(*args))


def make_case(c, ns, hw, dtype, with_res, device="cpu", seed=0):
    """Per-chunk inputs, residuals and upstream gradients
    (channels_last), plus fp32 gamma/beta. Inputs get a per-channel
    offset and scale so that mean and variance matter."""
    g = torch.Generator().manual_seed(seed)
    off = torch.randn(1, c, 1, 1, generator=g)
    amp = 0.5 + torch.rand(1, c, 1, 1, generator=g)

    def _t(n, kind):
        t = torch.randn(n, c, hw, hw, generator=g)
        if kind == "x":
            t = t * amp + off
        return t.to(device=device, dtype=dtype).contiguous(
            memory_format=torch.channels_last)

    xs = [_t(n, "x") for n in ns]
    ress = [_t(n, "r") for n in ns] if with_res else [None] * len(ns)
    dys = [_t(n, "d") for n in ns]
    weight = (0.5 + torch.rand(c, generator=g)).to(device)
    bias = (0.1 * torch.randn(c, generator=g)).to(device)
    return xs, ress, dys, weight, bias


def run_fake_ranks(be, xs, ress, dys, weight, bias, relu):
    c = xs[0].shape[1]
    dev = xs[0].device
    total = torch.stack([be.stats(x) for x in xs]).sum(0)
    count = total[2 * c:]
    fwd = []
    for x, res in zip(xs, ress):
        rm = torch.zeros(c, device=dev)
        rv = torch.ones(c, device=dev)
        y, mean, invstd, mask = be.apply(
            x, total.clone(), weight, bias, rm, rv, res, relu, MOMENTUM,
            EPS)
        fwd.append((y, mean, invstd, mask, rm, rv))
    bs = [be.bwd_reduce(dy, f[3], x, f[1], f[2], relu)
          for dy, x, f in zip(dys, xs, fwd)]
    btotal = torch.stack(bs).sum(0)
    has_res = ress[0] is not None
    bwd = [be.bwd_dx(dy, f[3], x, f[1], f[2], weight, btotal.clone(),
                     count, relu, has_res)
           for dy, x, f in zip(dys, xs, fwd)]
    return {
        "y": [f[0] for f in fwd], "mean": [f[1] for f in fwd],
        "invstd": [f[2] for f in fwd], "mask": [f[3] for f in fwd],
        "running_mean": [f[4] for f in fwd],
        "running_var": [f[5] for f in fwd],
        "dx": [b[0] for b in bwd],
        "dres": [b[1] for b in bwd] if has_res else None,
        "dbeta_sum": torch.stack([b[:c] for b in bs]).sum(0),
        "dgamma_sum": torch.stack([b[c:] for b in bs]).sum(0),
        "bsums": bs,
    }


def reference(xs, ress, dys, weight, bias, relu, dtype=torch.float64):
    """One process, ``F.batch_norm`` on the concatenated batch in
    ``dtype``, loss = sum over ranks of <y_r, dy_r>."""
    ns = [x.shape[0] for x in xs]
    x = torch.cat(xs).to(dtype).requires_grad_()
    res = None
    if ress[0] is not None:
        res = torch.cat(ress).to(dtype).requires_grad_()
    w = weight.to(dtype).requires_grad_()
    b = bias.to(dtype).requires_grad_()
    rm = torch.zeros_like(w).detach()
    rv = torch.ones_like(w).detach()
    y = F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS)
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    y.backward(torch.cat(dys).to(dtype))
    return {
        "y": list(y.detach().split(ns)), "dx": list(x.grad.split(ns)),
        "dres": list(res.grad.split(ns)) if res is not None else None,
        "dgamma": w.grad, "dbeta": b.grad, "running_mean": rm,
        "running_var": rv,
    }


def guard_relu_(xs, ress, dys, weight, bias, band=1e-3,
                dtype=torch.float32):
    """Zero the upstream gradient where the ReLU's argument lies within
    ``band`` of zero in the reference. There the derivative is decided
    by the last rounding of y, so kernel and reference may legitimately
    disagree by a whole ``dy``; with millions of elements a few such
    points are certain to exist."""
    x = torch.cat(xs).to(dtype)
    pre = F.batch_norm(x, None, None, weight.to(dtype), bias.to(dtype),
                       True, 0.0, EPS)
    if ress[0] is not None:
        pre = pre + torch.cat(ress).to(dtype)
    keep = (pre.abs() >= band).split([t.shape[0] for t in xs])
    for dy, k in zip(dys, keep):
        dy.mul_(k.to(dy.dtype))


def close(got, want, atol, rtol, what=""):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {got.shape}"
    err = (got - want).abs()
    over = err - (atol + rtol * want.abs())
    i = int(over.argmax())
    # the figures, also when the check passes (pytest shows them for a
    # failing test, or with -s)
    print(f"{what}: max abs err {float(err.max()):.3e}, worst margin "
          f"{float(-over.flatten()[i]):.3e} at reference value "
          f"{float(want.flatten()[i]):.3e} (max |reference| "
          f"{float(want.abs().max()):.3e}; atol {atol}, rtol {rtol})")
    assert bool((over <= 0).all()), (
        f"{what}: err {float(err.flatten()[i]):.3e} at reference value "
        f"{float(want.flatten()[i]):.3e} (atol {atol}, rtol {rtol})")


def check_against_reference(out, ref, tol, sum_tol, stat_tol):
    """tol / sum_tol / stat_tol: (atol, rtol) for y, dx, dres / for the
    channel sums dgamma, dbeta / for the running stats."""
    for r in range(len(out["y"])):
        close(out["y"][r], ref["y"][r], *tol, f"y[{r}]")
        close(out["dx"][r], ref["dx"][r], *tol, f"dx[{r}]")
        if ref["dres"] is not None:
            close(out["dres"][r], ref["dres"][r], *tol, f"dres[{r}]")
        close(out["running_mean"][r], ref["running_mean"], *stat_tol,
              f"running_mean[{r}]")
        close(out["running_var"][r], ref["running_var"], *stat_tol,
              f"running_var[{r}]")
    close(out["dgamma_sum"], ref["dgamma"], *sum_tol, "dgamma")
    close(out["dbeta_sum"], ref["dbeta"], *sum_tol, "dbeta")


# ---- spawned workers -------------------------------------------------
_MP = mp.get_context("spawn")


def run_workers(target, world, *args, timeout=180):
    """Start ``world`` processes running ``target(rank, port, *args,
    queue)``, collect one ``(rank, status, payload)`` each, join with a
    timeout and terminate whatever is left."""
    from ray_lightning_amd.util import find_free_port
    port = find_free_port()
    q = _MP.Queue()
    procs = [_MP.Process(target=target, args=(r, port) + args + (q,))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=timeout)
            assert status == "ok", f"rank {rank} failed:\n{payload}"
            results[rank] = payload
        for p in procs:
            p.join(30)
    finally:
        # after a failure the other rank may sit in a collective
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
    return results
