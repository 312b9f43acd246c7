"""Synchronized BatchNorm on the MI355X: the four HIP entry points
driven as fake ranks on one device, one rank against the plain kernels,
the C/V gate, and two processes sharing the device over gloo.

Reference (see sync_bn_common.py): one process, ``F.batch_norm`` on the
concatenation of the ranks' batches, in fp32 on the bf16-rounded input
(fp64 for fp32 input). Tolerances are those of test_fused_bn_gpu.py."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import fused_bn
from ray_lightning_amd.ops.fused_bn import FusedSyncBatchNorm2d

import sync_bn_common as sbc

BF16, FP32 = torch.bfloat16, torch.float32
TOL = {BF16: (5e-2, 5e-2), FP32: (1e-4, 1e-4)}
SUM_TOL = {BF16: (2e-1, 2e-2), FP32: (1e-3, 1e-4)}
STAT_TOL = (5e-2, 5e-2)

# name: (dtype, C, chunk batch sizes, H=W)
CASES = {
    # tpr=1, rpb=256, R far below one block
    "a": (BF16, 8, (3, 5), 3),
    # rpb=32, several blocks, ragged last block
    "b": (BF16, 64, (3, 5), 7),
    # rpb=1, fewer stage-1 blocks than kB2: fold2 gets empty slices
    "c": (BF16, 2048, (1, 1, 2), 2),
    # R=529 per chunk; the third holds R=1058 > kMaxStage1: grid cap and
    # the grid-stride loop
    "d": (BF16, 2048, (1, 1, 2), 23),
    # fp32 vector width
    "e": (FP32, 4, (2, 3), 5),
}


def _cuda(ts):
    return [None if t is None else t.cuda() for t in ts]


def _case(name, relu, with_res):
    dtype, c, ns, hw = CASES[name]
    xs, ress, dys, w, b = sbc.make_case(c, ns, hw, dtype, with_res)
    ref_dtype = torch.float32 if dtype == BF16 else torch.float64
    if relu:
        sbc.guard_relu_(xs, ress, dys, w, b, dtype=ref_dtype)
    ref = sbc.reference(xs, ress, dys, w, b, relu, dtype=ref_dtype)
    return dtype, (_cuda(xs), _cuda(ress), _cuda(dys), w.cuda(),
                   b.cuda()), ref


# ---------------------------------------------------------------------
# 5. entry points, fake ranks on one device
# ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("relu,with_res", sbc.FUSIONS, ids=sbc.FUSION_IDS)
def test_entry_points_fake_ranks(name, relu, with_res):
    dtype, args, ref = _case(name, relu, with_res)
    out = sbc.run_fake_ranks(sbc.ExtBackend(), *args, relu)
    torch.cuda.synchronize()
    sbc.check_against_reference(out, ref, TOL[dtype], SUM_TOL[dtype],
                                STAT_TOL)
    c = args[0][0].shape[1]
    for r, x in enumerate(args[0]):
        assert out["y"][r].dtype == dtype
        assert out["y"][r].is_contiguous(
            memory_format=torch.channels_last)
        assert out["mask"][r].numel() == \
            (x.numel() // (8 if dtype == BF16 else 4) if relu else 0)
        assert out["bsums"][r].shape == (2 * c,)
        assert torch.equal(out["mean"][r], out["mean"][0])
        assert torch.equal(out["running_var"][r], out["running_var"][0])


def test_entry_points_check_their_arguments():
    ext = _ops._load_ext()
    x = torch.randn(2, 64, 3, 3, device="cuda", dtype=BF16).contiguous(
        memory_format=torch.channels_last)
    sums = ext.fused_bn_sync_stats(x)
    assert sums.shape == (129,) and sums.dtype == FP32
    assert float(sums[128]) == 18.0
    w = torch.ones(64, device="cuda")
    b = torch.zeros(64, device="cuda")
    none = torch.Tensor()
    with pytest.raises(RuntimeError, match="power of two"):
        ext.fused_bn_sync_stats(torch.randn(
            2, 24, 3, 3, device="cuda", dtype=BF16).contiguous(
                memory_format=torch.channels_last))
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.fused_bn_sync_stats(torch.randn(2, 64, 3, 3, device="cuda",
                                            dtype=BF16))
    for bad in (sums[:-1], sums.double(), sums.cpu()):
        with pytest.raises(RuntimeError, match="sums must be fp32"):
            ext.fused_bn_sync_apply(x, bad, w, b, none, none, None, True,
                                    0.1, 1e-5)
    y, mean, invstd, mask = ext.fused_bn_sync_apply(
        x, sums, w, b, none, none, None, True, 0.1, 1e-5)
    bs = ext.fused_bn_sync_bwd_reduce(y, mask, x, mean, invstd, True)
    with pytest.raises(RuntimeError, match="fwd mask"):
        ext.fused_bn_sync_bwd_reduce(y, mask[:-1], x, mean, invstd, True)
    with pytest.raises(RuntimeError, match="bsums must be fp32"):
        ext.fused_bn_sync_bwd_dx(y, mask, x, mean, invstd, w, bs[:-1],
                                 sums[128:], True, False)
    with pytest.raises(RuntimeError, match="count must be fp32"):
        ext.fused_bn_sync_bwd_dx(y, mask, x, mean, invstd, w, bs,
                                 sums[127:], True, False)
    with pytest.raises(RuntimeError, match="bad gradient"):
        ext.fused_bn_sync_bwd_dx(y[:1], mask, x, mean, invstd, w, bs,
                                 sums[128:], True, False)


# ---------------------------------------------------------------------
# 6. one fake rank equals the plain kernels
# ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,n,hw", [(BF16, 64, 8, 7),
                                          (FP32, 4, 5, 5)])
@pytest.mark.parametrize("relu,with_res", sbc.FUSIONS, ids=sbc.FUSION_IDS)
def test_one_rank_equals_plain_kernels(dtype, c, n, hw, relu, with_res):
    ext = _ops._load_ext()
    xs, ress, dys, w, b = sbc.make_case(c, (n,), hw, dtype, with_res,
                                        device="cuda")
    out = sbc.run_fake_ranks(sbc.ExtBackend(), xs, ress, dys, w, b, relu)
    rm = torch.zeros(c, device="cuda")
    rv = torch.ones(c, device="cuda")
    y, mean, invstd, mask = ext.fused_bn_fwd(
        xs[0], w, b, rm, rv, ress[0], relu, True, sbc.MOMENTUM, sbc.EPS)
    outs = ext.fused_bn_bwd(dys[0], mask, xs[0], mean, invstd, w, relu,
                            with_res)
    sbc.close(out["mean"][0], mean, 1e-6, 1e-6, "mean")
    sbc.close(out["invstd"][0], invstd, 1e-6, 1e-6, "invstd")
    assert torch.equal(out["mask"][0], mask)
    sbc.close(out["y"][0], y, *TOL[dtype], "y")
    sbc.close(out["dx"][0], outs[0], *TOL[dtype], "dx")
    sbc.close(out["dgamma_sum"], outs[1], *SUM_TOL[dtype], "dgamma")
    sbc.close(out["dbeta_sum"], outs[2], *SUM_TOL[dtype], "dbeta")
    if with_res:
        sbc.close(out["dres"][0], outs[3], *TOL[dtype], "dres")
    sbc.close(out["running_mean"][0], rm, 1e-6, 1e-6, "running_mean")
    sbc.close(out["running_var"][0], rv, 1e-6, 1e-6, "running_var")


# ---------------------------------------------------------------------
# 7. the C/V gate
# ---------------------------------------------------------------------
class _NoopComm:
    world_size = 2
    rank = 0

    def all_reduce_(self, tensor, op="sum", async_op=False):
        pass


class _CountingExt:
    """The extension, counting calls of its sync-BN entry points."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if not name.startswith("fused_bn_"):
            return fn

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return counted


@pytest.mark.parametrize("c,engaged", [(24, False), (64, True)])
def test_gate_non_power_of_two_takes_the_twin(monkeypatch, c, engaged):
    counting = _CountingExt(_ops._load_ext())
    monkeypatch.setattr(fused_bn, "_load_ext", lambda: counting)
    xs, ress, dys, w, b = sbc.make_case(c, (4,), 5, BF16, True)
    sbc.guard_relu_(xs, ress, dys, w, b)
    ref = sbc.reference(xs, ress, dys, w, b, True, dtype=torch.float32)
    bn = FusedSyncBatchNorm2d(c, relu=True, comm=_NoopComm()).cuda()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    x = xs[0].cuda().requires_grad_()
    res = ress[0].cuda().requires_grad_()
    assert bn._kernel_ready(x) == engaged
    y = bn(x, res)
    y.backward(dys[0].cuda())
    torch.cuda.synchronize()
    want = {"fused_bn_sync_stats": 1, "fused_bn_sync_apply": 1,
            "fused_bn_sync_bwd_reduce": 1, "fused_bn_sync_bwd_dx": 1}
    assert counting.calls == (want if engaged else {})
    sbc.close(y, ref["y"][0], *TOL[BF16], "y")
    sbc.close(x.grad, ref["dx"][0], *TOL[BF16], "dx")
    sbc.close(res.grad, ref["dres"][0], *TOL[BF16], "dres")
    sbc.close(bn.weight.grad, ref["dgamma"], *SUM_TOL[BF16], "dgamma")
    sbc.close(bn.bias.grad, ref["dbeta"], *SUM_TOL[BF16], "dbeta")
    sbc.close(bn.running_mean, ref["running_mean"], *STAT_TOL, "rm")
    sbc.close(bn.running_var, ref["running_var"], *STAT_TOL, "rv")


# ---------------------------------------------------------------------
# 8. two processes sharing the device over gloo
# ---------------------------------------------------------------------
WORLD = 2
_NS = (3, 5)


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(11)
        self.conv = nn.Conv2d(3, 64, 3, padding=1, bias=False)
        self.bn = FusedSyncBatchNorm2d(64, relu=True)
        with torch.no_grad():
            self.bn.weight.uniform_(0.5, 1.5)
            self.bn.bias.normal_(0.0, 0.1)

    def forward(self, x):
        self.h = self.conv(x)
        self.h.retain_grad()  # what the BN layer hands back
        return self.bn(self.h)


def _rank_data(rank):
    g = torch.Generator().manual_seed(200 + rank)
    x = (torch.randn(_NS[rank], 3, 6, 6, generator=g) * (1.0 + rank) +
         rank).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(_NS[rank], 64, 6, 6, generator=g).to(BF16)
    return x, dy


def _ref_conv(net, x):
    """What the BN layer sees: the conv of the bf16-rounded image and
    weights, rounded to bf16 (straight-through for the gradient)."""
    wq = net.conv.weight + (net.conv.weight.to(BF16).float() -
                            net.conv.weight).detach()
    h = F.conv2d(x.to(BF16).float(), wq, padding=1)
    return h + (h.to(BF16).float() - h).detach()


def _all_rank_data():
    """Both ranks' (x, dy), dy zeroed where the ReLU's argument is within
    the tolerance on y of zero in the reference: the device conv and the
    reference conv round h differently, so there the ReLU's derivative is
    not determined to within a whole dy."""
    data = [_rank_data(r) for r in range(WORLD)]
    net = _Net()
    with torch.no_grad():
        h = _ref_conv(net, torch.cat([d[0] for d in data]))
        pre = F.batch_norm(h, None, None, net.bn.weight, net.bn.bias,
                           True, 0.0, sbc.EPS)
    keep = (pre.abs() >= TOL[BF16][0]).split(_NS)
    return [(x, dy * k.to(BF16)) for (x, dy), k in zip(data, keep)]


def _gpu_worker(rank, port, out_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        from ray_lightning_amd.engine.comm import (TorchDistCommunicator,
                                                   init_control_plane)
        from ray_lightning_amd.engine.ddp import NativeDDP
        init_control_plane(rank, WORLD)
        comm = TorchDistCommunicator()
        counting = _CountingExt(_ops._load_ext())
        fused_bn._load_ext = lambda: counting
        net = _Net().cuda().to(memory_format=torch.channels_last)
        net.bn.comm = comm
        ddp = NativeDDP(net, comm, bucket_cap_mb=0.0001)
        net.train()
        x, dy = _all_rank_data()[rank]
        with torch.autocast("cuda", BF16):
            y = net(x.cuda())
        (y.float() * dy.cuda().float()).sum().backward()
        ddp.finalize_backward()
        torch.cuda.synchronize()
        out = {k: v.detach().float().cpu().numpy()
               for k, v in net.state_dict().items()}
        out["y_is_bf16"] = y.dtype == BF16
        out["y"] = y.detach().float().cpu().numpy()
        out["h_is_nhwc_bf16"] = net.h.dtype == BF16 and net.h.is_contiguous(
            memory_format=torch.channels_last)
        out["dh"] = net.h.grad.float().cpu().numpy()
        for k, p in net.named_parameters():
            out["grad." + k] = p.grad.detach().float().cpu().numpy()
        out["calls"] = dict(counting.calls)
        out_q.put((rank, "ok", out))
    except BaseException as e:  # noqa: BLE001
        import traceback
        out_q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def _two_process_reference():
    """fp32, one process, on the concatenated batch."""
    net = _Net()
    data = _all_rank_data()
    dy = torch.cat([d[1] for d in data]).float()
    h = _ref_conv(net, torch.cat([d[0] for d in data]))
    h.retain_grad()
    rm, rv = torch.zeros(64), torch.ones(64)
    y = torch.relu(F.batch_norm(h, rm, rv, net.bn.weight, net.bn.bias,
                                True, sbc.MOMENTUM, sbc.EPS))
    (y * dy).sum().backward()
    return net, y.detach().split(_NS), h.grad.split(_NS), rm, rv


def test_two_processes_share_the_device_over_gloo():
    res = sbc.run_workers(_gpu_worker, WORLD)
    net, ys, dhs, rm, rv = _two_process_reference()
    failed = []

    def check(*args):  # every figure is printed before anything asserts
        try:
            sbc.close(*args)
        except AssertionError as e:
            failed.append(str(e))

    for rank in range(WORLD):
        got = res[rank]
        assert got["h_is_nhwc_bf16"] and got["y_is_bf16"]
        assert got["calls"] == {
            "fused_bn_sync_stats": 1, "fused_bn_sync_apply": 1,
            "fused_bn_sync_bwd_reduce": 1, "fused_bn_sync_bwd_dx": 1}
        check(torch.from_numpy(got["y"]), ys[rank], *TOL[BF16],
              f"rank {rank} y")
        check(torch.from_numpy(got["dh"]), dhs[rank], *TOL[BF16],
              f"rank {rank} dx of the BN layer")
        check(torch.from_numpy(got["bn.running_mean"]), rm, *STAT_TOL,
              f"rank {rank} running_mean")
        check(torch.from_numpy(got["bn.running_var"]), rv, *STAT_TOL,
              f"rank {rank} running_var")
        for k, p in net.named_parameters():
            # the engine averages: reference gradient / world size
            check(torch.from_numpy(got["grad." + k]), p.grad / WORLD,
                  *SUM_TOL[BF16], f"rank {rank} grad {k}")
    assert not failed, "\n".join(failed)
    for k in ("bn.running_mean", "bn.running_var"):
        assert (res[0][k] == res[1][k]).all(), k  # identical across ranks
