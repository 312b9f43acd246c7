"""Synchronized BatchNorm, CPU tier: the torch twins of the four
phases, ``convert_sync_batchnorm``, two ranks over gloo under NativeDDP,
and ``Trainer(sync_batchnorm=True)``.

Reference (see sync_bn_common.py): one process, ``F.batch_norm`` in fp64
on the concatenation of the ranks' batches. Tolerances are for fp32
arithmetic against that: 1e-5 absolute for y, dx and running stats
(values of order 1, a few fp32 roundings each), 1e-4/1e-4 for the
per-channel sums dgamma/dbeta (hundreds of terms, magnitudes up to
~100)."""
import copy
import os
import pickle
import warnings

import pytest
import torch
import torch.nn as nn

from ray_lightning_amd import LightningModule, RayStrategy, Trainer
from ray_lightning_amd.models.resnet import resnet18_like
from ray_lightning_amd.ops.fused_bn import (FusedBatchNorm2d,
                                            FusedSyncBatchNorm2d,
                                            convert_sync_batchnorm)

import sync_bn_common as sbc
from utils import get_trainer

WORLD = 2
TOL = (1e-5, 0.0)
SUM_TOL = (1e-4, 1e-4)


# ---------------------------------------------------------------------
# 1. the torch twins, fake ranks in one process
# ---------------------------------------------------------------------
@pytest.mark.parametrize("c,hw", [(8, 3), (64, 7)])
@pytest.mark.parametrize("relu,with_res", sbc.FUSIONS, ids=sbc.FUSION_IDS)
def test_twin_fake_ranks_match_reference(c, hw, relu, with_res):
    xs, ress, dys, w, b = sbc.make_case(c, (3, 5), hw, torch.float32,
                                        with_res)
    out = sbc.run_fake_ranks(sbc.TwinBackend, xs, ress, dys, w, b, relu)
    ref = sbc.reference(xs, ress, dys, w, b, relu)
    sbc.check_against_reference(out, ref, TOL, SUM_TOL, TOL)
    # every fake rank derived the same global statistics
    assert torch.equal(out["mean"][0], out["mean"][1])
    assert torch.equal(out["running_var"][0], out["running_var"][1])


# ---------------------------------------------------------------------
# 2. convert_sync_batchnorm
# ---------------------------------------------------------------------
class _FakeComm:
    """world_size 2, all_reduce_ leaves the tensor alone."""
    world_size = 2
    rank = 0

    def __init__(self):
        self.calls = 0

    def all_reduce_(self, tensor, op="sum", async_op=False):
        self.calls += 1


def _small_net():
    return nn.Sequential(
        nn.Conv2d(3, 8, 3, padding=1, bias=False),
        FusedBatchNorm2d(8, relu=True, eps=1e-3, momentum=0.2),
        nn.Conv2d(8, 8, 1, bias=False),
        nn.BatchNorm2d(8, affine=False))


def test_convert_keeps_parameter_and_buffer_objects():
    net = _small_net()
    net[1].eval()
    before = {k: v for k, v in list(net.named_parameters()) +
              list(net.named_buffers())}
    keys = list(net.state_dict().keys())
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    comm = _FakeComm()
    out = convert_sync_batchnorm(net, comm)
    assert out is net
    assert isinstance(net[1], FusedSyncBatchNorm2d)
    assert isinstance(net[3], FusedSyncBatchNorm2d)
    after = {k: v for k, v in list(net.named_parameters()) +
             list(net.named_buffers())}
    assert after.keys() == before.keys()
    for k in before:
        assert after[k] is before[k], k
    assert list(net.state_dict().keys()) == keys
    assert {id(p) for g in opt.param_groups for p in g["params"]} == \
        {id(p) for p in net.parameters()}
    assert net[1].relu is True and net[3].relu is False
    assert net[1].eps == 1e-3 and net[1].momentum == 0.2
    assert net[1].affine and not net[3].affine
    assert net[3].weight is None
    assert net[1].training is False and net[3].training is True
    assert net[1].comm is comm and net[3].comm is comm


def test_convert_is_idempotent():
    net = _small_net()
    comm = _FakeComm()
    convert_sync_batchnorm(net, comm)
    mods = list(net)
    other = _FakeComm()
    convert_sync_batchnorm(net, other)
    assert all(a is b for a, b in zip(mods, list(net)))
    assert net[1].comm is other  # rebound, not rebuilt


def test_convert_pickle_drops_comm_and_checkpoints_interchange():
    net = _small_net()
    plain_sd = copy.deepcopy(net.state_dict())
    convert_sync_batchnorm(net, _FakeComm())
    clone = pickle.loads(pickle.dumps(net))
    assert isinstance(clone[1], FusedSyncBatchNorm2d)
    assert clone[1].comm is None and clone[3].comm is None
    assert net[1].comm is not None  # the original keeps it
    for k, v in net.state_dict().items():
        assert torch.equal(clone.state_dict()[k], v)
    assert "comm" not in "".join(net.state_dict().keys())
    # checkpoints load both ways
    _small_net().load_state_dict(net.state_dict())
    net.load_state_dict(plain_sd)


def test_convert_leaves_bn1d_with_one_warning():
    net = nn.ModuleDict({
        "a": nn.BatchNorm2d(4), "b": nn.BatchNorm1d(4),
        "c": nn.Sequential(nn.BatchNorm3d(4))})
    bn1d, bn3d = net["b"], net["c"][0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        convert_sync_batchnorm(net, _FakeComm())
    assert len(rec) == 1
    msg = str(rec[0].message)
    assert "b (BatchNorm1d)" in msg and "c.0 (BatchNorm3d)" in msg
    assert net["b"] is bn1d and net["c"][0] is bn3d
    assert isinstance(net["a"], FusedSyncBatchNorm2d)


def test_sync_module_without_ranks_is_the_plain_module():
    """comm None, world size 1 and eval mode: FusedBatchNorm2d exactly,
    and no collective."""
    torch.manual_seed(0)
    x = torch.randn(4, 8, 3, 3)
    plain = FusedBatchNorm2d(8, relu=True)
    want = plain(x)

    class _One(_FakeComm):
        world_size = 1

    for comm in (None, _One()):
        m = FusedSyncBatchNorm2d(8, relu=True, comm=comm)
        assert torch.equal(m(x), want)
        assert torch.equal(m.running_mean, plain.running_mean)
        assert comm is None or comm.calls == 0
    comm = _FakeComm()
    m = FusedSyncBatchNorm2d(8, relu=True, comm=comm).eval()
    assert torch.equal(m(x), FusedBatchNorm2d(8, relu=True).eval()(x))
    assert comm.calls == 0


def test_training_forward_under_no_grad_still_synchronises():
    comm = _FakeComm()
    m = FusedSyncBatchNorm2d(8, comm=comm)
    with torch.no_grad():
        m(torch.randn(2, 8, 3, 3))
    assert comm.calls == 1
    assert int(m.num_batches_tracked) == 1


def test_converted_resnet_pool_and_dual_are_the_composed_forms():
    torch.manual_seed(0)
    net = resnet18_like(num_classes=4)
    for m in net.modules():  # zero-init would hide the bn3 branch
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
    comm = _FakeComm()
    convert_sync_batchnorm(net, comm)
    net.train()
    x = torch.randn(2, 64, 8, 8)
    a, b = copy.deepcopy(net.bn1), copy.deepcopy(net.bn1)
    a.comm = b.comm = comm
    assert torch.equal(a.forward_pool(x, net.maxpool), net.maxpool(b(x)))
    blk = net.layer1[0]
    assert blk._dual_bn
    h = torch.randn(2, 256, 4, 4)
    hd = torch.randn(2, 256, 4, 4)
    bn3a, bn3b = copy.deepcopy(blk.bn3), copy.deepcopy(blk.bn3)
    dsa, dsb = (copy.deepcopy(blk.downsample[1]),
                copy.deepcopy(blk.downsample[1]))
    for m in (bn3a, bn3b, dsa, dsb):
        m.comm = comm
    before = comm.calls
    got = bn3a.forward_dual(h, hd, dsa)
    assert comm.calls == before + 2  # both BNs went through forward
    assert torch.equal(got, bn3b(h, dsb(hd)))
    # and the whole converted model runs forward + backward
    net(torch.randn(2, 3, 32, 32)).sum().backward()
    assert all(p.grad is not None for p in net.parameters())


# ---------------------------------------------------------------------
# 3. world 2 over gloo, NativeDDP
# ---------------------------------------------------------------------
class _Net(nn.Module):
    """Conv -> BN+ReLU -> BN with the conv output as residual, + ReLU."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn1 = FusedBatchNorm2d(8, relu=True)
        self.bn2 = FusedBatchNorm2d(8, relu=True)

    def forward(self, x):
        h = self.conv(x)
        return self.bn2(self.bn1(h), h)


def _make_net():
    torch.manual_seed(7)
    net = _Net()
    with torch.no_grad():
        for bn in (net.bn1, net.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.1)
    return net


_NS = (3, 5)


def _rank_data(rank):
    g = torch.Generator().manual_seed(100 + rank)
    x = torch.randn(_NS[rank], 3, 6, 6, generator=g) * (1.0 + rank) + rank
    dy = torch.randn(_NS[rank], 8, 6, 6, generator=g)
    return x, dy


def _gloo_worker(rank, port, mode, out_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        from ray_lightning_amd.engine.comm import (TorchDistCommunicator,
                                                   init_control_plane)
        from ray_lightning_amd.engine.ddp import NativeDDP
        init_control_plane(rank, WORLD)
        comm = TorchDistCommunicator()
        net = _make_net()
        convert_sync_batchnorm(net, comm)
        ddp = NativeDDP(net, comm, bucket_cap_mb=0.0001)
        net.train()
        x, dy = _rank_data(rank)
        x.requires_grad_()
        if mode == "no_sync":
            with ddp.no_sync():
                y = net(x)
                (y * dy).sum().backward()
        else:
            y = net(x)
            (y * dy).sum().backward()
            ddp.finalize_backward()
        out = {k: v.detach().clone().numpy() for k, v in
               net.state_dict().items()}
        out["y"] = y.detach().numpy()
        out["dx"] = x.grad.numpy()
        for k, p in net.named_parameters():
            out["grad." + k] = p.grad.detach().clone().numpy()
        out_q.put((rank, "ok", out))
    except BaseException as e:  # noqa: BLE001
        import traceback
        out_q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def _net_reference():
    """The unconverted net in fp64 on the concatenated batch (CPU
    FusedBatchNorm2d is nn.BatchNorm2d.forward, i.e. F.batch_norm),
    loss = sum of the ranks' losses."""
    net = _make_net().double().train()
    data = [_rank_data(r) for r in range(WORLD)]
    x = torch.cat([d[0] for d in data]).double().requires_grad_()
    dy = torch.cat([d[1] for d in data]).double()
    y = net(x)
    (y * dy).sum().backward()
    return net, y.detach().split(_NS), x.grad.split(_NS)


def test_gloo_ddp_step_matches_reference():
    res = sbc.run_workers(_gloo_worker, WORLD, "ddp")
    net, ys, dxs = _net_reference()
    for rank in range(WORLD):
        got = res[rank]
        sbc.close(torch.from_numpy(got["y"]), ys[rank], *TOL, "y")
        sbc.close(torch.from_numpy(got["dx"]), dxs[rank], *TOL, "dx")
        for k, p in net.named_parameters():
            # the engine averages: reference gradient / world size
            sbc.close(torch.from_numpy(got["grad." + k]), p.grad / WORLD,
                      *SUM_TOL, "grad " + k)
        for k, b in net.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(got[k]) == 1
            else:
                sbc.close(torch.from_numpy(got[k]), b, *TOL, k)
    for k in res[0]:
        if "running_" in k:
            assert (res[0][k] == res[1][k]).all(), k  # bit-identical


def test_gloo_no_sync_still_synchronises_bn():
    res = sbc.run_workers(_gloo_worker, WORLD, "no_sync")
    _, ys, dxs = _net_reference()
    for rank in range(WORLD):
        sbc.close(torch.from_numpy(res[rank]["y"]), ys[rank], *TOL, "y")
        sbc.close(torch.from_numpy(res[rank]["dx"]), dxs[rank], *TOL,
                  "dx")


# ---------------------------------------------------------------------
# 4. Trainer(sync_batchnorm=...)
# ---------------------------------------------------------------------
class _Images(torch.utils.data.Dataset):
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        # sample-dependent offset: the two ranks' shards differ in mean
        self.data = torch.randn(32, 3, 4, 4, generator=g) + \
            torch.arange(32.0).view(32, 1, 1, 1) / 8

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i]


class _BNModule(LightningModule):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.conv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn = FusedBatchNorm2d(8, relu=True)
        self.head = nn.Linear(8, 2)

    def forward(self, x):
        return self.head(self.bn(self.conv(x)).mean((2, 3)))

    def training_step(self, batch, batch_idx):
        return self(batch).pow(2).mean()

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.05)

    def train_dataloader(self):
        return torch.utils.data.DataLoader(_Images(), batch_size=4)

    def on_train_end(self):
        rm = self.bn.running_mean.detach().cpu()
        hi = self.trainer.strategy.reduce(rm.clone(), op="max")
        lo = self.trainer.strategy.reduce(rm.clone(), op="min")
        self.log("bn_spread", (hi - lo).abs().max(), on_step=True,
                 on_epoch=False)
        n_sync = sum(isinstance(m, FusedSyncBatchNorm2d)
                     for m in self.modules())
        self.log("n_sync_bn", float(n_sync), on_step=True, on_epoch=False)


def _fit_two_workers(tmp_path, **kw):
    model = _BNModule()
    trainer = get_trainer(str(tmp_path), limit_train_batches=3,
                          checkpoint_callback=False,
                          strategy=RayStrategy(num_workers=2), **kw)
    trainer.fit(model)
    assert trainer.state.finished
    return trainer, model


def test_trainer_sync_batchnorm_equalises_running_stats(tmp_path):
    trainer, model = _fit_two_workers(tmp_path, sync_batchnorm=True)
    assert trainer.sync_batchnorm is True
    assert float(trainer.callback_metrics["n_sync_bn"]) == 1
    assert float(trainer.callback_metrics["bn_spread"]) == 0.0
    assert float(model.bn.running_mean.abs().max()) > 0  # it trained


def test_trainer_without_flag_leaves_per_rank_stats(tmp_path):
    """The control: the same run without the flag diverges."""
    trainer, _ = _fit_two_workers(tmp_path)
    assert float(trainer.callback_metrics["n_sync_bn"]) == 0
    assert float(trainer.callback_metrics["bn_spread"]) > 0.0


def test_trainer_flag_with_one_worker_converts_nothing(tmp_path):
    model = _BNModule()
    trainer = get_trainer(str(tmp_path), limit_train_batches=3,
                          checkpoint_callback=False, sync_batchnorm=True)
    trainer.fit(model)
    assert trainer.state.finished
    assert not any(isinstance(m, FusedSyncBatchNorm2d)
                   for m in model.modules())
    assert int(model.bn.num_batches_tracked) == 3


def test_trainer_flag_defaults_off():
    assert Trainer().sync_batchnorm is False
