"""``FusedBatchNorm2d.forward_pool`` / ``forward_dual`` off the GPU: both
take the composed path and equal plain torch BatchNorm + relu +
max_pool2d / add."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ray_lightning_amd.ops.fused_bn import FusedBatchNorm2d


def _pair(C, relu, seed):
    """A FusedBatchNorm2d and an nn.BatchNorm2d with the same state."""
    torch.manual_seed(seed)
    fused = FusedBatchNorm2d(C, relu=relu)
    with torch.no_grad():
        fused.weight.uniform_(0.5, 1.5)
        fused.bias.uniform_(-0.5, 0.5)
    ref = nn.BatchNorm2d(C)
    ref.load_state_dict(fused.state_dict())
    return fused.train(), ref.train()


def _same_state(a, b):
    for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(u, v), k


def test_forward_pool_cpu_matches_torch():
    fused, ref = _pair(8, True, 0)
    x = torch.randn(2, 8, 9, 11)
    pool = nn.MaxPool2d(3, stride=2, padding=1)
    y = fused.forward_pool(x, pool)
    y_ref = F.max_pool2d(torch.relu(ref(x)), 3, stride=2, padding=1)
    assert torch.equal(y, y_ref)
    _same_state(fused, ref)


def test_forward_pool_other_geometry_is_composed():
    """MaxPool2d(2, 2) is not the fused geometry: composed path, and
    the pooled shape is that pool's own."""
    fused, ref = _pair(8, True, 1)
    x = torch.randn(2, 8, 10, 10)
    y = fused.forward_pool(x, nn.MaxPool2d(2, 2))
    assert y.shape == (2, 8, 5, 5)
    assert torch.equal(y, F.max_pool2d(torch.relu(ref(x)), 2, 2))
    _same_state(fused, ref)


def test_pool_geometry_gate():
    from ray_lightning_amd.ops.fused_bn import _pool_is_3_2_1
    assert _pool_is_3_2_1(nn.MaxPool2d(3, stride=2, padding=1))
    assert _pool_is_3_2_1(nn.MaxPool2d((3, 3), (2, 2), (1, 1)))
    assert not _pool_is_3_2_1(nn.MaxPool2d(2, 2))
    assert not _pool_is_3_2_1(nn.MaxPool2d(3, stride=2, padding=1,
                                           ceil_mode=True))
    assert not _pool_is_3_2_1(nn.MaxPool2d(3, stride=2, padding=1,
                                           dilation=2))
    assert not _pool_is_3_2_1(nn.AvgPool2d(3, stride=2, padding=1))


def test_forward_dual_cpu_matches_torch():
    bn3, ref3 = _pair(8, True, 2)
    bnd, refd = _pair(8, False, 3)
    x3 = torch.randn(2, 8, 7, 7, requires_grad=True)
    xd = torch.randn(2, 8, 7, 7, requires_grad=True)
    y = bn3.forward_dual(x3, xd, bnd)
    y_ref = torch.relu(ref3(x3) + refd(xd))
    assert torch.equal(y, y_ref)
    _same_state(bn3, ref3)
    _same_state(bnd, refd)
    g3, gd = torch.autograd.grad(y.sum(), (x3, xd))
    r3, rd = torch.autograd.grad(y_ref.sum(), (x3, xd))
    assert torch.equal(g3, r3) and torch.equal(gd, rd)


def test_switch_is_read_at_construction(monkeypatch):
    from ray_lightning_amd.models.resnet import resnet18_like
    monkeypatch.setenv("RLA_BN_FUSIONS", "0")
    off = resnet18_like(num_classes=4)
    monkeypatch.delenv("RLA_BN_FUSIONS")
    on = resnet18_like(num_classes=4)
    assert not off._stem_pool and not off.layer1[0]._dual_bn
    assert on._stem_pool and on.layer1[0]._dual_bn
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off.load_state_dict(on.state_dict())
    x = torch.randn(2, 3, 32, 32)
    assert torch.equal(on.train()(x), off.train()(x))
