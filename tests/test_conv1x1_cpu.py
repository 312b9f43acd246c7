"""``conv1x1_fork`` on the CPU (the composed path): against ``F.conv2d``
plus a second use of ``x``, in float64, and at model level with
``RLA_CONV1X1_BWD`` on against off."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_lightning_amd.ops.conv1x1 import (  # noqa: E402
    conv1x1_bwd_supported, conv1x1_fork)


def _inputs():
    torch.manual_seed(0)
    x = torch.randn(2, 6, 5, 4, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3, 6, 1, 1, dtype=torch.float64, requires_grad=True)
    return x, w


def _second_use(x):
    return (x * x).sum()  # gradient 2x, distinct from conv's


def _reference(with_skip):
    x, w = _inputs()
    out = F.conv2d(x, w)
    loss = (out * out).sum()
    if with_skip:
        loss = loss + _second_use(x)
    loss.backward()
    return out.detach(), x.grad, w.grad


def _forked(with_skip):
    x, w = _inputs()
    out, skip = conv1x1_fork(x, w)
    assert skip.data_ptr() == x.data_ptr(), "skip must alias x, not copy"
    loss = (out * out).sum()
    if with_skip:
        loss = loss + _second_use(skip)
    loss.backward()
    return out.detach(), x.grad, w.grad


@pytest.mark.parametrize("flag", ["1", "0"])
@pytest.mark.parametrize("with_skip", [True, False])
def test_fork_matches_conv2d(monkeypatch, flag, with_skip):
    monkeypatch.setenv("RLA_CONV1X1_BWD", flag)
    out_r, dx_r, dw_r = _reference(with_skip)
    out_f, dx_f, dw_f = _forked(with_skip)
    assert torch.equal(out_f, out_r)
    assert torch.equal(dw_f, dw_r)
    # a two-term float64 sum does not depend on the order of its terms
    assert torch.equal(dx_f, dx_r)


def test_only_skip_used():
    x, w = _inputs()
    _, skip = conv1x1_fork(x, w)
    _second_use(skip).backward()
    assert torch.equal(x.grad, 2 * x.detach())
    assert w.grad is None


def test_predicate_false_on_cpu():
    dy = torch.randn(2, 64, 4, 4).bfloat16().to(
        memory_format=torch.channels_last)
    w = torch.randn(64, 256, 1, 1).bfloat16()
    assert not conv1x1_bwd_supported(dy, w)


def test_rejects_other_kernels():
    with pytest.raises(ValueError):
        conv1x1_fork(torch.randn(1, 4, 8, 8), torch.randn(4, 4, 3, 3))


def _model(flag):
    from ray_lightning_amd.models.resnet import resnet18_like
    os.environ["RLA_CONV1X1_BWD"] = flag
    torch.manual_seed(0)
    return resnet18_like(num_classes=10)


def test_model_switch_cpu(monkeypatch):
    monkeypatch.setenv("RLA_CONV1X1_BWD", "1")  # restored afterwards
    on = _model("1")
    off = _model("0")
    assert all(b._conv1_fork for layer in (on.layer1, on.layer2)
               for b in layer)
    assert not any(b._conv1_fork for b in off.modules()
                   if hasattr(b, "_conv1_fork"))
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    with torch.no_grad():
        for m in on.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
    off.load_state_dict(on.state_dict())
    on.double().train()
    off.double().train()
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    t = torch.randint(0, 10, (2,))
    losses = []
    for model in (on, off):
        loss = F.cross_entropy(model(x), t)
        loss.backward()
        losses.append(loss.detach())
    assert torch.equal(losses[0], losses[1])
    for (name, p), q in zip(on.named_parameters(), off.parameters()):
        assert torch.equal(p.grad, q.grad), name
    for (name, b), c in zip(on.named_buffers(), off.buffers()):
        assert torch.equal(b, c), name
