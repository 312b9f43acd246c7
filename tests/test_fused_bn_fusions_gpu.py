"""The stem BN+ReLU+maxpool and the downsample-junction dual-BN kernel
sets against the composed path they replace: two ``FusedBatchNorm2d``
calls plus ``F.max_pool2d`` / the residual form ``bn3(x3, bn_ds(xd))``,
same parameters, same process. Forward values must be bit-identical."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

# the fused path must be the one under test — fail loudly if the HIP
# extension did not load on a GPU box (no silent eager fallback)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops as _ops  # noqa: E402
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops.fused_bn import FusedBatchNorm2d  # noqa: E402

DEV = "cuda"


def _tols(dtype):
    """(elementwise, per-channel reduction) tolerances: those of
    test_fused_bn_gpu.py for bf16, atol=rtol=1e-4 for fp32."""
    if dtype == torch.bfloat16:
        return dict(atol=5e-2, rtol=5e-2), dict(atol=2e-1, rtol=2e-2)
    return dict(atol=1e-4, rtol=1e-4), dict(atol=1e-4, rtol=1e-4)


def _cl(t, dtype):
    return t.to(dtype).to(memory_format=torch.channels_last)


def _make_bn(C, relu, seed):
    torch.manual_seed(seed)
    bn = FusedBatchNorm2d(C, relu=relu).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    return bn.train()


def _same_stats(a, b):
    assert torch.equal(a.running_mean, b.running_mean)
    assert torch.equal(a.running_var, b.running_var)
    assert torch.equal(a.num_batches_tracked, b.num_batches_tracked)
    assert int(a.num_batches_tracked) == 1


def _check_stem(x0, dtype, bn=None):
    C = x0.shape[1]
    pool = nn.MaxPool2d(3, stride=2, padding=1)
    bn_f = bn if bn is not None else _make_bn(C, True, 0)
    bn_c = copy.deepcopy(bn_f)
    xf = _cl(x0, dtype).requires_grad_(True)
    xc = xf.detach().clone().requires_grad_(True)

    yf = bn_f.forward_pool(xf, pool)
    assert type(yf.grad_fn).__name__.startswith("_FusedBNReluPool"), \
        "the fused stem path did not engage"
    yc = F.max_pool2d(bn_c(xc), 3, stride=2, padding=1)
    assert yf.shape == yc.shape
    assert torch.equal(yf, yc), "pooled forward differs"
    _same_stats(bn_f, bn_c)

    torch.manual_seed(1)
    dy = torch.randn_like(yf)
    yf.backward(dy)
    yc.backward(dy)
    tol, rtol = _tols(dtype)
    assert torch.allclose(xf.grad.float(), xc.grad.float(), **tol), "dx"
    assert torch.allclose(bn_f.weight.grad, bn_c.weight.grad, **rtol), \
        "dgamma"
    assert torch.allclose(bn_f.bias.grad, bn_c.bias.grad, **rtol), "dbeta"
    return xf.grad, xc.grad, yf


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(2, 64, 10, 10), (2, 16, 9, 11)])
def test_stem_generic(dtype, shape):
    torch.manual_seed(0)
    _check_stem(torch.randn(*shape, device=DEV), dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(2, 64, 10, 10), (2, 16, 9, 11)])
def test_stem_ties(dtype, shape):
    """Small-integer inputs: positive ties inside a window and windows
    with no positive value are abundant. A wrong tie rule moves a whole
    gradient element to another position."""
    torch.manual_seed(0)
    x0 = torch.randint(-2, 3, shape, device=DEV).float()
    _, _, y = _check_stem(x0, dtype)
    # the case is only worth its name if both kinds of window occur
    assert (y == 0).any() and (y > 0).any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stem_all_dead(dtype):
    """beta far below zero: every BN output is negative, every window
    is dead, and dx must still equal the composed path's."""
    torch.manual_seed(0)
    bn = _make_bn(16, True, 0)
    with torch.no_grad():
        bn.bias.fill_(-100.0)
    x0 = torch.randint(-2, 3, (2, 16, 9, 11), device=DEV).float()
    gf, gc, y = _check_stem(x0, dtype, bn=bn)
    assert not y.any(), "every window was meant to be dead"
    assert torch.equal(gf, gc)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(4, 64, 7, 7), (2, 2048, 7, 7)])
def test_dual_bn(dtype, shape):
    C = shape[1]
    torch.manual_seed(0)
    x3f = _cl(torch.randn(*shape, device=DEV), dtype).requires_grad_(True)
    xdf = _cl(torch.randn(*shape, device=DEV) * 2 + 0.5,
              dtype).requires_grad_(True)
    x3c = x3f.detach().clone().requires_grad_(True)
    xdc = xdf.detach().clone().requires_grad_(True)
    bn3_f, bnd_f = _make_bn(C, True, 1), _make_bn(C, False, 2)
    bn3_c, bnd_c = copy.deepcopy(bn3_f), copy.deepcopy(bnd_f)

    yf = bn3_f.forward_dual(x3f, xdf, bnd_f)
    # fp32 vectors hold 4 channels, so C=2048 is beyond the kernels'
    # 256 vectors per row (as for fused_bn_fwd): that case must take
    # the composed path, every other one the fused path
    fused = type(yf.grad_fn).__name__.startswith("_FusedDualBN")
    assert fused == (C // (8 if dtype == torch.bfloat16 else 4) <= 256), \
        "the wrong dual path engaged"
    yc = bn3_c(x3c, bnd_c(xdc))
    assert torch.equal(yf, yc), "forward differs"
    _same_stats(bn3_f, bn3_c)
    _same_stats(bnd_f, bnd_c)

    torch.manual_seed(3)
    dy = torch.randn_like(yf)
    yf.backward(dy)
    yc.backward(dy)
    tol, rtol = _tols(dtype)
    assert torch.allclose(x3f.grad.float(), x3c.grad.float(), **tol), "dx3"
    assert torch.allclose(xdf.grad.float(), xdc.grad.float(), **tol), "dxd"
    for f, c, name in ((bn3_f, bn3_c, "bn3"), (bnd_f, bnd_c, "bn_ds")):
        assert torch.allclose(f.weight.grad, c.weight.grad, **rtol), \
            name + " dgamma"
        assert torch.allclose(f.bias.grad, c.bias.grad, **rtol), \
            name + " dbeta"


def _model_switch_check():
    """resnet18_like with RLA_BN_FUSIONS on against off: the switch is
    read when a model is constructed."""
    from ray_lightning_amd.models.resnet import resnet18_like
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    os.environ["RLA_BN_FUSIONS"] = "1"
    on = resnet18_like(num_classes=10)
    os.environ["RLA_BN_FUSIONS"] = "0"
    off = resnet18_like(num_classes=10)
    assert on._stem_pool and on.layer1[0]._dual_bn
    assert not off._stem_pool and not off.layer1[0]._dual_bn
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    # bn3.weight is zero-initialised; give every BN a real scale so the
    # main branch takes part
    with torch.no_grad():
        for m in on.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
    off.load_state_dict(on.state_dict())
    on = on.to(DEV).to(memory_format=torch.channels_last).train()
    off = off.to(DEV).to(memory_format=torch.channels_last).train()

    x = torch.randn(2, 3, 64, 64, device=DEV).to(
        memory_format=torch.channels_last)
    t = torch.randint(0, 10, (2,), device=DEV)
    losses = []
    for model in (on, off):
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(model(x).float(), t)
        loss.backward()
        losses.append(loss.detach())
    assert torch.equal(losses[0], losses[1]), "loss differs"
    tol, _ = _tols(torch.bfloat16)
    for (name, p), q in zip(on.named_parameters(), off.parameters()):
        assert torch.allclose(p.grad, q.grad, **tol), name
    for (name, b), c in zip(on.named_buffers(), off.buffers()):
        assert torch.equal(b, c), name


def test_model_switch(tmp_path):
    """Model level, in a process of its own. MIOpen's default choice
    for the stride-2 1x1 convolutions does not reproduce itself bit for
    bit (two switched-off copies with one state_dict gave losses 2.5e-3
    apart), so the convolutions run in deterministic mode: the
    bit-equality of the loss is then a statement about the BN kernels
    alone. Deterministic mode leaves MIOpen few solvers, and settings it
    reads once per process (other tests import bench.py, which turns
    the naive solvers off) can leave it none for the 7x7 stem
    convolution; hence the fresh process with those settings cleared
    and an empty find-db."""
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV")}
    env["MIOPEN_USER_DB_PATH"] = str(tmp_path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    _model_switch_check()
    print("model switch OK")
