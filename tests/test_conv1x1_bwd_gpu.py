"""``conv1x1_bwd_data`` (csrc/conv1x1_bwd.hip) alone against a float64
reference from the same bf16 inputs, and ``resnet18_like`` with
``RLA_CONV1X1_BWD`` on against off in a process of its own.

Bound, from one RNE bf16 rounding of a fp32 sum of ``Cout + 1`` terms::

    |dx - e| <= 2^-8 |e| + (Cout + 2) 2^-23 (|dy| . |W| + |skip|)

elementwise, with ``e = dy.double() @ W.double() + skip.double()``."""
import functools
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_lightning_amd import ops as _ops  # noqa: E402
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import conv1x1  # noqa: E402
from ray_lightning_amd.ops.conv1x1 import (  # noqa: E402
    conv1x1_bwd_data, conv1x1_bwd_supported)

DEV = "cuda"
PAIRS = [(64, 64), (64, 256), (128, 512), (256, 1024), (512, 2048)]
# rows: below any tile, 98, one row tile + 1, three row tiles - 1
ROW_KINDS = ["r8", "r98", "tile+1", "3tiles-1"]


def _rows(kind, cout, cin):
    bm = _ops._load_ext().conv1x1_bwd_data_row_tile(cout, cin)
    assert bm > 0
    return {"r8": 8, "r98": 98, "tile+1": bm + 1,
            "3tiles-1": 3 * bm - 1}[kind]


def _nhw(rows):
    return {8: (2, 2, 2), 98: (2, 7, 7)}.get(rows, (1, 1, rows))


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _flat(t):
    """[N, C, H, W] -> [R, C] in NHWC row order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@functools.lru_cache(maxsize=None)
def _case(cout, cin, rows):
    """Inputs and the float64 pieces of the reference, made once per
    shape and left unchanged."""
    g = torch.Generator(device=DEV).manual_seed(cout * 7919 + cin + rows)
    n, h, w_ = _nhw(rows)
    dy = _cl(torch.randn(n, cout, h, w_, device=DEV, generator=g)
             .bfloat16())
    w = (torch.randn(cout, cin, 1, 1, device=DEV, generator=g)
         / cout ** 0.5).bfloat16()
    skip = _cl(torch.randn(n, cin, h, w_, device=DEV, generator=g)
               .bfloat16())
    w2 = w.view(cout, cin).double()
    prod = _flat(dy).double() @ w2
    absprod = _flat(dy).double().abs() @ w2.abs()
    return dy, w, skip, prod, absprod


def _check(dx, e, mag, cout, what):
    """The bound of the module docstring; ``mag`` = |dy|.|W| + |skip|."""
    assert dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    err = (_flat(dx).double() - e).abs()
    bound = 2.0 ** -8 * e.abs() + (cout + 2) * 2.0 ** -23 * mag
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"max (err - bound) {worst:.3e}")
    assert worst <= 0.0, what


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("cout,cin", PAIRS)
def test_against_float64(cout, cin, kind, with_skip):
    rows = _rows(kind, cout, cin)
    dy, w, skip, prod, absprod = _case(cout, cin, rows)
    if with_skip:
        assert conv1x1_bwd_supported(dy, w, skip)
        dx = conv1x1_bwd_data(dy, w, skip)
        s = _flat(skip).double()
        _check(dx, prod + s, absprod + s.abs(), cout, "with skip")
    else:
        assert conv1x1_bwd_supported(dy, w)
        dx = conv1x1_bwd_data(dy, w)
        _check(dx, prod, absprod, cout, "without skip")
    assert tuple(dx.shape) == (dy.shape[0], cin, dy.shape[2], dy.shape[3])


@pytest.mark.parametrize("cout,cin", PAIRS)
def test_cancellation(cout, cin):
    """skip = -bf16(dy . W): what is left is the rounding error of the
    product, far below a bf16 ulp of either addend. Two roundings would
    return zero or a whole ulp."""
    rows = _rows("tile+1", cout, cin)
    dy, w, _, prod, absprod = _case(cout, cin, rows)
    n, h, w_ = _nhw(rows)
    skip = _cl((-prod).to(torch.bfloat16).view(n, h, w_, cin)
               .permute(0, 3, 1, 2))
    dx = conv1x1_bwd_data(dy, w, skip)
    s = _flat(skip).double()
    _check(dx, prod + s, absprod + s.abs(), cout, "cancellation")


@pytest.mark.parametrize("cout,cin", PAIRS)
def test_zero_dy(cout, cin):
    rows = _rows("3tiles-1", cout, cin)
    dy, w, skip, _, _ = _case(cout, cin, rows)
    zero = torch.zeros_like(dy)
    assert torch.equal(conv1x1_bwd_data(zero, w, skip), skip)
    assert not conv1x1_bwd_data(zero, w).any()


@pytest.mark.parametrize("cout,cin", PAIRS)
def test_two_calls_bit_equal(cout, cin):
    rows = _rows("3tiles-1", cout, cin)
    dy, w, skip, _, _ = _case(cout, cin, rows)
    a = conv1x1_bwd_data(dy, w, skip)
    b = conv1x1_bwd_data(dy, w, skip)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_unsupported_shapes():
    dy = _cl(torch.randn(2, 64, 4, 4, device=DEV).bfloat16())
    w = torch.randn(64, 256, 1, 1, device=DEV).bfloat16()
    skip = _cl(torch.randn(2, 256, 4, 4, device=DEV).bfloat16())
    assert conv1x1_bwd_supported(dy, w, skip)
    # Cin = 96
    w96 = torch.randn(64, 96, 1, 1, device=DEV).bfloat16()
    assert not conv1x1_bwd_supported(dy, w96)
    with pytest.raises(RuntimeError):
        conv1x1_bwd_data(dy, w96)
    # fp32 tensors
    assert not conv1x1_bwd_supported(dy.float(), w.float())
    assert not conv1x1_bwd_supported(dy, w, skip.float())
    # NCHW-contiguous dy / skip
    assert not conv1x1_bwd_supported(dy.contiguous(), w)
    assert not conv1x1_bwd_supported(dy, w, skip.contiguous())
    # a skip of another shape, tensors on the CPU
    assert not conv1x1_bwd_supported(dy, w, skip[:1])
    assert not conv1x1_bwd_supported(dy.cpu(), w.cpu())


class _CountingExt:
    """The extension, counting calls of the new entry point."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def conv1x1_bwd_data(self, *args):
        self.calls += 1
        return self._ext.conv1x1_bwd_data(*args)


def _tols():
    """The project's bf16 elementwise tolerance (test_fused_bn_gpu.py)."""
    return dict(atol=5e-2, rtol=5e-2)


def _model_switch_check():
    """resnet18_like with RLA_CONV1X1_BWD on against off: the switch is
    read when a model is constructed."""
    from ray_lightning_amd.models.resnet import Bottleneck, resnet18_like
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    os.environ["RLA_CONV1X1_BWD"] = "1"
    on = resnet18_like(num_classes=10)
    os.environ["RLA_CONV1X1_BWD"] = "0"
    off = resnet18_like(num_classes=10)
    wired = [m._conv1_fork for m in on.modules()
             if isinstance(m, Bottleneck)]
    assert wired[0] and wired[1], "layers 1 and 2 must be wired"
    assert not any(m._conv1_fork for m in off.modules()
                   if isinstance(m, Bottleneck))
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

    counting = _CountingExt(_ops._load_ext())
    conv1x1._load_ext = lambda: counting

    x = torch.randn(2, 3, 64, 64, device=DEV).to(
        memory_format=torch.channels_last)
    t = torch.randint(0, 10, (2,), device=DEV)
    losses, calls = [], []
    for model in (on, off):
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(model(x).float(), t)
        loss.backward()
        losses.append(loss.detach())
        calls.append(counting.calls)
    assert calls == [sum(wired), sum(wired)], \
        f"kernel calls after on / off: {calls}, wired blocks {wired}"
    assert torch.equal(losses[0], losses[1]), "loss differs"
    for (name, p), q in zip(on.named_parameters(), off.parameters()):
        assert torch.allclose(p.grad, q.grad, **_tols()), name
    for (name, b), c in zip(on.named_buffers(), off.buffers()):
        assert torch.equal(b, c), name


def test_model_switch(tmp_path):
    """Model level, in a process of its own, with deterministic
    convolutions, MIOpen's per-process settings cleared and an empty
    find-db, for the reasons given at
    test_fused_bn_fusions_gpu.py::test_model_switch. Forward is the same
    convolution call either way, so loss and buffers are bit-equal; the
    parameter gradients differ by the one rounding saved per junction."""
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
