"""``flash_attention``'s dropout argument off the GPU: validation and
the SDPA fallback."""
import pytest
import torch

from ray_lightning_amd.ops.flash_attn import flash_attention


def _qkv():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(1, 2, 16, 8, generator=g) for _ in range(3)]


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5])
def test_dropout_p_outside_unit_interval_raises(bad):
    q, k, v = _qkv()
    with pytest.raises(ValueError):
        flash_attention(q, k, v, dropout_p=bad)


def test_cpu_fallback_still_drops():
    q, k, v = _qkv()
    base = flash_attention(q, k, v)
    assert torch.equal(flash_attention(q, k, v, dropout_p=0.0), base)
    torch.manual_seed(1)
    a = flash_attention(q, k, v, dropout_p=0.5)
    assert not torch.equal(a, base)
    # row 0 attends to one key: it is either dropped (0) or doubled
    r0 = a[0, 0, 0]
    assert torch.equal(r0, torch.zeros_like(r0)) or torch.allclose(
        r0, 2 * base[0, 0, 0])
    torch.manual_seed(1)
    assert torch.equal(flash_attention(q, k, v, dropout_p=0.5), a)
