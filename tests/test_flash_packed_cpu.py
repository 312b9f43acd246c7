"""``flash_attention_qkvpacked`` without a GPU: the fallback (split,
transpose, ``flash_attention``) against fp32 torch, and its errors.

Tolerance: both sides are fp32 softmax attention on the same numbers in
a different reduction order, as in test_flash_docs_cpu.py, whose
``atol = rtol = 1e-5`` is used here."""
import pytest
import torch

from ray_lightning_amd.ops.flash_attn import (doc_bounds,
                                              flash_attention_qkvpacked)


@pytest.mark.parametrize("docs", [False, True])
def test_fallback_against_fp32(docs):
    B, H, T, hs = 2, 3, 40, 8       # T % 64 != 0: no kernel would take it
    C = H * hs
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, T, 3 * C, generator=g)
    ids = torch.randint(0, 3, (B, T), generator=g) if docs else None
    got = flash_attention_qkvpacked(qkv, H, doc_ids=ids)

    q, k, v = (t.view(B, T, H, hs).transpose(1, 2)
               for t in qkv.split(C, dim=2))
    pos = torch.arange(T)
    start = doc_bounds(ids)[0] if docs else torch.zeros(B, T)
    allowed = (pos[None, :] <= pos[:, None])[None] & \
        (pos[None, None, :] >= start[:, :, None])
    s = (q @ k.transpose(-1, -2)) / hs ** 0.5
    s = s.masked_fill(~allowed[:, None], float("-inf"))
    want = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
    assert got.shape == (B, T, C)
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("shape,n_head", [((2, 40, 100), 3),
                                          ((2, 3, 40, 72), 3)])
def test_value_errors(shape, n_head):
    with pytest.raises(ValueError):
        flash_attention_qkvpacked(torch.zeros(shape), n_head)
