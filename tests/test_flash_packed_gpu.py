"""Packed-QKV flash attention (``flash_attention_qkvpacked`` and the
PACKED instantiations of the v3 kernels behind it): against fp32 torch,
bit for bit against the unpacked kernels, through GPT-2, and the host
checks of the forward entry point."""
import math

import pytest
import torch

from ray_lightning_amd.ops import flash_attn as fa

pytestmark = pytest.mark.gpu
HS = 64
SCALE = 1.0 / math.sqrt(HS)


def _slots(qkv, H):
    """q, k, v as [B, H, T, 64] views of qkv [B, T, 3C]."""
    B, T, _ = qkv.shape
    return [t.view(B, T, H, HS).transpose(1, 2)
            for t in qkv.split(H * HS, dim=2)]


def _rows(t):
    """[B, H, T, 64] -> [B, T, C]."""
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B, T, H * HS)


@pytest.mark.parametrize("B,H,T", [(1, 1, 64), (2, 3, 128), (1, 2, 256)])
def test_packed_against_fp32(B, H, T):
    ext = fa._load_ext()
    torch.manual_seed(3)
    C = H * HS
    qkv = (torch.randn(B, T, 3 * C, device="cuda") * 0.5).bfloat16()
    dy = (torch.randn(B, T, C, device="cuda") * 0.5).bfloat16()
    o, lse, _, _ = ext.flash_attn_fwd_v3_packed(qkv, H, SCALE, 0.0)
    dqkv = ext.flash_attn_bwd_v3_packed(dy, qkv, o, lse, H, SCALE, 0.0,
                                        0, 0)

    ref_in = qkv.float().requires_grad_(True)
    q, k, v = _slots(ref_in, H)
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(torch.ones(T, T, device="cuda").triu(1).bool(),
                      float("-inf"))
    ref = _rows(torch.softmax(s, -1) @ v)
    ref.backward(dy.float())

    assert o.shape == (B, T, C) and dqkv.shape == qkv.shape
    assert torch.allclose(lse, torch.logsumexp(s, -1), atol=2e-3,
                          rtol=1e-3)
    assert torch.allclose(o.float(), ref, atol=3e-2, rtol=3e-2)
    err = (dqkv.float() - ref_in.grad).abs()     # the whole of dqkv
    for i, name in enumerate(("dq", "dk", "dv")):
        e = err[:, :, i * C:(i + 1) * C].max().item()
        assert e < 2e-2 * math.sqrt(T / 64), f"{name} max err {e}"


def _mixed_ids(B, T):
    """Row 0: documents beginning at 1, 64, 100 and 255; the other rows
    at 64 and 255."""
    pos = torch.arange(T, device="cuda")
    ids = torch.stack([sum((pos >= b).long() for b in bounds)
                       for bounds in [(1, 64, 100, 255)] +
                       [(64, 255)] * (B - 1)])
    return ids


@pytest.mark.parametrize("docs", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_packed_same_bits_as_unpacked(p, docs, monkeypatch):
    monkeypatch.setenv("RLA_FLASH_PACKED", "1")
    B, H, T = 2, 3, 256
    C = H * HS
    torch.manual_seed(5)
    qkv = (torch.randn(B, T, 3 * C, device="cuda") * 0.5).bfloat16()
    dy = (torch.randn(B, T, C, device="cuda") * 0.5).bfloat16()
    ids = _mixed_ids(B, T) if docs else None

    qkv_p = qkv.clone().requires_grad_(True)
    torch.manual_seed(7)
    o_p = fa.flash_attention_qkvpacked(qkv_p, H, dropout_p=p, doc_ids=ids)
    assert o_p.grad_fn.name().startswith("_FlashAttnPacked")
    o_p.backward(dy)

    q, k, v = (t.contiguous().requires_grad_(True)
               for t in _slots(qkv, H))
    torch.manual_seed(7)
    o_u = fa.flash_attention(q, k, v, dropout_p=p, doc_ids=ids)
    o_u.backward(dy.view(B, T, H, HS).transpose(1, 2))

    assert torch.equal(o_p, _rows(o_u))
    want = torch.cat([_rows(g) for g in (q.grad, k.grad, v.grad)], dim=2)
    assert torch.equal(qkv_p.grad, want)


def test_gpt2_same_with_and_without_packed(monkeypatch):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    torch.manual_seed(2)
    cfg = GPT2Config(vocab_size=503, n_positions=128, n_embd=128,
                     n_layer=2, n_head=2)
    model = to_bf16_training(GPT2(cfg).cuda())
    idx = torch.randint(0, 503, (2, 128), device="cuda")
    tgt = torch.randint(0, 503, (2, 128), device="cuda")
    out = {}
    for gate in ("1", "0"):
        monkeypatch.setenv("RLA_FLASH_PACKED", gate)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(4)
        _, loss = model(idx, tgt)
        loss.backward()
        out[gate] = (loss.detach().clone(),
                     {n: p.grad.clone()
                      for n, p in model.named_parameters()})
    assert torch.equal(out["1"][0], out["0"][0])
    for n, g in out["1"][1].items():
        assert torch.equal(g, out["0"][1][n]), n


@pytest.mark.parametrize("make", [
    lambda: torch.zeros(1, 64, 2 * 192, device="cuda",
                        dtype=torch.bfloat16)[:, :, ::2],    # strided
    lambda: torch.zeros(1, 96, 192, device="cuda", dtype=torch.bfloat16),
    lambda: torch.zeros(1, 64, 96, device="cuda", dtype=torch.bfloat16),
    lambda: torch.zeros(1, 64, 192, device="cuda"),          # float32
], ids=["strided", "T96", "hs32", "float32"])
def test_packed_forward_host_checks(make):
    with pytest.raises(RuntimeError):
        fa._load_ext().flash_attn_fwd_v3_packed(make(), 1, SCALE, 0.0)
