"""The fp8 KV cache's format, torch twins and generate(kv_fp8=True)."""
import math

import pytest
import torch

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config, to_bf16_training
from ray_lightning_amd.ops import append_attn as aa
from ray_lightning_amd.ops import decode_attn as da

BF16, FP8, HS = torch.bfloat16, torch.float8_e4m3fn, 64


def _rows(seed=0):
    """40 binades, a zero row, absmax on / under / over 448."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(40, HS, generator=g) * torch.exp2(
        torch.arange(40) - 20.0)[:, None]
    edge = torch.randn(3, HS, generator=g).clamp(-1, 1)
    edge[:, 0] = torch.tensor([448.0, 446.0, 450.0])
    return torch.cat([x, torch.zeros(1, HS), edge]).to(BF16)


def test_quantize_kv_round_trip_scale_and_idempotence():
    x = _rows()
    codes, scale = da.quantize_kv(x)
    assert codes.dtype == FP8 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:1]
    amax = x.float().abs().amax(dim=1)
    # a power of two, the smallest with absmax / scale <= 448
    assert torch.equal(torch.frexp(scale)[0], torch.full_like(scale, 0.5))
    assert (amax / scale <= 448).all()
    assert (amax / (scale / 2) > 448)[amax > 0].all()
    assert scale[40] == 1 and (codes[40].float() == 0).all()
    assert scale[41] == 1 and scale[42] == 1 and scale[43] == 2
    # within half an e4m3 step (2^-4 relative; subnormal step 2^-9)
    dq = da.dequantize_kv(codes, scale, torch.float32)
    step = torch.maximum(dq.abs() * 2.0 ** -4, scale[:, None] * 2.0 ** -10)
    assert ((dq - x.float()).abs() <= step).all()
    # exact in bf16; a fixed point in value, and in codes and scale unless
    # rounding took the absmax to 224 * scale (row 43: 450 / 2 -> 224)
    assert torch.equal(da.dequantize_kv(codes, scale).float(), dq)
    codes2, scale2 = da.quantize_kv(da.dequantize_kv(codes, scale))
    assert torch.equal(da.dequantize_kv(codes2, scale2).float(), dq)
    top = codes.float().abs().amax(dim=1)
    same = (top > 224) | (top == 0)
    assert same[:43].sum() >= 35 and not same[43]
    assert torch.equal(codes2[same].view(torch.uint8),
                       codes[same].view(torch.uint8))
    assert torch.equal(scale2[same], scale[same])
    assert torch.equal(scale2[~same], scale[~same] / 2)


def _fp8_case(B, H, Tmax, T, pos_list, seed):
    """fp8 caches, NaN code / NaN scales from each row's pos on."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * HS, generator=g).to(BF16)
    k8, ks = da.quantize_kv(torch.randn(B, H, Tmax, HS, generator=g).to(BF16))
    v8, vs = da.quantize_kv(torch.randn(B, H, Tmax, HS, generator=g).to(BF16))
    for b, p in enumerate(pos_list):
        p = max(p, 0)
        for c in (k8, v8):
            c.view(torch.uint8)[b, :, p:] = 0x7F
        ks[b, :, p:] = math.nan
        vs[b, :, p:] = math.nan
    pos = torch.tensor(pos_list, dtype=torch.int32)
    return qkv, k8, v8, ks, vs, pos


def _dequantized_qkv(qkv, H):
    B, T, _ = qkv.shape
    q, k, v = qkv.view(B, T, 3, H, HS).unbind(2)
    return torch.stack([q, da.dequantize_kv(*da.quantize_kv(k)),
                        da.dequantize_kv(*da.quantize_kv(v))],
                       dim=2).reshape(B, T, 3 * H * HS)


@pytest.mark.parametrize("T", [1, 5])
def test_twins_equal_the_bf16_twin_on_dequantized_values(T):
    """T = 1: decode, T = 5: append. Rows 1 and 3 are inactive."""
    B, H, Tmax, max_pos = 4, 2, 48, 30
    pos_list = [0, 40, 17, -1]
    qkv, k8, v8, ks, vs, pos = _fp8_case(B, H, Tmax, T, pos_list, T)
    before = [t.clone() for t in (k8, v8, ks, vs)]
    kb, vb = da.dequantize_kv(k8, ks), da.dequantize_kv(v8, vs)
    qd = _dequantized_qkv(qkv, H)
    if T == 1:
        out = da.decode_attention(qkv[:, 0], k8, v8, pos, max_pos,
                                  k_scale=ks, v_scale=vs)
        ref = da.decode_attention(qd[:, 0], kb, vb, pos, max_pos)
    else:
        out = aa.append_attention(qkv, k8, v8, pos, max_pos,
                                  k_scale=ks, v_scale=vs)
        ref = aa.append_attention(qd, kb, vb, pos, max_pos)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.isfinite(out).all() and (out[1] == 0).all() \
        and (out[3] == 0).all()
    # active rows store quantize_kv of their new rows; nothing else changes
    _, k, v = qkv.view(B, T, 3, H, HS).unbind(2)
    for cache, scale, new, c0, s0 in ((k8, ks, k, before[0], before[2]),
                                      (v8, vs, v, before[1], before[3])):
        want_c, want_s = c0.clone().view(torch.uint8), s0.clone()
        codes, s = da.quantize_kv(new.transpose(1, 2))
        for b in (0, 2):
            sl = slice(pos_list[b], pos_list[b] + T)
            want_c[b, :, sl] = codes[b].view(torch.uint8)
            want_s[b, :, sl] = s[b]
        assert torch.equal(cache.view(torch.uint8), want_c)
        assert torch.equal(scale.view(torch.int32), want_s.view(torch.int32))


def _tiny(dtype_bf16=True):
    torch.manual_seed(0)
    m = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=61,
                        n_positions=128)).eval()
    return to_bf16_training(m).eval() if dtype_bf16 else m


@pytest.mark.parametrize("kw", [{}, dict(prefill_chunk=4),
                                dict(draft_tokens=3, seed=1)],
                         ids=["plain", "prefill_chunk", "draft_tokens"])
def test_generate_kv_fp8_runs(kw, monkeypatch):
    """An fp8 cache with scales; prompts kept, tokens of the vocabulary."""
    m = _tiny()
    made = []
    monkeypatch.setattr(da, "KVCache", lambda *a, _f=da.KVCache:
                        (made.append(_f(*a)), made[-1])[1])
    idx = torch.randint(0, 61, (2, 9), generator=torch.Generator()
                        .manual_seed(2))
    out = m.generate(idx, 6, prompt_lens=[9, 4], temperature=0.0,
                     kv_fp8=True, **kw)
    cache = made[-1]
    assert cache.k[0].dtype == FP8 and cache.v_scale[0].dtype == torch.float32
    assert cache.k_scale[1].shape == cache.v[1].shape[:3]
    assert out.shape == (2, 15) and ((out >= 0) & (out < 61)).all()
    assert torch.equal(out[0, :9], idx[0, :9])
    assert torch.equal(out[1, :4], idx[1, :4])


def test_kv_fp8_needs_a_bf16_model_with_head_size_64():
    idx = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError):
        _tiny(dtype_bf16=False).generate(idx, 2, kv_fp8=True)
    torch.manual_seed(0)
    m = to_bf16_training(GPT2(GPT2Config(
        n_layer=1, n_embd=64, n_head=2, vocab_size=61, n_positions=64)))
    with pytest.raises(ValueError):
        m.generate(idx, 2, kv_fp8=True)
    from ray_lightning_amd.models.benchmark import GPT2LM
    with pytest.raises(ValueError):
        GPT2LM(gen_fp8_kv=True, bf16_weights=False)
