"""Multi-token append over the KV cache on the CPU tier (fp32): the
torch twin of ``append_attention``, ``GPT2.forward(extend=True)`` and
``generate(prefill_chunk=)`` against the uncached forward."""
import math

import pytest
import torch

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
from ray_lightning_amd.ops.append_attn import append_attention
from ray_lightning_amd.ops.decode_attn import KVCache


def tiny_model(seed=0):
    torch.manual_seed(seed)
    return GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                           n_positions=128)).eval()


def tokens(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, T), generator=g)


@pytest.mark.parametrize("pos_list,max_pos", [([0, 13, 20], None),
                                              ([3, -1, 9], None),
                                              ([3, 20, 9], 15)])
def test_twin_against_explicit_softmax(pos_list, max_pos):
    B, H, Tmax, hs, T = len(pos_list), 2, 32, 64, 5
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, T, 3 * H * hs, generator=g)
    kc = torch.randn(B, H, Tmax, hs, generator=g)
    vc = torch.randn(B, H, Tmax, hs, generator=g)
    top = Tmax - T if max_pos is None else max_pos
    live = [0 <= p <= top for p in pos_list]
    for b, p in enumerate(pos_list):
        if live[b]:
            kc[b, :, p:] = math.nan
            vc[b, :, p:] = math.nan
    kc0, vc0 = kc.clone(), vc.clone()
    pos = torch.tensor(pos_list, dtype=torch.int32)
    o = append_attention(qkv, kc, vc, pos, max_pos=max_pos)
    q, k, v = qkv.view(B, T, 3, H, hs).unbind(2)          # [B, T, H, hs]
    for b, p in enumerate(pos_list):
        if not live[b]:                 # inactive: zeros, nothing moves
            assert torch.equal(o[b], torch.zeros_like(o[b]))
            assert torch.equal(kc[b], kc0[b]) and torch.equal(vc[b], vc0[b])
            continue
        for h in range(H):
            keys = torch.cat([kc0[b, h, :p], k[b, :, h]])
            vals = torch.cat([vc0[b, h, :p], v[b, :, h]])
            s = q[b, :, h] @ keys.T / math.sqrt(hs)
            s = s.masked_fill(torch.ones(T, p + T).triu(p + 1).bool(),
                              -math.inf)
            ref = torch.softmax(s, dim=-1) @ vals
            got = o[b, :, h * hs:(h + 1) * hs]
            assert (got - ref).abs().max().item() <= 1e-5
            # slots p .. p+T-1 hold the new rows, every other slot its bits
            assert torch.equal(kc[b, h, p:p + T], k[b, :, h])
            assert torch.equal(vc[b, h, p:p + T], v[b, :, h])
            for c, c0 in ((kc, kc0), (vc, vc0)):
                assert torch.equal(c[b, h, :p], c0[b, h, :p])
                assert torch.equal(c[b, h, p + T:].view(torch.int32),
                                   c0[b, h, p + T:].view(torch.int32))


def test_prefill_extend_decode_matches_the_full_forward():
    model, idx = tiny_model(), tokens(3, 20, 1)
    cache = KVCache(2, 3, 2, 32, 64, torch.float32, "cpu")
    with torch.no_grad():
        model(idx[:, :12], cache=cache)
        l_ext, _ = model(idx[:, 12:19], cache=cache, extend=True)
        assert cache.max_pos == 19 and cache.pos.tolist() == [19] * 3
        l_dec, _ = model(idx[:, 19:], cache=cache)
        full, _ = model(idx)
    assert cache.max_pos == 20 and cache.pos.tolist() == [20] * 3
    assert l_ext.shape == (3, 7, 256)
    assert (l_ext - full[:, 12:19]).abs().max().item() <= 1e-4
    assert (l_dec[:, 0] - full[:, 19]).abs().max().item() <= 1e-4


def test_ragged_turn_right_pads_then_sets_lengths():
    model, idx = tiny_model(1), tokens(2, 20, 2)
    turn = [7, 3]                       # row 1 appends 3 real tokens
    cache = KVCache(2, 2, 2, 32, 64, torch.float32, "cpu")
    with torch.no_grad():
        model(idx[:, :12], cache=cache)
        padded = idx[:, 12:19].clone()
        padded[1, 3:] = 0
        l_ext, _ = model(padded, cache=cache, extend=True)
        cache.set_lengths(torch.tensor([19, 15], dtype=torch.int32), 19)
        nxt = torch.stack([idx[0, 19], idx[1, 15]])[:, None]
        l_dec, _ = model(nxt, cache=cache)
        for b, n in enumerate(turn):
            full, _ = model(idx[b:b + 1, :12 + n + 1])
            assert (l_ext[b, :n] - full[0, 12:12 + n]).abs().max() <= 1e-4
            assert (l_dec[b, 0] - full[0, 12 + n]).abs().max() <= 1e-4
    assert cache.pos.tolist() == [20, 16] and cache.max_pos == 20


def test_generate_with_prefill_chunk_emits_the_same_tokens():
    model, idx = tiny_model(2), tokens(3, 12, 3)
    lens = [5, 1, 12]
    want, l0 = model.generate(idx, 16, prompt_lens=lens, temperature=0.0,
                              return_logits=True)
    got, l1 = model.generate(idx, 16, prompt_lens=lens, temperature=0.0,
                             return_logits=True, prefill_chunk=5)
    assert torch.equal(got, want)
    assert (l1 - l0).abs().max().item() <= 1e-4


def test_extend_needs_a_filled_cache_with_room():
    model, idx = tiny_model(), tokens(1, 30, 4)
    cache = KVCache(2, 1, 2, 32, 64, torch.float32, "cpu")
    with torch.no_grad():
        with pytest.raises(ValueError):
            model(idx[:, :4], cache=cache, extend=True)
        model(idx[:, :28], cache=cache)
        with pytest.raises(ValueError):
            model(idx[:, :5], cache=cache, extend=True)
        model(idx[:, 28:], cache=cache, extend=True)     # 28 + 2 fits 32
    assert cache.max_pos == 30
