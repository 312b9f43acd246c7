"""GPT-2 generation on the CPU tier (fp32): the decode-attention twin,
greedy decoding with the KV cache against the uncached forward,
sampling, EOS handling, the edges, and Trainer.predict."""
import math

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
from ray_lightning_amd.ops.decode_attn import KVCache, decode_attention

LENS = [5, 1, 12]
P = 12
NEW = 32


def tiny_cfg():
    return GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                      n_positions=128)


def make(seed):
    torch.manual_seed(seed)
    model = GPT2(tiny_cfg())
    g = torch.Generator().manual_seed(100 + seed)
    idx = torch.randint(0, 256, (3, P), generator=g)
    return model, idx


_greedy_cache = {}


def greedy(seed):
    """(model, idx, tokens, logits) of the greedy run, computed once."""
    if seed not in _greedy_cache:
        model, idx = make(seed)
        out, logits = model.generate(idx, NEW, prompt_lens=LENS,
                                     temperature=0.0, return_logits=True)
        _greedy_cache[seed] = (model, idx, out, logits)
    return _greedy_cache[seed]


# ------------------------------------------------------------------ twin
def _twin_case(pos_list, max_pos=None):
    B, H, Tmax, hs = len(pos_list), 2, 32, 64
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, 3 * H * hs, generator=g)
    kc = torch.randn(B, H, Tmax, hs, generator=g)
    vc = torch.randn(B, H, Tmax, hs, generator=g)
    pos = torch.tensor(pos_list, dtype=torch.int32)
    for b, p in enumerate(pos_list):
        if 0 <= p < Tmax:
            kc[b, :, p:] = math.nan
            vc[b, :, p:] = math.nan
    return qkv, kc, vc, pos


def _explicit(qkv, kc, vc, pos_list):
    B, H, Tmax, hs = kc.shape
    q, k, v = qkv.view(B, 3, H, hs).unbind(1)
    out = torch.zeros(B, H, hs)
    for b, p in enumerate(pos_list):
        for h in range(H):
            keys = torch.cat([kc[b, h, :p], k[b, h][None]])
            vals = torch.cat([vc[b, h, :p], v[b, h][None]])
            w = torch.softmax(keys @ q[b, h] / math.sqrt(hs), dim=0)
            out[b, h] = w @ vals
    return out.reshape(B, H * hs)


def test_twin_matches_explicit_softmax_and_appends():
    pos_list = [0, 13, 31]
    qkv, kc, vc, pos = _twin_case(pos_list)
    kc0, vc0 = kc.clone(), vc.clone()
    o = decode_attention(qkv, kc, vc, pos)
    assert torch.isfinite(o).all()
    ref = _explicit(qkv, kc0, vc0, pos_list)
    assert (o - ref).abs().max().item() <= 1e-5
    B, H, Tmax, hs = kc.shape
    k_new, v_new = qkv.view(B, 3, H, hs)[:, 1], qkv.view(B, 3, H, hs)[:, 2]
    for cache, before, new in ((kc, kc0, k_new), (vc, vc0, v_new)):
        changed = (cache.view(torch.int32) != before.view(torch.int32)) \
            .any(dim=3).any(dim=1)                      # [B, Tmax]
        want = torch.zeros(B, Tmax, dtype=torch.bool)
        for b, p in enumerate(pos_list):
            want[b, p] = True
            assert torch.equal(cache[b, :, p].view(torch.int32),
                               new[b].contiguous().view(torch.int32))
        assert torch.equal(changed, want)


@pytest.mark.parametrize("bad,max_pos", [(-1, None), (20, 15)])
def test_twin_inactive_row(bad, max_pos):
    pos_list = [3, bad, 9]
    qkv, kc, vc, pos = _twin_case(pos_list)
    kc[1], vc[1] = 1.5, -2.5      # row 1 is inactive: nothing in it moves
    kc0, vc0 = kc.clone(), vc.clone()
    o = decode_attention(qkv, kc, vc, pos, max_pos=max_pos)
    assert torch.equal(o[1], torch.zeros_like(o[1]))
    assert torch.equal(kc[1], kc0[1]) and torch.equal(vc[1], vc0[1])
    ref = _explicit(qkv, kc0, vc0, [3, 0, 9])
    for b in (0, 2):
        assert (o[b] - ref[b]).abs().max().item() <= 1e-5


# ------------------------------------------- greedy: cached == uncached
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_greedy_with_cache_equals_without(seed):
    model, idx, out, logits = greedy(seed)
    model.eval()
    checked = 0
    for b, n in enumerate(LENS):
        seq = out[b, :n + NEW][None]
        with torch.no_grad():
            full, _ = model(seq)
        # the logits that produced the token at position n + s
        ref = full[0, n - 1:n - 1 + NEW].float()
        err = (logits[b] - ref).abs().max().item()
        assert err <= 1e-4, (b, err)
        top2 = ref.topk(2, dim=-1).values
        margin = top2[:, 0] - top2[:, 1]
        assert margin.min().item() > 1e-3, \
            f"row {b}: a step would be left out (margin {margin.min()})"
        assert torch.equal(out[b, n:n + NEW], ref.argmax(dim=-1))
        checked += NEW
    assert checked == 96


def test_output_layout():
    model, idx, out, _ = greedy(0)
    assert out.shape == (3, P + NEW)
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :n], idx[b, :n])
        assert (out[b, n + NEW:] == 0).all()


# -------------------------------------------------------------- sampling
def test_top_k_1_is_greedy():
    model, idx, out, _ = greedy(0)
    g = torch.Generator().manual_seed(3)
    got = model.generate(idx, NEW, prompt_lens=LENS, temperature=1.0,
                         top_k=1, generator=g)
    assert torch.equal(got, out)


def test_top_k_5_and_seeds():
    model, idx, _, _ = greedy(0)

    def run(seed):
        g = torch.Generator().manual_seed(seed)
        return model.generate(idx, NEW, prompt_lens=LENS, temperature=1.0,
                              top_k=5, generator=g, return_logits=True)

    out, logits = run(11)
    top5 = logits.topk(5, dim=-1).indices            # [B, NEW, 5]
    for b, n in enumerate(LENS):
        tok = out[b, n:n + NEW]
        assert (top5[b] == tok[:, None]).any(dim=-1).all()
    again, _ = run(11)
    assert torch.equal(again, out)
    other, _ = run(12)
    assert not torch.equal(other, out)


# ------------------------------------------------------------------- EOS
def test_eos_pads_one_row_and_leaves_the_others():
    # greedy on a random-init model mostly repeats itself; at seed 2 one
    # row changes its token a few steps in
    model, idx, _, _ = greedy(2)
    pad = 255
    base = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0,
                          pad_token_id=pad)
    new = [base[b, n:n + NEW] for b, n in enumerate(LENS)]
    pick = None
    for b in range(3):
        others = torch.cat([new[o] for o in range(3) if o != b])
        for s in range(1, NEW - 1):
            t = int(new[b][s])
            first = int((new[b] == t).nonzero()[0])
            if t != pad and first >= 2 and not (others == t).any():
                pick = (b, first, t)
                break
        if pick:
            break
    assert pick is not None, "no token is emitted by one row only"
    row, first, eos = pick
    got = model.generate(idx, NEW, prompt_lens=LENS, temperature=0.0,
                         eos_token_id=eos, pad_token_id=pad)
    want = base.clone()
    want[row, LENS[row] + first + 1:] = pad
    assert torch.equal(got, want)


def test_eos_everywhere_stops_early():
    model, idx, out, _ = greedy(0)
    # the only row finishes at its first token: the look the loop takes
    # every 16 steps ends it early, and the rest is padding all the same
    eos = int(out[0, LENS[0]])
    got = model.generate(idx[:1], NEW, prompt_lens=LENS[:1],
                         temperature=0.0, eos_token_id=eos, pad_token_id=7)
    assert int(got[0, LENS[0]]) == eos
    assert (got[0, LENS[0] + 1:] == 7).all()


# ----------------------------------------------------------------- edges
def test_max_new_tokens_0_and_1():
    model, idx, out, logits = greedy(0)
    full = torch.randint(0, 256, (2, 9))
    assert torch.equal(model.generate(full, 0), full)
    one, l1 = model.generate(idx, 1, prompt_lens=LENS, temperature=0.0,
                             return_logits=True)
    assert one.shape == (3, P + 1) and l1.shape == (3, 1, 256)
    for b, n in enumerate(LENS):
        assert int(one[b, n]) == int(out[b, n])
    assert (l1[:, 0] - logits[:, 0]).abs().max().item() <= 1e-5


def test_last_position_is_used():
    model, _ = make(1)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 256, (2, 96), generator=g)
    out, logits = model.generate(idx, 32, temperature=0.0,
                                 return_logits=True)
    assert out.shape == (2, 128)
    model.eval()
    with torch.no_grad():
        full, _ = model(out)
    ref = full[:, 95:127].float()
    assert (logits - ref).abs().max().item() <= 1e-4
    assert torch.equal(out[:, 96:], ref.argmax(dim=-1))


def test_validation_errors():
    model, idx = make(0)
    with pytest.raises(ValueError):
        model.generate(torch.zeros(1, 100, dtype=torch.long), 29)
    with pytest.raises(ValueError):
        model.generate(idx, 4, prompt_lens=[0, 3, 3])
    with pytest.raises(ValueError):
        model.generate(idx, 4, prompt_lens=[3, 13, 3])
    with pytest.raises(ValueError):
        model.generate(idx, 4, prompt_lens=[3, 3])
    # the longest prompt counts, not the padded width
    model.generate(torch.zeros(1, 100, dtype=torch.long), 29,
                   prompt_lens=[99])


def test_training_mode_is_restored():
    model, idx = make(0)
    model.train()
    model.generate(idx, 2, temperature=0.0)
    assert model.training and all(m.training for m in model.modules())
    model.eval()
    model.generate(idx, 2, temperature=0.0)
    assert not model.training


def test_forward_without_cache_keeps_its_bits():
    model, idx = make(2)
    model.eval()
    with torch.no_grad():
        got, loss = model(idx)
        x = model.wte(idx) + model.wpe(torch.arange(P))
        for block in model.h:
            h = F.layer_norm(x, (128,), block.ln_1.weight,
                             block.ln_1.bias, block.ln_1.eps)
            x = x + block.attn(h)
            h = F.layer_norm(x, (128,), block.ln_2.weight,
                             block.ln_2.bias, block.ln_2.eps)
            x = x + block.mlp(h)
        h = F.layer_norm(x, (128,), model.ln_f.weight, model.ln_f.bias,
                         model.ln_f.eps)
        want = model.lm_head(h)
    assert loss is None
    assert torch.equal(got, want)


def test_forward_with_cache_steps():
    """The public forward: prefill, then one token per call."""
    model, idx = make(0)
    model.eval()
    cache = KVCache(2, 3, 2, 32, 64, torch.float32, "cpu")
    with torch.no_grad():
        l0, _ = model(idx, cache=cache)
        nxt = l0[:, -1].argmax(dim=-1, keepdim=True)
        l1, _ = model(nxt, cache=cache)
        full, _ = model(torch.cat([idx, nxt], dim=1))
    assert cache.max_pos == P + 1 and cache.pos.tolist() == [P + 1] * 3
    assert (l1[:, 0] - full[:, -1]).abs().max().item() <= 1e-4
    with pytest.raises(ValueError):
        model(idx, cache=cache)


# --------------------------------------------------------------- trainer
def test_trainer_predict(tmp_path, monkeypatch):
    from torch.utils.data import DataLoader

    from ray_lightning_amd import Trainer
    from ray_lightning_amd.models.benchmark import GPT2LM

    monkeypatch.setattr(GPT2Config, "gpt2",
                        classmethod(lambda cls: tiny_cfg()))
    torch.manual_seed(0)
    lm = GPT2LM(model_size="gpt2", bf16_weights=False,
                gen_max_new_tokens=4)
    assert lm.model.cfg.n_layer == 2
    prompts = torch.randint(0, 256, (6, 10))
    trainer = Trainer(default_root_dir=str(tmp_path), accelerator="cpu")
    preds = trainer.predict(lm, dataloaders=DataLoader(prompts,
                                                       batch_size=3))
    assert len(preds) == 2
    for i, p in enumerate(preds):
        assert p.shape == (3, 14)
        assert torch.equal(p[:, :10].cpu(), prompts[3 * i:3 * i + 3])
    # (idx, prompt_lens) batches; the trainer may have moved the module
    dev = next(lm.parameters()).device
    out = lm.predict_step((prompts[:3].to(dev),
                           torch.tensor([10, 2, 7])), 0)
    assert out.shape == (3, 14)
    assert lm.hparams["gen_max_new_tokens"] == 4
