"""ops/spec_decode.py on the CPU tier (the torch twin) against the plain
Python reference of spec_common.py, and GPT2.generate(draft_tokens=)
against the plain seeded call."""
import pytest
import torch

import sample_common as sc
import spec_common as sp
from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config

DEV = "cpu"


def test_reference_by_hand():
    assert sp.ref_draft([30, 1, 2, 1, 2], 3, 4, 0) == [2, 1, 2, 1, 2]
    assert sp.ref_draft([5, 6, 7, 30, 40, 6, 7, 31, 41, 5, 6, 7], 3, 2,
                        0) == [7, 30, 40]
    assert sp.ref_draft([4, 4], 3, 3, 0) == [4, 4, 4, 4]
    assert sp.ref_draft([3, 8], 3, 2, 0) == [8, 8, 8]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T1", [1, 4, 16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", sc.VS)
def test_tokens_bit_for_bit(V, B, T1, dtype):
    sp.token_case(DEV, V, B, T1, dtype)


@pytest.mark.parametrize("ngram,next_T", [(3, 4), (8, 15), (1, 0)])
def test_commit_and_draft(ngram, next_T):
    rows, toks = sp.state_rows()
    sp.check_step(DEV, sp.dominant(toks), rows, sp.WIDTH, sp.LIMIT,
                  dict(temperature=0.0), eos=sp.EOS, pad=sp.PAD,
                  ngram=ngram, next_T=next_T)


@pytest.mark.parametrize("name", sorted(sp.bad_operands("cpu")[1]))
def test_rejected_operand(name):
    ok, bad = sp.bad_operands(DEV)
    sp.call(ok)
    with pytest.raises(ValueError):
        sp.call(dict(ok, **bad[name]))


# ---------------------------------------------------------------- generate
MODEL_SEED = 0
LENS, P, NEW = [5, 1, 12], 12, 32


def tiny(n_positions=128):
    torch.manual_seed(MODEL_SEED)
    model = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                            n_positions=n_positions))
    g = torch.Generator().manual_seed(100 + MODEL_SEED)
    idx = torch.randint(0, 256, (3, P), generator=g)
    idx[2] = torch.tensor([7, 8, 9] * 4)          # a periodic prompt
    return model, idx


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("sampler", [dict(temperature=0.0),
                                     dict(temperature=1.0, top_k=8)])
def test_generate_equals_plain_seeded(T, sampler):
    model, idx = tiny()
    plain, logits = model.generate(idx, NEW, prompt_lens=LENS, seed=11,
                                   return_logits=True, **sampler)
    # pick an EOS one row emits mid-way, so padding is exercised
    eos = int(plain[0, LENS[0] + 9])
    kw = dict(prompt_lens=LENS, seed=11, eos_token_id=eos, pad_token_id=3,
              **sampler)
    plain = model.generate(idx, NEW, **kw)
    if sampler["temperature"] == 0:
        # the decode and the append twin sum in different orders: the
        # greedy choice must not hang on that
        top2 = logits.topk(2, dim=-1).values
        assert (top2[..., 0] - top2[..., 1]).min().item() > 1e-4
    got, stats = model.generate(idx, NEW, draft_tokens=T, return_stats=True,
                                **kw)
    assert torch.equal(got, plain)
    if sampler["temperature"] == 0:
        assert stats["forwards"] < NEW


def test_generate_stats_and_tail_near_n_positions():
    # 12 + 32 = 44 positions: the last steps draft fewer than 4 tokens
    model, idx = tiny(n_positions=P + NEW)
    plain = model.generate(idx, NEW, prompt_lens=LENS, seed=5,
                           temperature=0.0)
    got, stats = model.generate(idx, NEW, prompt_lens=LENS, seed=5,
                                temperature=0.0, draft_tokens=4,
                                return_stats=True)
    assert torch.equal(got, plain)
    assert stats["committed"] == 3 * (NEW - 1)
    assert stats["forwards"] < NEW


def test_generate_rejects():
    model, idx = tiny()
    for kw in (dict(draft_tokens=16), dict(draft_tokens=-1),
               dict(draft_tokens=2, draft_ngram=9),
               dict(draft_tokens=2, return_logits=True)):
        with pytest.raises(ValueError):
            model.generate(idx, 4, **kw)
