"""ops/sample.py on the CPU: the torch twin against the fp64 reference of
sample_common.py, and GPT2.generate(top_p=, seed=) through it."""
import pytest
import torch

import sample_common as sc
from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
from ray_lightning_amd.ops.sample import sample_tokens


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", sc.VS)
def test_twin_against_fp64(V, B, dtype):
    sc.run_cases(sample_tokens, sc.make_rows(V, B, dtype), "cpu")


def test_all_neg_inf_row_is_token_zero():
    rows = torch.full((2, 100), -torch.inf)
    rows[1, 40] = 1.0
    seeds = torch.zeros(2, dtype=torch.int64)
    for t in (0.0, 1.0):
        assert sample_tokens(rows, seeds, 0, temperature=t,
                             top_p=0.9).tolist() == [0, 40]


def test_bitwise_and_row_alone():
    sc.check_rows_alone(sample_tokens, sc.make_rows(4097, 3, torch.float32),
                        "cpu")


def test_epilogue():
    sc.check_epilogue(sample_tokens, "cpu")


_OK, _BAD = sc.bad_operands("cpu")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_rejected_operand(name):
    kw = dict(_OK, **_BAD[name])
    with pytest.raises((ValueError, RuntimeError)):
        sample_tokens(kw.pop("logits"), kw.pop("seeds"), kw.pop("step"),
                      **kw)


@pytest.mark.parametrize("top_p,top_k", [(0.9, 40), (1.0, None)])
def test_generate_tokens_in_their_intervals(top_p, top_k):
    torch.manual_seed(0)
    m = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                        n_positions=128)).eval()
    idx = torch.randint(0, 256, (3, 12))
    lens, new, seed = [5, 1, 12], 8, 1234
    kw = dict(prompt_lens=lens, top_p=top_p, top_k=top_k, seed=seed,
              return_logits=True)
    out, logits = m.generate(idx, new, **kw)
    assert torch.equal(out, m.generate(idx, new, **kw)[0])
    for b, n in enumerate(lens):
        for s in range(new):
            sc.Ref(logits[b, s], 1.0, top_k, top_p).check(
                int(out[b, n + s]), seed + b, s)
