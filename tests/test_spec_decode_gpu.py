"""csrc/spec_decode.hip on MI355X against the plain Python reference of
spec_common.py, tokens against the sampling kernel, and
GPT2.generate(draft_tokens=) in bf16 against an fp32 copy of the model.

Measured on an MI355X (profiles/spec_decode.md): test_generate_greedy
leaves out 0 of its 96 positions under the 4 * e_full margin (e_full
6.9e-3) and runs 7 forwards for 32 tokens."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

import sample_common as sc  # noqa: E402
import spec_common as sp  # noqa: E402
from ray_lightning_amd import ops as _ops  # noqa: E402
from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,  # noqa: E402
                                           to_bf16_training)

assert _ops._load_ext() is not None, "HIP extension failed to load"
DEV = "cuda"


@pytest.fixture(autouse=True)
def gates_on(monkeypatch):
    monkeypatch.setenv("RLA_FUSED_SAMPLE", "1")
    monkeypatch.delenv("RLA_SPEC_DECODE", raising=False)


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


def test_hand_over_under_load():
    """1024 workgroups, 16 to a row: whichever arrives last commits."""
    B, T1, V, L = 64, 16, 4097, 1100
    logits = sc.make_rows(V, B * T1, torch.bfloat16).view(B, T1, V)
    sampler = dict(temperature=1.0, top_k=40, top_p=0.9)
    g = torch.Generator().manual_seed(9)

    def rows():
        g.manual_seed(9)
        return [dict(h=torch.randint(0, 3, (2 + 17 * b,),
                                     generator=g).tolist(),
                     draft=[0] * (T1 - 1), fin=b % 13 == 5, em=b % 7)
                for b in range(B)]

    # drafts that agree with the tokens for b % 16 positions
    first = sp.check_step(DEV, logits, rows(), L, 12, sampler, eos=17)
    drafted = rows()
    for b, r in enumerate(drafted):
        r["draft"] = first["tok"][b, :T1 - 1].tolist()
        r["draft"][b % 16 % (T1 - 1)] += 1
    again = [sp.check_step(DEV, logits, copy.deepcopy(drafted), L, 12,
                           sampler, eos=17, next_T=15) for _ in range(2)]
    assert len(set(again[0]["n_commit"].tolist())) > 4
    for k, v in again[0].items():
        assert torch.equal(v, again[1][k]), k


@pytest.mark.parametrize("name", sorted(sp.bad_operands("cpu")[1])
                         + ["seeds_cpu"])
def test_rejected_operand(name):
    ok, bad = sp.bad_operands(DEV)
    with pytest.raises(ValueError):
        sp.call(dict(ok, **bad[name]))
    torch.cuda.synchronize()


def test_generate_greedy():
    torch.manual_seed(0)
    m32 = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                          n_positions=128)).to(DEV).eval()
    m16 = to_bf16_training(copy.deepcopy(m32)).eval()
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (3, 12), generator=g)
    idx[2] = torch.tensor([7, 8, 9] * 4)
    idx, lens, new = idx.to(DEV), [5, 1, 12], 32
    out, stats = m16.generate(idx, new, prompt_lens=lens, temperature=0.0,
                              draft_tokens=4, return_stats=True)
    assert stats["forwards"] < new
    assert stats["committed"] == 3 * (new - 1)
    e_full, checks = 0.0, []
    with torch.no_grad():
        for b, n in enumerate(lens):
            assert torch.equal(out[b, :n], idx[b, :n])
            seq = out[b, :n + new][None]
            ref = m32(seq)[0][0, n - 1:n - 1 + new].float()
            full = m16(seq)[0][0, n - 1:n - 1 + new].float()
            e_full = max(e_full, (full - ref).abs().max().item())
            checks.append((out[b, n:n + new], ref))
    under = 0
    for tok, ref in checks:
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4 * e_full
        under += int((~clear).sum())
        assert torch.equal(tok[clear], ref.argmax(dim=-1)[clear])
    print(f"forwards {stats['forwards']}  e_full {e_full:.3e}  "
          f"under margin {under}/{3 * new}")
    assert under <= 3 * new // 10
