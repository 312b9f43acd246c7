"""GPT2.generate on MI355X in bf16: the cached path (flash prefill, the
decode-attention kernel) against an fp32 copy of the model, measured
with the uncached bf16 forward as the yardstick.

``e_full`` is the largest logit error of the uncached bf16 forward
against fp32 at the generated positions, ``e_cached`` the same for the
logits ``generate`` sampled from. Both are bf16 paths that differ in
rounding order only, so ``e_cached <= 2 * e_full`` is required; the
values measured are in profiles/gpt2_generate.md."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,  # noqa: E402
                                           to_bf16_training)
from ray_lightning_amd.ops import decode_attn as da  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    m32 = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                          n_positions=128)).to(DEV).eval()
    m16 = to_bf16_training(copy.deepcopy(m32)).eval()
    # the fp32 copy holds the bf16 model's weights exactly
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16, m32


def _prompts(B, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, P), generator=g).to(DEV)


def _errors(m16, m32, idx, lens, new):
    """(e_full, e_cached, steps under the margin) of one greedy run,
    after asserting the token agreement."""
    out, logits = m16.generate(idx, new, prompt_lens=lens, temperature=0.0,
                               return_logits=True)
    assert out.shape == (idx.shape[0], idx.shape[1] + new)
    e_full = e_cached = 0.0
    rows = []
    with torch.no_grad():
        for b, n in enumerate(lens):
            assert torch.equal(out[b, :n], idx[b, :n])
            seq = out[b, :n + new][None]
            ref = m32(seq)[0][0, n - 1:n - 1 + new].float()
            full = m16(seq)[0][0, n - 1:n - 1 + new].float()
            e_full = max(e_full, (full - ref).abs().max().item())
            e_cached = max(e_cached, (logits[b] - ref).abs().max().item())
            rows.append((out[b, n:n + new], ref))
    under = 0
    for tok, ref in rows:
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4 * e_full
        under += int((~clear).sum())
        assert torch.equal(tok[clear], ref.argmax(dim=-1)[clear])
    total = new * len(lens)
    print(f"e_full {e_full:.3e}  e_cached {e_cached:.3e}  "
          f"under margin {under}/{total}")
    assert under <= total // 10, f"{under} of {total} steps under the margin"
    return e_full, e_cached


@pytest.fixture(autouse=True)
def _kernel_on(monkeypatch):
    monkeypatch.setenv("RLA_DECODE_ATTN", "1")


def _kernel_calls(monkeypatch):
    calls = []
    ext = _ops._load_ext()

    class Spy:
        def decode_attn_fwd(self, *args):
            calls.append(1)
            return ext.decode_attn_fwd(*args)

        def __getattr__(self, name):  # everything else: the extension's
            return getattr(ext, name)

    monkeypatch.setattr(da, "_load_ext", lambda: Spy())
    return calls


def test_ragged_prompts_logits_and_tokens(models, monkeypatch):
    m16, m32 = models
    calls = _kernel_calls(monkeypatch)
    lens = [5, 1, 12]
    e_full, e_cached = _errors(m16, m32, _prompts(3, 12, 1), lens, 32)
    assert len(calls) == 2 * 31, "the decode kernel did not run"
    assert e_cached <= 2 * e_full


@pytest.mark.parametrize("P,new", [(64, 32), (70, 32), (70, 16)])
def test_prompt_on_and_off_the_flash_tile(models, P, new):
    """64: the prefill is on the flash kernels as it stands; 70: padded
    to 128 = n_positions."""
    m16, m32 = models
    e_full, e_cached = _errors(m16, m32, _prompts(2, P, P), [P, P], new)
    assert e_cached <= 2 * e_full


def test_kernel_against_fallback(models, monkeypatch):
    m16, m32 = models
    idx, lens = _prompts(3, 12, 1), [5, 1, 12]
    e_full1, e_kernel = _errors(m16, m32, idx, lens, 32)
    monkeypatch.setenv("RLA_DECODE_ATTN", "0")
    e_full0, e_twin = _errors(m16, m32, idx, lens, 32)
    assert e_kernel <= 2 * e_full1
    assert e_twin <= 2 * e_full0
