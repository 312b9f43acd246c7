"""GPT2.forward(extend=True) on MI355X in bf16: flash prefill of 64
tokens, 20 appended through ``append_attention`` (kernel and twin), one
decode step, against an fp32 copy of the model. The criterion is that of
tests/test_generate_gpu.py: the largest logit error of the cached path,
``e_cached``, is at most twice that of the uncached bf16 forward,
``e_full``; the values measured are in profiles/append_attn.md."""
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
from ray_lightning_amd.ops.decode_attn import KVCache  # noqa: E402

DEV = "cuda"
B, P, NEW = 3, 64, 20


@pytest.fixture(scope="module")
def reference():
    """(m16, idx, fp32 logits, e_full) at positions P .. P+NEW."""
    torch.manual_seed(0)
    m32 = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=256,
                          n_positions=128)).to(DEV).eval()
    m16 = to_bf16_training(copy.deepcopy(m32)).eval()
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (B, P + NEW + 1), generator=g).to(DEV)
    with torch.no_grad():
        ref = m32(idx)[0][:, P:].float()
        e_full = (m16(idx)[0][:, P:].float() - ref).abs().max().item()
    return m16, idx, ref, e_full


@pytest.mark.parametrize("gate", ["1", "0"], ids=["kernel", "twin"])
def test_prefill_extend_decode(reference, monkeypatch, gate):
    m16, idx, ref, e_full = reference
    monkeypatch.setenv("RLA_APPEND_ATTN", gate)
    cache = KVCache(2, B, 2, 128, 64, torch.bfloat16, DEV)
    with torch.no_grad():
        m16(idx[:, :P], cache=cache)
        l_ext = m16(idx[:, P:P + NEW], cache=cache, extend=True)[0]
        l_dec = m16(idx[:, P + NEW:], cache=cache)[0]
    assert cache.max_pos == P + NEW + 1
    assert cache.pos.tolist() == [P + NEW + 1] * B
    got = torch.cat([l_ext, l_dec], dim=1).float()
    e_cached = (got - ref).abs().max().item()
    print(f"gate {gate}: e_full {e_full:.3e}  e_cached {e_cached:.3e}")
    assert e_cached <= 2 * e_full
