"""fp8_linear's twin and a model without its bf16 block weights, on the
CPU tier."""
import copy

import pytest
import torch

from ray_lightning_amd.models.benchmark import GPT2LM
from ray_lightning_amd.models.gpt2 import GPT2Config
from ray_lightning_amd.ops import skinny_linear as sl
from ray_lightning_amd.ops.fp8_linear import fp8_linear
from skinny_common import BF16, operands, tiny_models


@pytest.mark.parametrize("gelu", [False, True])
def test_twin_bits_equal_the_skinny_twin_on_dequantized(gelu):
    op = operands(65, 81, 96, "plain", True, "cpu", seed=1)
    q, s = sl.quantize_weight(op["weight"])
    got = fp8_linear(op["x"], q, s, op["bias"], gelu=gelu)
    want = sl.skinny_linear(op["x"], sl.dequantize_weight(q, s), op["bias"],
                            gelu=gelu)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    x3 = op["x"][:60].view(4, 15, 96)
    assert torch.equal(fp8_linear(x3, q, s, op["bias"], gelu=gelu),
                       got[:60].view(4, 15, 81))
    for bad in ((op["x"], op["weight"], s), (op["x"], q, s[:-1]),
                (op["x"][:, :64], q, s)):
        with pytest.raises(ValueError):
            fp8_linear(*bad, op["bias"], gelu=gelu)


def _logit_error(m, m32, idx, new, **kw):
    out, logits = m.generate(idx, new, temperature=0.0, return_logits=True,
                             **kw)
    P = idx.shape[1]
    with torch.no_grad():
        ref = m32(out)[0][:, P - 1:P - 1 + new].float()
    return (logits - ref).abs().max().item(), out


def test_dropped_model():
    kept, m32 = tiny_models(251, "cpu")
    keys = list(kept.state_dict())
    kept.quantize_weights_fp8()
    m32.load_state_dict({k: v.float() for k, v in kept.state_dict().items()})
    dropped = copy.deepcopy(kept).quantize_weights_fp8(drop_bf16=True)
    for lin in dropped._block_linears():
        N, K = lin.weight_fp8.shape
        held = sum(t.numel() * t.element_size() for t in
                   (lin.weight, lin.weight_fp8, lin.weight_scale))
        assert held == N * K + 4 * N and tuple(lin.weight.shape) == (0, K)
    assert dropped.wte.weight.dtype == BF16 and dropped.wte.weight.numel()
    sd = dropped.state_dict()
    assert set(sd) == set(keys) | {
        k[:-len("weight")] + b for k in keys for b in
        ("weight_fp8", "weight_scale")
        if k.startswith("h.") and k.endswith(("c_attn.weight", "c_fc.weight",
                                              "c_proj.weight"))}
    # a strict load into a second dropped model, made from other weights
    other = copy.deepcopy(kept)
    for p in other.parameters():
        p.data.mul_(0.5)
    other.quantize_weights_fp8(drop_bf16=True)
    other.load_state_dict(sd)
    idx = torch.randint(0, 251, (3, 7),
                        generator=torch.Generator().manual_seed(3))
    e_kept, _ = _logit_error(kept, m32, idx, 6, prefill_chunk=4)
    e_dropped, out = _logit_error(dropped, m32, idx, 6, prefill_chunk=4)
    assert e_dropped <= 2 * e_kept
    assert torch.equal(other.generate(idx, 6, temperature=0.0,
                                      prefill_chunk=4), out)
    drafted = dropped.generate(idx, 6, temperature=0.0, seed=0,
                               draft_tokens=3)
    assert drafted.shape == (3, 13) and torch.equal(drafted[:, :7], idx)
    with pytest.raises(RuntimeError):
        dropped.quantize_weights_fp8()
    with pytest.raises(RuntimeError):
        dropped.train()(idx)


def test_gpt2lm_drops_on_its_first_predict_step(monkeypatch):
    monkeypatch.setattr(GPT2Config, "gpt2", classmethod(
        lambda cls: GPT2Config(n_layer=2, n_embd=128, n_head=2,
                               vocab_size=251, n_positions=128)))
    lm = GPT2LM(model_size="gpt2", gen_max_new_tokens=2,
                gen_fp8_weights="drop")
    idx = torch.randint(0, lm.model.cfg.vocab_size, (2, 5),
                        generator=torch.Generator().manual_seed(0))
    assert not lm.model.weights_dropped()
    out = lm.predict_step(idx, 0)
    assert out.shape == (2, 7) and lm.model.weights_dropped()
    assert torch.equal(lm.predict_step(idx, 0), out)
