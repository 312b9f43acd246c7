"""fp8 weights for the skinny linears on the CPU tier: the quantization
rule, the twin, and a quantized model against a bf16 model that was given
the dequantized weights."""
import copy

import pytest
import torch

from ray_lightning_amd.ops import skinny_linear as sl
from skinny_common import BF16, EPS, operands, tiny_models


def _weight(seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(40, 96, generator=g) * 0.02
    w *= torch.exp2(torch.arange(40) % 13 - 6.0)[:, None]
    w[3] = 0.0
    w[5] = torch.where(w[5].abs() == w[5].abs().max(), 448 * 0.25, 0.01)
    w[6] = torch.where(w[6].abs() == w[6].abs().max(), 225 * 0.25, 0.01)
    return w


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_quantize_weight_properties(dtype):
    w = _weight(0).to(dtype)
    q, s = sl.quantize_weight(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape
    assert s.dtype == torch.float32 and s.shape == (40,)
    assert torch.equal(torch.frexp(s)[0], torch.full((40,), 0.5))  # 2^j
    # the smallest such power of two: absmax / s in (224, 448]
    r = w.float().abs().amax(dim=1) / s
    live = torch.arange(40) != 3
    assert (r[live] <= 448).all() and (r[live] > 224).all()
    assert s[3] == 1 and (q[3].view(torch.uint8) == 0).all()
    assert s[5] == 0.25 and s[6] == 0.25
    assert ((q.view(torch.uint8) & 0x7F) != 0x7F).all()  # no NaN code
    deq = q.float() * s[:, None]
    assert torch.equal(deq.to(BF16).float(), deq)  # exact in bf16
    assert torch.equal(sl.dequantize_weight(q, s).float(), deq)
    q2, s2 = sl.quantize_weight(deq.to(BF16))
    assert torch.equal(q2.float() * s2[:, None], deq)
    assert s2[6] == 0.125  # largest code 224: the pair moves, the value not


@pytest.mark.parametrize("M,N,K,mode,gelu", [
    (1, 16, 32, "plain", False), (17, 81, 96, "add_ln", True)])
def test_twin_bits_equal_the_bf16_twin_on_dequantized(M, N, K, mode, gelu):
    op = operands(M, N, K, mode, True, "cpu", seed=M + N + K)
    q, s = sl.quantize_weight(op["weight"])
    kw = dict(residual=op["residual"], ln_weight=op["ln_weight"],
              ln_bias=op["ln_bias"], eps=EPS, gelu=gelu)
    got = sl.skinny_linear(op["x"], q, op["bias"], weight_scale=s, **kw)
    want = sl.skinny_linear(op["x"], sl.dequantize_weight(q, s), op["bias"],
                            **kw)
    for a, b in zip(*((got, want) if mode == "add_ln" else ([got], [want]))):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    with pytest.raises(ValueError):
        sl.skinny_linear(op["x"], q, op["bias"])
    with pytest.raises(ValueError):
        sl.skinny_linear(op["x"], q, op["bias"], weight_scale=s[:-1])


def test_quantized_model_generates_as_bf16_on_dequantized(monkeypatch):
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "1")
    m16, _ = tiny_models(251, "cpu")
    keys = list(m16.state_dict())
    mq = copy.deepcopy(m16)
    assert mq.quantize_weights_fp8() is mq
    assert list(mq.state_dict()) == keys
    lin = mq.h[1].mlp.c_fc
    assert torch.equal(sl.dequantize_weight(lin.weight_fp8, lin.weight_scale),
                       lin.weight)
    assert not torch.equal(lin.weight, m16.h[1].mlp.c_fc.weight)
    plain = copy.deepcopy(m16)
    plain.load_state_dict(mq.state_dict())  # strict
    routed = []
    monkeypatch.setattr(sl, "dequantize_weight",
                        lambda *a, _f=sl.dequantize_weight:
                        (routed.append(1), _f(*a))[1])
    idx = torch.randint(0, 251, (3, 7),
                        generator=torch.Generator().manual_seed(3))
    out = [m.generate(idx, 6, temperature=0.0, return_logits=True)
           for m in (mq, plain)]
    assert len(routed) == 2 * 4 * 5  # the fp8 pairs went to skinny_linear
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
