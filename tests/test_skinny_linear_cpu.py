"""skinny_linear / decode_layer on the CPU tier: the torch twin against
the fp64 reference with the bound of the GPU test (at most twice the
error of the composed bf16 path), the argument errors, and the model's
decode step through decode_layer without a device."""
import pytest
import torch

from ray_lightning_amd.ops import skinny_linear as sl
from skinny_common import (EPS, composed, decode_errors, err, operands,
                           reference, tiny_models)


@pytest.mark.parametrize("M,N,K,mode,gelu,bias", [
    (1, 16, 32, "plain", False, False),
    (17, 81, 96, "add_ln", True, True),
    (64, 24, 1600, "ln", True, True),
])
def test_twin_against_fp64(M, N, K, mode, gelu, bias):
    op = operands(M, N, K, mode, bias, "cpu", seed=M + N + K)
    ref = reference(op, gelu)
    out = sl.skinny_linear(op["x"], op["weight"], op["bias"],
                           residual=op["residual"],
                           ln_weight=op["ln_weight"], ln_bias=op["ln_bias"],
                           eps=EPS, gelu=gelu)
    y = out[0] if mode == "add_ln" else out
    if mode == "add_ln":
        want = (op["x"].float() + op["residual"].float()).bfloat16()
        assert torch.equal(out[1], want)
    assert err(y, ref) <= 2 * err(composed(op, gelu), ref)


def test_value_errors():
    op = operands(4, 24, 96, "add_ln", True, "cpu")
    x, w, b, r = op["x"], op["weight"], op["bias"], op["residual"]
    lw, lb = op["ln_weight"], op["ln_bias"]
    for kw in (dict(residual=r), dict(ln_weight=lw),
               dict(ln_weight=lw[:95], ln_bias=lb[:95]),
               dict(residual=r[:3], ln_weight=lw, ln_bias=lb)):
        with pytest.raises(ValueError):
            sl.skinny_linear(x, w, b, **kw)
    with pytest.raises(ValueError):
        sl.skinny_linear(x, w, b[:23])
    with pytest.raises(ValueError):
        sl.skinny_linear(x, w[:, :64])


def test_model_decode_steps_run_the_twin(monkeypatch):
    m16, m32 = tiny_models(251, "cpu")
    twin = []
    monkeypatch.setattr(sl, "_twin", lambda *a, _f=sl._twin:
                        (twin.append(1), _f(*a))[1])
    e_off, e_on, calls = decode_errors(m16, m32, 251, "cpu", monkeypatch, sl)
    assert calls == 2 * 8 and len(twin) == (2 * 4 + 1) * 8
    assert e_on <= 2 * e_off
