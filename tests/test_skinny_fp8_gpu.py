"""The fp8-weight skinny-linear kernels and decode_layer's fp8 route on
MI355X. The yardsticks are existing code on the dequantized bf16 weight,
which holds the same values exactly: ``reference()`` in fp64 and
``composed()`` in bf16, with ``e_kernel <= 2 * e_composed`` as in
tests/test_skinny_linear_gpu.py. The values measured are in
profiles/skinny_linear_fp8.md."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import skinny_linear as sl  # noqa: E402
from skinny_common import (BF16, EPS, composed, decode_errors,  # noqa: E402
                           err, operands, reference, tiny_models)

DEV = "cuda"
FP8 = torch.float8_e4m3fn

# (M, N, K, mode, gelu, bias): one k-step, an odd step count, 50 and 200
# steps (6, 7 or 25 per wave: pairs and a tail), half a tile, an odd N, one
# and two row tiles per workgroup, every MT. The last case adds pairs of
# k-steps to the two-tile kernels.
CASES = [
    (1, 16, 32, "plain", False, False),
    (1, 24, 96, "plain", True, True),
    (16, 81, 32, "ln", True, True),
    (17, 81, 96, "add_ln", True, True),
    (17, 16, 1600, "ln", True, False),
    (64, 81, 1600, "add_ln", True, True),
    (8, 256, 6400, "plain", False, True),
    (17, 4113, 96, "add_ln", True, True),
    (64, 4099, 32, "ln", False, False),
    (1, 4112, 96, "plain", False, True),
    (17, 4113, 1600, "add_ln", True, True),
]


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "1")


def _quantized(M, N, K, mode, bias, seed):
    """operands() with the weight rows scaled by 2^(n % 13 - 6), quantized:
    ``weight`` is the dequantized bf16 matrix, ``q`` / ``scale`` the fp8
    pair as slices of buffers whose rows past N are the NaN code / NaN."""
    op = operands(M, N, K, mode, bias, DEV, seed=seed)
    rows = torch.exp2(torch.arange(N, device=DEV) % 13 - 6.0)[:, None]
    q, scale = sl.quantize_weight(op["weight"].float() * rows)
    qbuf = torch.full((N + 3, K), 0x7F, dtype=torch.uint8, device=DEV)
    qbuf[:N] = q.view(torch.uint8)
    sbuf = torch.full((N + 3,), math.nan, device=DEV)
    sbuf[:N] = scale
    op["weight"] = sl.dequantize_weight(q, scale)
    return op, qbuf.view(FP8)[:N], sbuf[:N]


def _run(op, q, scale, gelu):
    out = sl.skinny_linear(op["x"], q, op["bias"], residual=op["residual"],
                           ln_weight=op["ln_weight"], ln_bias=op["ln_bias"],
                           eps=EPS, gelu=gelu, weight_scale=scale)
    return out if op["residual"] is not None else (out, None)


@pytest.mark.parametrize("M,N,K,mode,gelu,bias", CASES)
def test_kernel_against_fp64(M, N, K, mode, gelu, bias, monkeypatch):
    twin = []
    monkeypatch.setattr(sl, "_twin", lambda *a: twin.append(1))
    op, q, scale = _quantized(M, N, K, mode, bias, M + N + K)
    ref = reference(op, gelu)
    y, x_new = _run(op, q, scale, gelu)
    e_kernel, e_composed = err(y, ref), err(composed(op, gelu), ref)
    print(f"fp8 kernel {(M, N, K, mode, gelu, bias)}: e_kernel "
          f"{e_kernel:.3e}  e_composed {e_composed:.3e}")
    assert not twin
    assert y.shape == (M, N) and y.dtype == BF16
    if mode == "add_ln":
        want = (op["x"].float() + op["residual"].float()).to(BF16)
        assert torch.equal(x_new.view(torch.int16), want.view(torch.int16))
    assert e_kernel <= 2 * e_composed


# K = 256 is one k-step per wave; K = 1024 is two pairs per wave, so there
# the one-hot rows also show the k order of the wide loads
@pytest.mark.parametrize("K,k0", [(256, 0), (256, 64), (256, 128),
                                  (256, 192), (1024, 0), (1024, 960)])
def test_every_e4m3_code_converts_exactly(K, k0):
    """Row n holds byte (k + n) mod 256 (the two NaN codes as 0) with
    scale 2^(n - 8); x is 64 one-hot rows at k0 .., so y[m, n] must be
    the dequantized W[n, k0 + m], which is exact in bf16. Bit for bit,
    but for the sign of code 0x80: -0 added to an accumulator's +0 is
    +0 in IEEE arithmetic, so `want` gets the same + 0."""
    n, k = torch.arange(16)[:, None], torch.arange(K)[None, :]
    code = ((k + n) % 256).to(torch.uint8)
    code[(code & 0x7F) == 0x7F] = 0
    q = code.to(DEV).view(FP8)
    scale = torch.exp2(torch.arange(16, device=DEV) - 8.0)
    x = torch.zeros(64, K, dtype=BF16, device=DEV)
    x[torch.arange(64), k0 + torch.arange(64)] = 1.0
    y = sl.skinny_linear(x, q, weight_scale=scale)
    want = sl.dequantize_weight(code.view(FP8), scale.cpu())[:, k0:k0 + 64]
    want = (want.t().float() + 0.0).to(BF16)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("N", [81, 4113])  # one and two weight tiles
def test_same_bits_twice_and_row_alone(N):
    op, q, scale = _quantized(17, N, 96, "add_ln", True, 5)
    y, x_new = _run(op, q, scale, True)
    y2, x_new2 = _run(op, q, scale, True)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(x_new.view(torch.int16), x_new2.view(torch.int16))
    for m in range(17):
        alone = dict(op, x=op["x"][m:m + 1], residual=op["residual"][m:m + 1])
        ym, _ = _run(alone, q, scale, True)
        assert torch.equal(ym[0].view(torch.int16), y[m].view(torch.int16)), m


def test_operand_checks_raise_before_any_launch():
    ext = _ops._load_ext()
    op, q, s = _quantized(4, 24, 96, "plain", True, 0)
    x, b = op["x"], op["bias"]
    wide = torch.zeros(24, 192, dtype=torch.uint8, device=DEV).view(FP8)
    x48, q48 = x[:, :48].contiguous(), q[:, :48].contiguous()
    x65 = torch.zeros(65, 96, dtype=BF16, device=DEV)
    bad = [
        ("bf16 scale", (x, q, b, s.to(BF16))),
        ("scale length N - 1", (x, q, b, s[:23])),
        ("non-contiguous fp8 W", (x, wide[:, ::2], b, s)),
        ("fp8 W without a scale", (x, q, b, None)),
        ("K = 48", (x48, q48, b, s)),
        ("M = 65", (x65, q, b, s)),
    ]
    for what, (x_, q_, b_, s_) in bad:
        with pytest.raises(RuntimeError):
            ext.skinny_linear_fwd(x_, q_, b_, None, None, None, EPS, False,
                                  s_)
    y, x_new = ext.skinny_linear_fwd(x[:0], q, b, None, None, None, EPS,
                                     False, s)
    assert y.shape == (0, 24) and x_new is None


@pytest.mark.parametrize("vocab,fp8", [(256, "1"), (251, "1"), (251, "0")])
def test_model_decode_steps(vocab, fp8, monkeypatch):
    monkeypatch.setenv("RLA_SKINNY_FP8", fp8)
    asked = []
    monkeypatch.setattr(sl, "_ext_with", lambda s, _f=sl._ext_with:
                        (asked.append(s), _f(s))[1])
    m16, m32 = tiny_models(vocab, DEV)
    m16.quantize_weights_fp8()
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    e_off, e_on, calls = decode_errors(m16, m32, vocab, DEV, monkeypatch, sl)
    assert calls == 2 * 8, "decode_layer did not run once per layer and step"
    want, other = (("decode_layer_fp8_fwd", "decode_layer_fwd") if fp8 == "1"
                   else ("decode_layer_fwd", "decode_layer_fp8_fwd"))
    assert want in asked and other not in asked
    assert e_on <= 2 * e_off
