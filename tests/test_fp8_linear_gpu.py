"""The tiled fp8-weight GEMM (csrc/fp8_linear.hip) and a model without
its bf16 block weights on MI355X. The yardsticks are existing code on the
dequantized bf16 weight, which holds the same values exactly:
``reference()`` in fp64 and ``composed()`` in bf16, with ``e_kernel <=
2 * e_composed`` as in tests/test_skinny_fp8_gpu.py. The extension is
called directly so that small M reaches the new kernel."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import fp8_linear as fl  # noqa: E402
from ray_lightning_amd.ops import skinny_linear as sl  # noqa: E402
from skinny_common import (BF16, composed, err, operands,  # noqa: E402
                           reference, tiny_models)

DEV = "cuda"
FP8 = torch.float8_e4m3fn
ext = _ops._load_ext()

# (M, N, K, gelu, bias): the smallest; tails in M and N with a half k-step;
# exactly one 128 tile and one step; several tiles and 25 steps; long K;
# many row tiles. The last one is the smallest grid at which the host picks
# the 128 x 128 tile itself (17 x 22 of them), with tails and a half step.
CASES = [
    (1, 16, 32, False, False),
    (65, 81, 96, True, True),
    (128, 128, 64, False, True),
    (129, 257, 1600, True, True),
    (64, 130, 6400, False, True),
    (300, 16, 32, True, False),
    (2049, 2689, 96, True, True),
]


def _quantized(M, N, K, bias, seed):
    """operands() with the weight rows scaled by 2^(n % 13 - 6), quantized:
    ``weight`` is the dequantized bf16 matrix, ``q`` / ``scale`` the fp8
    pair as slices of buffers whose rows past N are the NaN code / NaN."""
    op = operands(M, N, K, "plain", bias, DEV, seed=seed)
    rows = torch.exp2(torch.arange(N, device=DEV) % 13 - 6.0)[:, None]
    q, scale = sl.quantize_weight(op["weight"].float() * rows)
    qbuf = torch.full((N + 3, K), 0x7F, dtype=torch.uint8, device=DEV)
    qbuf[:N] = q.view(torch.uint8)
    sbuf = torch.full((N + 3,), math.nan, device=DEV)
    sbuf[:N] = scale
    op["weight"] = sl.dequantize_weight(q, scale)
    return op, qbuf.view(FP8)[:N], sbuf[:N]


def _bits(t):
    return t.view(torch.int16)


# tile 0 is the host's pick; 64 and 128 force either instantiation
@pytest.mark.parametrize("tile", [0, 64, 128])
@pytest.mark.parametrize("M,N,K,gelu,bias", CASES)
def test_kernel_against_fp64(M, N, K, gelu, bias, tile):
    op, q, scale = _quantized(M, N, K, bias, M + N + K)
    ref = reference(op, gelu)
    y = ext.fp8_linear_fwd_at(op["x"], q, scale, op["bias"], gelu, tile)
    if tile == 0:
        y0 = ext.fp8_linear_fwd(op["x"], q, scale, op["bias"], gelu)
        assert torch.equal(_bits(y), _bits(y0))
    e_kernel, e_composed = err(y, ref), err(composed(op, gelu), ref)
    print(f"fp8_linear {(M, N, K, gelu, bias)} tile {tile}: e_kernel "
          f"{e_kernel:.3e}  e_composed {e_composed:.3e}")
    assert y.shape == (M, N) and y.dtype == BF16
    assert e_kernel <= 2 * e_composed


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("k0", [0, 64, 128, 192])
def test_every_e4m3_code_converts_exactly(k0, tile):
    """Row n holds byte (k + n) mod 256 (the two NaN codes as 0) with
    scale 2^(n - 8); x is 128 one-hot rows at k0 + (m % 64), so y[m, n]
    must be the dequantized W[n, k0 + m % 64], which is exact in bf16. Bit
    for bit, but for the sign of code 0x80: -0 added to an accumulator's
    +0 is +0 in IEEE arithmetic, so `want` gets the same + 0."""
    K = 256
    n, k = torch.arange(16)[:, None], torch.arange(K)[None, :]
    code = ((k + n) % 256).to(torch.uint8)
    code[(code & 0x7F) == 0x7F] = 0
    q = code.to(DEV).view(FP8)
    scale = torch.exp2(torch.arange(16, device=DEV) - 8.0)
    col = k0 + torch.arange(128) % 64
    x = torch.zeros(128, K, dtype=BF16, device=DEV)
    x[torch.arange(128), col] = 1.0
    y = ext.fp8_linear_fwd_at(x, q, scale, None, False, tile)
    want = sl.dequantize_weight(code.view(FP8), scale.cpu())[:, col]
    want = (want.t().float() + 0.0).to(BF16)
    assert torch.equal(_bits(y.cpu()), _bits(want))


def test_same_bits_twice_a_row_alone_and_either_tile():
    op, q, scale = _quantized(129, 257, 96, True, 5)
    run = lambda x, tile: ext.fp8_linear_fwd_at(  # noqa: E731
        x, q, scale, op["bias"], True, tile)
    y = run(op["x"], 64)
    assert torch.equal(_bits(y), _bits(run(op["x"], 64)))
    assert torch.equal(_bits(y), _bits(run(op["x"], 128)))
    for m in (0, 64, 128):
        for tile in (64, 128):
            alone = run(op["x"][m:m + 1], tile)
            assert torch.equal(_bits(alone[0]), _bits(y[m])), (m, tile)


def test_operand_checks_raise_before_any_launch():
    op, q, s = _quantized(4, 24, 96, True, 0)
    x, b = op["x"], op["bias"]
    wide = torch.zeros(24, 192, dtype=torch.uint8, device=DEV).view(FP8)
    x48, q48 = x[:, :48].contiguous(), q[:, :48].contiguous()
    bad = [
        ("bf16 scale", (x, q, s.to(BF16), b)),
        ("scale length N - 1", (x, q, s[:23], b)),
        ("non-contiguous W", (x, wide[:, ::2], s, b)),
        ("K = 48", (x48, q48, s, b)),
        ("bf16 W", (x, op["weight"], s, b)),
        ("x on the CPU", (x.cpu(), q, s, b)),
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError):
            ext.fp8_linear_fwd(*args, False)
    y = ext.fp8_linear_fwd(x[:0], q, s, b, False)
    assert y.shape == (0, 24)


def test_dropped_model_generates(monkeypatch):
    """A model with the fp8 pairs only against one that kept its bf16
    copies, same weights: the first prefill slice (3 x 64 padded rows, the
    tiled kernel), an extend slice and decode steps (the skinny one).
    Logit errors against the fp32 copy holding the dequantized values."""
    vocab, new, lens = 251, 6, [5, 1, 12]
    asked = []
    monkeypatch.setattr(fl, "_ext_with", lambda s, _f=fl._ext_with:
                        (asked.append(s), _f(s))[1])
    kept, m32 = tiny_models(vocab, DEV)
    kept.quantize_weights_fp8()
    m32.load_state_dict({k: v.float() for k, v in kept.state_dict().items()})
    dropped = copy.deepcopy(kept).quantize_weights_fp8(drop_bf16=True)
    for lin in dropped._block_linears():
        assert lin.weight.numel() == 0
    idx = torch.randint(0, vocab, (3, 12),
                        generator=torch.Generator().manual_seed(1)).to(DEV)
    errs = {}
    for name, m in (("kept", kept), ("dropped", dropped)):
        out, logits = m.generate(idx, new, prompt_lens=lens, prefill_chunk=8,
                                 temperature=0.0, return_logits=True)
        e, rows = 0.0, []
        with torch.no_grad():
            for b, n in enumerate(lens):
                ref = m32(out[b, :n + new][None])[0][0, n - 1:n - 1 + new]
                e = max(e, (logits[b] - ref.float()).abs().max().item())
                rows.append((out[b, n:n + new], ref.float()))
        errs[name] = (e, rows)
    e_kept, e_dropped = errs["kept"][0], errs["dropped"][0]
    print(f"e_kept {e_kept:.3e}  e_dropped {e_dropped:.3e}")
    assert "fp8_linear_fwd" in asked and "skinny_linear_fwd" in asked
    assert e_dropped <= 2 * e_kept
    for tok, ref in errs["dropped"][1]:
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4 * e_kept
        assert torch.equal(tok[clear], ref.argmax(dim=-1)[clear])
