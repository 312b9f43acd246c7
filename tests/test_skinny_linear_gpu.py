"""The skinny-linear MFMA kernel and decode_layer on MI355X against an
fp64 reference from the same bf16 operands. ``e_kernel`` is the kernel's
largest absolute error, ``e_composed`` that of the path the model takes
without it (fused add + LayerNorm, F.linear, F.gelu, all bf16); both are
bf16 computations of one quantity that differ in rounding order, so
``e_kernel <= 2 * e_composed`` is required. The values measured are in
profiles/skinny_linear.md."""
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

# (M, N, K, mode, gelu, bias). M: one row, a full tile, a tile boundary,
# the most tiles. N: one tile, half a tile, an odd width. K: one k-step
# (fewer than the waves), 3 (does not divide among them), 50 (GPT-2-XL).
# From N = 4096 on a workgroup owns two 16-row weight tiles: 4113 = 32 *
# 128 + 17 leaves the last workgroup's second tile one row, as vocabulary
# 50257 does, 4099 and 4112 leave it none (4112: the vector store).
CASES = [
    (1, 16, 32, "plain", False, False),
    (1, 24, 96, "plain", True, True),
    (1, 81, 1600, "add_ln", False, False),
    (16, 24, 96, "ln", False, True),
    (16, 81, 32, "ln", True, True),
    (17, 81, 96, "add_ln", True, True),
    (17, 16, 1600, "ln", True, False),
    (17, 24, 1600, "plain", False, True),
    (64, 24, 32, "plain", True, True),
    (64, 16, 96, "add_ln", False, True),
    (64, 81, 1600, "add_ln", True, True),
    (8, 256, 6400, "plain", False, True),   # the MLP c_proj's depth
    (17, 4113, 96, "add_ln", True, True),
    (64, 4099, 32, "ln", False, False),
    (64, 4113, 1600, "add_ln", True, True),
    (1, 4112, 96, "plain", False, True),
]


@pytest.fixture(autouse=True)
def _gate_on(monkeypatch):
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "1")


def _run(op, gelu):
    out = sl.skinny_linear(op["x"], op["weight"], op["bias"],
                           residual=op["residual"],
                           ln_weight=op["ln_weight"], ln_bias=op["ln_bias"],
                           eps=EPS, gelu=gelu)
    return out if op["residual"] is not None else (out, None)


def _check(M, N, K, mode, gelu, bias, what):
    op = operands(M, N, K, mode, bias, DEV, seed=M + N + K)
    ref = reference(op, gelu)
    y, x_new = _run(op, gelu)
    e_kernel, e_composed = err(y, ref), err(composed(op, gelu), ref)
    print(f"{what} {(M, N, K, mode, gelu, bias)}: e_kernel {e_kernel:.3e}  "
          f"e_composed {e_composed:.3e}")
    assert y.shape == (M, N) and y.dtype == BF16
    if mode == "add_ln":
        want = (op["x"].float() + op["residual"].float()).to(BF16)
        assert torch.equal(x_new.view(torch.int16), want.view(torch.int16))
    assert e_kernel <= 2 * e_composed


@pytest.mark.parametrize("M,N,K,mode,gelu,bias", CASES)
def test_kernel_against_fp64(M, N, K, mode, gelu, bias, monkeypatch):
    twin = []
    monkeypatch.setattr(sl, "_twin", lambda *a: twin.append(1))
    _check(M, N, K, mode, gelu, bias, "kernel")
    assert not twin


@pytest.mark.parametrize("N", [81, 4113])  # one and two weight tiles
def test_same_bits_twice_and_row_alone(N):
    op = operands(17, N, 96, "add_ln", True, DEV, seed=5)
    y, x_new = _run(op, True)
    y2, x_new2 = _run(op, True)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(x_new.view(torch.int16), x_new2.view(torch.int16))
    for m in range(17):
        alone = dict(op, x=op["x"][m:m + 1], residual=op["residual"][m:m + 1])
        ym, _ = _run(alone, True)
        assert torch.equal(ym[0].view(torch.int16), y[m].view(torch.int16)), m


def test_gate_off_runs_the_twin(monkeypatch):
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "0")
    called = []
    monkeypatch.setattr(sl, "_twin", lambda *a, _f=sl._twin:
                        (called.append(1), _f(*a))[1])
    _check(17, 81, 96, "add_ln", True, True, "twin")
    assert called


def test_operand_checks_raise_before_any_launch():
    ext = _ops._load_ext()
    op = operands(4, 24, 96, "add_ln", True, DEV)
    x, w, b, r = op["x"], op["weight"], op["bias"], op["residual"]
    lw, lb = op["ln_weight"], op["ln_bias"]
    wide = torch.zeros(24, 192, dtype=BF16, device=DEV)
    x48, w48 = x[:, :48].contiguous(), w[:, :48].contiguous()
    x65 = torch.zeros(65, 96, dtype=BF16, device=DEV)
    bad = [
        ("fp16 x", (x.half(), w, b, None, None, None)),
        ("non-contiguous W", (x, wide[:, ::2], b, None, None, None)),
        ("K = 48", (x48, w48, b, None, None, None)),
        ("M = 65", (x65, w, b, None, None, None)),
        ("residual without LN", (x, w, b, r, None, None)),
        ("ln_weight without ln_bias", (x, w, b, None, lw, None)),
        ("wrong bias length", (x, w, b[:23], None, None, None)),
        ("bf16 ln_weight", (x, w, b, None, lw.to(BF16), lb.to(BF16))),
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError):
            ext.skinny_linear_fwd(*args, EPS, False)
    y, x_new = ext.skinny_linear_fwd(x[:0], w, b, r[:0], lw, lb, EPS, False)
    assert y.shape == (0, 24) and x_new.shape == (0, 96)


# RLA_DECODE_ATTN=0 keeps decode attention's kernel off: the block is then
# composed in Python and the one-call entry, which reaches it from C++, rests
@pytest.mark.parametrize("vocab,attn", [(256, "1"), (251, "1"), (251, "0")])
def test_model_decode_steps(vocab, attn, monkeypatch):
    monkeypatch.setenv("RLA_DECODE_ATTN", attn)
    asked = []
    monkeypatch.setattr(sl, "_ext_with", lambda s, _f=sl._ext_with:
                        (asked.append(s), _f(s))[1])
    m16, m32 = tiny_models(vocab, DEV)
    e_off, e_on, calls = decode_errors(m16, m32, vocab, DEV, monkeypatch, sl)
    assert calls == 2 * 8, "decode_layer did not run once per layer and step"
    assert ("decode_layer_fwd" in asked) == (attn == "1")
    assert e_on <= 2 * e_off


@pytest.mark.parametrize("B,ln_dtype", [(65, torch.float32), (3, BF16)])
def test_composed_path_where_the_kernels_do_not_serve(B, ln_dtype,
                                                      monkeypatch):
    """More than 64 rows, or LayerNorm parameters the kernel does not take:
    the parent's path, not the twin."""
    m16, _ = tiny_models(256, DEV)
    for mod in m16.modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.to(ln_dtype)
    calls = []
    monkeypatch.setattr(sl, "decode_layer", lambda *a: calls.append(1))
    monkeypatch.setattr(sl, "_twin", lambda *a: calls.append(1))
    idx = torch.randint(0, 256, (B, 8),
                        generator=torch.Generator().manual_seed(2)).to(DEV)
    on = m16.generate(idx, 3, temperature=0.0, return_logits=True)
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "0")
    off = m16.generate(idx, 3, temperature=0.0, return_logits=True)
    assert not calls
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
