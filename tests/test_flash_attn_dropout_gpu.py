"""Attention dropout inside the v3 flash attention kernels: the mask
against the numpy Philox reference bit for bit, numerics against fp32
torch given the mask, and the gate in ``flash_attention``.

The mask is never materialised by the op, so the tests recover it
through the op. With ``q = k = 0`` the probabilities are uniform over
the causal row (``P[q, kv] = 1/(q+1) > 0``), so
- forward: with ``V`` zero except rows ``[64c, 64c+64)`` = identity,
  ``o[b,h,q,d] != 0`` iff ``(q, 64c+d)`` is kept;
- dkv: with ``dO`` that one-hot block, ``dV[b,h,kv,d] != 0`` iff
  ``(64c+d, kv)`` is kept;
re-seeding before each call makes every call draw the same
``(seed, offset)``."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

# the custom path must be the one under test — fail loudly if the HIP
# extension did not load on a GPU box (no silent eager fallback)
from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from philox_ref import keep_mask  # noqa: E402
from ray_lightning_amd.ops import flash_attn as fa  # noqa: E402
from ray_lightning_amd.ops.flash_attn import flash_attention  # noqa: E402

HS = 64
SCALE = 1.0 / math.sqrt(HS)
BF16 = torch.bfloat16

# the smallest shapes that reach each path: one diagonal tile; an
# off-diagonal tile, both LDS buffers and bh > 0 in the counter; buffer
# alternation over 4 tiles
SHAPES = [(1, 1, 64), (2, 3, 128), (1, 2, 256)]
PS = [0.1, 0.5]
_ids = [f"B{b}H{h}T{t}" for b, h, t in SHAPES]


@pytest.fixture(autouse=True)
def _custom_path(monkeypatch):
    monkeypatch.setenv("RLA_FLASH", "1")
    monkeypatch.setenv("RLA_FLASH_DROPOUT", "1")
    monkeypatch.delenv("RLA_FLASH_SHFL", raising=False)


def _ext():
    return _ops._load_ext()


def _tril(T):
    return torch.tril(torch.ones(T, T, device="cuda", dtype=torch.bool))


@functools.lru_cache(maxsize=None)
def ref_mask(B, H, T, p, seed, offset=0):
    """philox_ref's mask for the [B, H, T, T] probabilities, on the
    causal region (False elsewhere)."""
    m = keep_mask(seed, offset, B * H * T * T, p).reshape(B, H, T, T)
    return torch.from_numpy(m).cuda() & _tril(T)


def _one_hot_block(B, H, T, c):
    x = torch.zeros(B, H, T, HS, device="cuda", dtype=BF16)
    x[:, :, 64 * c:64 * c + 64, :] = torch.eye(
        HS, device="cuda", dtype=BF16)
    return x


@functools.lru_cache(maxsize=None)
def recover_fwd_mask(B, H, T, p, seed, use_permlane, skip=0):
    """Keep mask (causal region) of the forward call number ``skip``
    after ``manual_seed(seed)``, read off ``o``."""
    ext = _ext()
    z = torch.zeros(B, H, T, HS, device="cuda", dtype=BF16)
    m = torch.zeros(B, H, T, T, device="cuda", dtype=torch.bool)
    for c in range(T // 64):
        v = _one_hot_block(B, H, T, c)
        torch.manual_seed(seed)
        for _ in range(skip):
            ext.flash_attn_fwd_v3_dropout(z, z, v, SCALE, p, use_permlane)
        o, _lse, s, off = ext.flash_attn_fwd_v3_dropout(
            z, z, v, SCALE, p, use_permlane)
        assert (s, off) == (seed, 4 * skip)
        m[..., 64 * c:64 * c + 64] = o != 0
    return m


@functools.lru_cache(maxsize=None)
def recover_dkv_mask(B, H, T, p, seed, use_permlane, offset=0):
    """Keep mask (causal region) the dkv kernel regenerates from
    ``(seed, offset)``, read off ``dV``."""
    ext = _ext()
    z = torch.zeros(B, H, T, HS, device="cuda", dtype=BF16)
    # lse of the uniform causal row; o only enters D, which dV ignores
    lse = torch.log(torch.arange(1, T + 1, device="cuda",
                                 dtype=torch.float32)).expand(
        B, H, T).contiguous()
    m = torch.zeros(B, H, T, T, device="cuda", dtype=torch.bool)
    for c in range(T // 64):
        dout = _one_hot_block(B, H, T, c)
        _dq, _dk, dv = ext.flash_attn_bwd_v3_dropout(
            dout, z, z, z, z, lse, SCALE, p, seed, offset, use_permlane)
        # dv[b,h,kv,d] <-> (q = 64c+d, kv)
        m[:, :, 64 * c:64 * c + 64, :] = (dv != 0).transpose(-1, -2)
    return m


# ------------------------------------------------------------- 1. mask
@pytest.mark.parametrize("use_permlane", [True, False])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,H,T", SHAPES, ids=_ids)
def test_mask_is_philox_ref_bit_for_bit(B, H, T, p, use_permlane):
    seed = 100 + T
    for call in range(2):
        want = ref_mask(B, H, T, p, seed, 4 * call)
        fwd = recover_fwd_mask(B, H, T, p, seed, use_permlane, call)
        assert torch.equal(fwd, want), f"fwd, call {call}"
        dkv = recover_dkv_mask(B, H, T, p, seed, use_permlane, 4 * call)
        assert torch.equal(dkv, want), f"dkv, call {call}"


# --------------------------------------------------------- 2. numerics
def _inputs(B, H, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.randn(B, H, T, HS, device="cuda", generator=g)
             * 0.5).to(BF16) for _ in range(4)]


def _ref_dropout_attention(q, k, v, M, p):
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~_tril(q.shape[2]), float("-inf"))
    pr = torch.softmax(s, dim=-1) * M / (1.0 - p)
    return pr @ v, torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("shfl", [False, True])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,H,T", SHAPES, ids=_ids)
def test_numerics_against_fp32_given_the_mask(B, H, T, p, shfl,
                                              monkeypatch):
    """Max abs errors measured on MI355X are recorded in
    profiles/flash_attn_dropout.md."""
    if shfl:
        monkeypatch.setenv("RLA_FLASH_SHFL", "1")
    seed = 100 + T
    M = recover_fwd_mask(B, H, T, p, seed, not shfl).float()
    q, k, v, dy = _inputs(B, H, T, seed)
    for t in (q, k, v):
        t.requires_grad_(True)
    torch.manual_seed(seed)
    o = flash_attention(q, k, v, dropout_p=p)
    lse = [t for t in o.grad_fn.saved_tensors if t.dim() == 3][0]
    o.backward(dy)

    q32, k32, v32 = (t.detach().float().requires_grad_(True)
                     for t in (q, k, v))
    ref, lse_ref = _ref_dropout_attention(q32, k32, v32, M, p)
    ref.backward(dy.float())

    s = 1.0 / (1.0 - p)

    def close(name, got, want, atol, rtol):
        err = (got.float() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert torch.allclose(got.float(), want, atol=atol,
                              rtol=rtol), f"{name} max err {err}"

    close("o", o, ref, 3e-2 * s, 3e-2)
    close("lse", lse, lse_ref.detach(), 2e-2, 2e-2)
    close("dq", q.grad, q32.grad, 5e-2 * s, 5e-2)
    close("dk", k.grad, k32.grad, 5e-2 * s, 5e-2)
    close("dv", v.grad, v32.grad, 5e-2 * s, 5e-2)


# -------------------------------------------------------- 3. keep rate
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,H,T", SHAPES, ids=_ids)
def test_keep_rate(B, H, T, p):
    m = recover_fwd_mask(B, H, T, p, 100 + T, True)
    n = B * H * T * (T + 1) // 2
    kept = m.sum().item()
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"keep rate {kept / n:.5f}, {(kept / n - (1 - p)) / sigma:+.2f} "
          f"sigma")
    assert abs(kept / n - (1 - p)) <= 5 * sigma


# ------------------------------------------------ 4. fully dropped row
def test_fully_dropped_row():
    B, H, T, p, seed = 2, 3, 128, 0.5, 228
    assert not ref_mask(B, H, T, p, seed)[0, 0, 1].any()
    q, k, v, dy = _inputs(B, H, T, seed)
    for t in (q, k, v):
        t.requires_grad_(True)
    torch.manual_seed(seed)
    o = flash_attention(q, k, v, dropout_p=p)
    o.backward(dy)
    assert (o[0, 0, 1] == 0).all()
    assert o[0, 0, 0].abs().sum() + o[0, 0, 2].abs().sum() > 0
    for t in (o, q.grad, k.grad, v.grad):
        assert torch.isfinite(t).all()


# ------------------------------------------------- 5. nothing T x T kept
@pytest.mark.parametrize("B,H,T", SHAPES, ids=_ids)
def test_saved_tensors(B, H, T):
    q, k, v, _ = _inputs(B, H, T, 1)
    q.requires_grad_(True)
    o = flash_attention(q, k, v, dropout_p=0.1)
    n = B * H * T
    assert sorted(t.numel() for t in o.grad_fn.saved_tensors) == sorted(
        [n * HS] * 4 + [n])


# ------------------------------------------------------ 6. determinism
def test_deterministic_under_seed_and_advancing():
    B, H, T, p, seed = 2, 3, 128, 0.1, 7
    q0, k0, v0, dy = _inputs(B, H, T, seed)

    def run():
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        o = flash_attention(q, k, v, dropout_p=p)
        o.backward(dy)
        return o.detach(), q.grad, k.grad, v.grad

    torch.manual_seed(seed)
    first = run()
    second = run()           # no reseed: the generator has moved on
    torch.manual_seed(seed)
    again = run()
    for a, c in zip(first, again):
        assert torch.equal(a, c)
    assert not torch.equal(first[0], second[0])


# ------------------------------------------------------------- 7. gate
def _is_dropout_fn(o):
    return o.grad_fn is not None and \
        o.grad_fn.name() == "_FlashAttnDropoutBackward"


def test_gate_usable_call_takes_the_dropout_kernels():
    q, k, v, _ = _inputs(1, 2, 64, 3)
    q.requires_grad_(True)
    assert _is_dropout_fn(flash_attention(q, k, v, dropout_p=0.1))
    assert not _is_dropout_fn(flash_attention(q, k, v))


def test_gate_default_is_what_the_module_records(monkeypatch):
    monkeypatch.delenv("RLA_FLASH_DROPOUT")
    q, k, v, _ = _inputs(1, 2, 64, 3)
    q.requires_grad_(True)
    o = flash_attention(q, k, v, dropout_p=0.1)
    assert _is_dropout_fn(o) == fa._DROPOUT_DEFAULT
    monkeypatch.setenv("RLA_FLASH_DROPOUT", "0")
    assert not _is_dropout_fn(flash_attention(q, k, v, dropout_p=0.1))


@pytest.mark.parametrize("case", ["T32", "hs32", "fp32", "RLA_FLASH=0"])
def test_gate_fallbacks_still_drop(case, monkeypatch):
    T, hs, dtype = 64, 64, BF16
    if case == "T32":
        T = 32
    elif case == "hs32":
        hs = 32
    elif case == "fp32":
        dtype = torch.float32
    else:
        monkeypatch.setenv("RLA_FLASH", "0")
    g = torch.Generator(device="cuda").manual_seed(4)
    q, k, v = (torch.randn(1, 2, T, hs, device="cuda", generator=g).to(
        dtype) for _ in range(3))
    q.requires_grad_(True)
    torch.manual_seed(4)
    o = flash_attention(q, k, v, dropout_p=0.5)
    assert not _is_dropout_fn(o)
    assert not torch.equal(o, flash_attention(q, k, v))


def test_gate_p0_is_the_dropout_free_call():
    q, k, v, _ = _inputs(1, 2, 64, 5)
    assert torch.equal(flash_attention(q, k, v, dropout_p=0.0),
                       flash_attention(q, k, v))


def test_gate_mismatched_kv_falls_back():
    q = _inputs(1, 2, 64, 6)[0]
    k, v = _inputs(1, 2, 128, 6)[:2]
    want = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    assert torch.equal(flash_attention(q, k, v), want)
    q.requires_grad_(True)
    assert not _is_dropout_fn(flash_attention(q, k, v, dropout_p=0.1))
    # dtype mismatch never reaches the kernels either
    assert not fa._usable(q, k[:, :, :64].float(), v[:, :, :64].float())


@pytest.mark.parametrize("bad", [1.0, -0.1])
def test_gate_bad_p_raises(bad):
    q, k, v, _ = _inputs(1, 1, 64, 7)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, dropout_p=bad)


def test_ext_entry_points_check_their_operands():
    ext = _ext()
    q, k, v, dy = _inputs(1, 1, 64, 8)
    k2 = _inputs(1, 1, 128, 8)[0]
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3_dropout(q, k2, v, SCALE, 0.1, True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3_dropout(q, k, v.float(), SCALE, 0.1, True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3_dropout(q, k, v, SCALE, 1.0, True)
    o, lse, seed, off = ext.flash_attn_fwd_v3_dropout(q, k, v, SCALE, 0.1,
                                                      True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_bwd_v3_dropout(dy, q, k2, v, o, lse, SCALE, 0.1,
                                      seed, off, True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_bwd_v3_dropout(dy[:, :, :32], q, k, v, o, lse,
                                      SCALE, 0.1, seed, off, True)

    # the p = 0 entry points share the checks. Every bad operand is
    # larger than the good one would be.
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3(q, k2, v, SCALE, True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3(q, k, v.float(), SCALE, True)
    o, lse = ext.flash_attn_fwd_v3(q, k, v, SCALE, True)
    o2, dy2 = torch.zeros_like(k2), torch.zeros_like(k2)
    for bad in (dict(k=k2), dict(v=v.float()), dict(o=o2), dict(dout=dy2),
                dict(lse=torch.cat([lse, lse])), dict(lse=lse.double())):
        a = dict(dout=dy, q=q, k=k, v=v, o=o, lse=lse)
        a.update(bad)
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_v3(a["dout"], a["q"], a["k"], a["v"],
                                  a["o"], a["lse"], SCALE, True)
    # and the good operands pass
    ext.flash_attn_bwd_v3(dy, q, k, v, o, lse, SCALE, True)


# ------------------------------------------------------------ 8. GPT-2
def _gpt2(attn_pdrop):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    torch.manual_seed(2)
    cfg = GPT2Config(vocab_size=503, n_positions=64, n_embd=256,
                     n_layer=2, n_head=4, attn_pdrop=attn_pdrop)
    return to_bf16_training(GPT2(cfg).cuda())


def test_gpt2_end_to_end(monkeypatch):
    calls = []
    real = fa._dropout_kernels_enabled
    monkeypatch.setattr(fa, "_dropout_kernels_enabled",
                        lambda: calls.append(1) or real())
    m0, m1 = _gpt2(0.0), _gpt2(0.1)
    m1.load_state_dict(m0.state_dict())
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = torch.randint(0, 503, (2, 64), device="cuda", generator=g)
    tgt = torch.randint(0, 503, (2, 64), device="cuda", generator=g)

    m1.train()
    with torch.no_grad():
        torch.manual_seed(9)
        a = m1(idx)[0]
        b = m1(idx)[0]
        torch.manual_seed(9)
        c = m1(idx)[0]
    assert len(calls) == 3 * 2   # every layer took the dropout kernels
    assert torch.equal(a, c)
    assert not torch.equal(a, b)

    _, loss = m1(idx, tgt)
    loss.backward()
    assert torch.isfinite(loss)
    for name, prm in m1.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name

    m0.eval()
    m1.eval()
    with torch.no_grad():
        assert torch.equal(m0(idx)[0], m1(idx)[0])
