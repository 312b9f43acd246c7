"""Dropout knobs of GPT-2 and FusedLayerNorm on the CPU (torch
fallback) path: defaults, eval/train semantics, reproducibility, the
two forward compositions, argument checking."""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
from ray_lightning_amd.ops.fused_ln import (FusedLayerNorm,
                                            dropout_add_layer_norm)


def _tiny(**pdrops):
    return GPT2Config(vocab_size=97, n_positions=16, n_embd=32,
                      n_layer=2, n_head=2, **pdrops)


def _pair(p=0.1):
    """Two models with the same weights: dropout off / all three on."""
    torch.manual_seed(0)
    m0 = GPT2(_tiny())
    m1 = GPT2(_tiny(embd_pdrop=p, resid_pdrop=p, attn_pdrop=p))
    m1.load_state_dict(m0.state_dict())
    return m0, m1


def test_config_defaults_are_zero():
    cfg = GPT2Config()
    assert (cfg.embd_pdrop, cfg.resid_pdrop, cfg.attn_pdrop) == (
        0.0, 0.0, 0.0)
    for mk in (GPT2Config.gpt2, GPT2Config.gpt2_xl):
        c = mk()
        assert (c.embd_pdrop, c.resid_pdrop, c.attn_pdrop) == (
            0.0, 0.0, 0.0)


def test_eval_ignores_dropout():
    m0, m1 = _pair()
    m0.eval()
    m1.eval()
    idx = torch.randint(0, 97, (2, 12))
    with torch.no_grad():
        assert torch.equal(m0(idx)[0], m1(idx)[0])


def test_train_forward_differs_and_repeats_under_seed():
    _, m1 = _pair()
    m1.train()
    idx = torch.randint(0, 97, (2, 12))
    with torch.no_grad():
        torch.manual_seed(5)
        a = m1(idx)[0]
        b = m1(idx)[0]
        torch.manual_seed(5)
        c = m1(idx)[0]
    assert not torch.equal(a, b)
    assert torch.equal(a, c)


def test_train_backward_reaches_every_parameter():
    _, m1 = _pair()
    m1.train()
    idx = torch.randint(0, 97, (2, 12))
    tgt = torch.randint(0, 97, (2, 12))
    _, loss = m1(idx, tgt)
    loss.backward()
    for name, p in m1.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_fused_chain_matches_block_composition_in_eval():
    _, m1 = _pair()
    m1.eval()
    idx = torch.randint(0, 97, (2, 12))
    with torch.no_grad():
        logits = m1(idx)[0]
        x = m1.wte(idx) + m1.wpe(torch.arange(12))
        for block in m1.h:
            x = block(x)
        ref = m1.lm_head(m1.ln_f(x))
    assert torch.allclose(logits, ref, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("with_residual", [True, False])
def test_fused_layer_norm_dropout_matches_torch(with_residual):
    torch.manual_seed(1)
    C, p = 32, 0.25
    ln = FusedLayerNorm(C)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    x = torch.randn(6, C)
    res = torch.randn(6, C) if with_residual else None

    torch.manual_seed(7)
    out = ln(x, residual=res, dropout_p=p)
    assert isinstance(out, tuple) and len(out) == 2
    x_new, y = out

    torch.manual_seed(7)
    ref_new = F.dropout(x, p, True)
    if with_residual:
        ref_new = res + ref_new
    assert torch.equal(x_new, ref_new)
    assert (x_new == (res if with_residual else 0)).any()  # some dropped
    assert torch.equal(
        y, F.layer_norm(ref_new, (C,), ln.weight, ln.bias, ln.eps))

    # the functional form is the same op
    torch.manual_seed(7)
    f_new, f_y = dropout_add_layer_norm(x, res, ln.weight, ln.bias,
                                        ln.eps, p, True)
    assert torch.equal(f_new, x_new) and torch.equal(f_y, y)

    # eval: the pair, without dropout
    ln.eval()
    e_new, e_y = ln(x, residual=res, dropout_p=p)
    want = res + x if with_residual else x
    assert torch.equal(e_new, want)
    assert torch.equal(
        e_y, F.layer_norm(want, (C,), ln.weight, ln.bias, ln.eps))


def test_dropout_p_zero_keeps_return_shape():
    ln = FusedLayerNorm(8)
    x, res = torch.randn(3, 8), torch.randn(3, 8)
    assert torch.is_tensor(ln(x, dropout_p=0.0))
    assert torch.equal(ln(x, dropout_p=0.0), ln(x))
    a, b = ln(x, residual=res, dropout_p=0.0)
    c, d = ln(x, residual=res)
    assert torch.equal(a, c) and torch.equal(b, d)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
@pytest.mark.parametrize("training", [True, False])
def test_bad_p_raises(p, training):
    ln = FusedLayerNorm(8).train(training)
    x = torch.randn(3, 8)
    with pytest.raises(ValueError):
        ln(x, dropout_p=p)
    with pytest.raises(ValueError):
        ln(x, residual=x, dropout_p=p)
    with pytest.raises(ValueError):
        dropout_add_layer_norm(x, x, ln.weight, ln.bias, ln.eps, p,
                               training)


def test_flash_attention_dropout_argument():
    from ray_lightning_amd.ops.flash_attn import flash_attention
    torch.manual_seed(3)
    q, k, v = (torch.randn(1, 2, 8, 16) for _ in range(3))
    base = flash_attention(q, k, v)
    assert torch.equal(flash_attention(q, k, v, dropout_p=0.0), base)
    assert not torch.equal(flash_attention(q, k, v, dropout_p=0.5), base)


def test_philox_reference_known_answers():
    """The numpy Philox the GPU tests compare the kernel's mask with
    reproduces the published Philox4x32-10 known-answer vectors."""
    import numpy as np
    from philox_ref import keep_mask, philox4x32_10
    z = np.zeros(1, dtype=np.uint64)
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(w[0]) for w in philox4x32_10((0, 0), (z, z, z, z))] == [
        0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w[0]) for w in philox4x32_10(
        (0xFFFFFFFF, 0xFFFFFFFF), (f, f, f, f))] == [
        0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    m = keep_mask(seed=11, offset=0, numel=1 << 16, p=0.25)
    assert abs(m.mean() - 0.75) < 5 * (0.25 * 0.75 / (1 << 16)) ** 0.5
    assert not np.array_equal(
        m, keep_mask(seed=11, offset=4, numel=1 << 16, p=0.25))


def test_gpt2lm_forwards_pdrops():
    from ray_lightning_amd.models.benchmark import GPT2LM
    import inspect
    sig = inspect.signature(GPT2LM.__init__).parameters
    for name in ("embd_pdrop", "resid_pdrop", "attn_pdrop"):
        assert sig[name].default == 0.0
    lm = GPT2LM(resid_pdrop=0.1, embd_pdrop=0.2, attn_pdrop=0.3,
                bf16_weights=False)
    cfg = lm.model.cfg
    assert (cfg.resid_pdrop, cfg.embd_pdrop, cfg.attn_pdrop) == (
        0.1, 0.2, 0.3)
