"""Fused dropout + residual-add + LayerNorm CDNA4 kernels: numerics
against fp32 torch given the mask, and the properties of the mask
itself. The mask is never materialised by the op, so the tests recover
it through the op: with ``residual = 0`` and ``sub = 1`` in fp32,
``x_new = M / (1-p)``; reseeding before the call under test makes it
draw the same ``M``."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

# the fused path must be the one under test — fail loudly if the HIP
# extension did not load on a GPU box (no silent eager fallback)
from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops.fused_ln import (FusedLayerNorm,  # noqa: E402
                                            dropout_add_layer_norm)

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-5

# (dtype, C, R): the smallest shapes that reach each code path
SHAPES = [
    (BF16, 1600, 64),   # GPT-2-XL width, not a multiple of kT*V
    (F32, 1600, 64),
    (BF16, 8, 3),       # one vector slot
    (F32, 4, 3),
    (BF16, 4096, 16),   # nvec > kT: row is not register-staged
    (BF16, 64, 8200),   # more rows than the 8192-block grid cap
    (F32, 64, 8200),
]
_ids = [f"{'bf16' if d == BF16 else 'f32'}-C{c}-R{r}" for d, c, r in SHAPES]


def _affine(C):
    g = torch.Generator(device="cuda").manual_seed(1234)
    w = torch.empty(C, device="cuda").uniform_(0.5, 1.5, generator=g)
    b = torch.empty(C, device="cuda").uniform_(-0.5, 0.5, generator=g)
    return w, b


def recover_mask(R, C, p, seed, dtype=F32):
    """The keep mask the next op call after ``manual_seed(seed)`` draws
    for an [R, C] input, read off x_new = 0 + keep * 1 / (1-p)."""
    w, b = _affine(C)
    sub = torch.ones(R, C, device="cuda", dtype=dtype)
    res = torch.zeros(R, C, device="cuda", dtype=dtype)
    torch.manual_seed(seed)
    x_new, _ = dropout_add_layer_norm(sub, res, w, b, EPS, p, True)
    m = x_new != 0
    # kept entries carry exactly the scale, rounded once to dtype
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(dtype)
    assert torch.equal(x_new, m.to(dtype) * scale.to("cuda"))
    return m


def keep_rate_ok(m, p):
    n = m.numel()
    return abs(m.float().mean().item() - (1 - p)) <= 5 * math.sqrt(
        p * (1 - p) / n)


def _check_numerics(dtype, C, R, p, with_residual):
    seed = 100 + C + R
    M = recover_mask(R, C, p, seed).float()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    w, b = _affine(C)
    w.requires_grad_(True)
    b.requires_grad_(True)
    sub = torch.randn(R, C, device="cuda", generator=gen).to(
        dtype).requires_grad_(True)
    res = (torch.randn(R, C, device="cuda", generator=gen).to(
        dtype).requires_grad_(True) if with_residual else None)
    # grads arriving at y and at x_new's second consumer
    dy = torch.randn(R, C, device="cuda", generator=gen).to(dtype)
    dxn = torch.randn(R, C, device="cuda", generator=gen).to(dtype)

    torch.manual_seed(seed)
    x_new, y = dropout_add_layer_norm(sub, res, w, b, EPS, p, True)
    # nothing mask-sized is kept for backward
    saved = y.grad_fn.saved_tensors
    assert sorted(t.numel() for t in saved) == sorted(
        [R * C, R, R, C])
    torch.autograd.backward([x_new, y], [dxn, dy])

    scale = 1.0 / (1.0 - p)
    sub32 = sub.detach().float().requires_grad_(True)
    w32 = w.detach().clone().requires_grad_(True)
    b32 = b.detach().clone().requires_grad_(True)
    xn32 = sub32 * M * scale
    if with_residual:
        res32 = res.detach().float().requires_grad_(True)
        xn32 = res32 + xn32
    y32 = F.layer_norm(xn32, (C,), w32, b32, EPS)
    torch.autograd.backward([xn32, y32], [dxn.float(), dy.float()])

    bf = dtype == BF16
    tol = dict(atol=5e-2, rtol=5e-2) if bf else dict(atol=1e-4, rtol=1e-4)
    gb = dict(atol=5e-1, rtol=3e-2) if bf else dict(atol=1e-2, rtol=1e-4)
    sub_tol = dict(atol=tol["atol"] * scale, rtol=tol["rtol"])

    def close(name, got, want, t):
        err = (got.float() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert torch.allclose(got.float(), want, **t), name

    close("x_new", x_new, xn32, tol)
    close("y", y, y32, tol)
    close("d_sub", sub.grad, sub32.grad, sub_tol)
    close("dgamma", w.grad, w32.grad, gb)
    close("dbeta", b.grad, b32.grad, gb)
    dropped = M == 0
    if R * C >= 1024:  # a 12-element mask may well keep everything
        assert (dropped.any() or p == 0) and not dropped.all()
    assert (sub.grad[dropped] == 0).all()
    if with_residual:
        close("d_residual", res.grad, res32.grad, tol)
        assert torch.equal(x_new[dropped], res.detach()[dropped])
    else:
        assert (x_new[dropped] == 0).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype,C,R", SHAPES, ids=_ids)
def test_numerics_with_residual(dtype, C, R, p):
    _check_numerics(dtype, C, R, p, True)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype,C,R", SHAPES, ids=_ids)
def test_numerics_no_residual(dtype, C, R, p):
    _check_numerics(dtype, C, R, p, False)


@pytest.mark.parametrize("with_residual", [True, False],
                         ids=["residual", "no_residual"])
@pytest.mark.parametrize("dtype,C,R", SHAPES, ids=_ids)
def test_numerics_without_dropout(dtype, C, R, with_residual):
    """p = 0 runs the dropout-free instantiations of the same kernels
    over the same edge shapes; the recovered mask keeps everything."""
    _check_numerics(dtype, C, R, 0.0, with_residual)


def test_rng_untouched_when_nothing_is_dropped():
    """Only a call that drops draws from the device's generator."""
    R, C = 3, 8
    ln = FusedLayerNorm(C).to("cuda").float()
    x = torch.randn(R, C, device="cuda").to(BF16)
    r = torch.randn(R, C, device="cuda").to(BF16)
    torch.manual_seed(8)
    before = torch.cuda.get_rng_state()
    ln.train()
    ln(x, residual=r, dropout_p=0)
    ln(x, dropout_p=0)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    ln.eval()
    ln(x, residual=r, dropout_p=0.3)
    ln(x, dropout_p=0.3)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    ln.train()
    ln(x, residual=r, dropout_p=0.3)
    assert not torch.equal(torch.cuda.get_rng_state(), before)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_same_past_the_grid_cap(p):
    """Rows handled by a later grid-stride iteration draw from the same
    distribution as the first 8192."""
    M = recover_mask(8200, 64, p, seed=3)
    assert keep_rate_ok(M[:8192], p)
    assert keep_rate_ok(M[8192:], p)


@pytest.mark.parametrize("C,R", [(1600, 64), (8, 3), (4096, 16),
                                 (64, 8200)])
def test_mask_same_for_both_dtypes(C, R):
    assert torch.equal(recover_mask(R, C, 0.5, seed=4, dtype=F32),
                       recover_mask(R, C, 0.5, seed=4, dtype=BF16))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_is_the_documented_function_of_seed_offset_index(p):
    """keep(i) = philox(seed, (offset/4, i>>2))[i&3] >= floor(p*2^32),
    with the offset advancing by 4 per call."""
    from philox_ref import keep_mask
    R, C, seed = 64, 1600, 77
    w, b = _affine(C)
    sub = torch.ones(R, C, device="cuda")
    res = torch.zeros(R, C, device="cuda")
    torch.manual_seed(seed)
    for call in range(2):
        x_new, _ = dropout_add_layer_norm(sub, res, w, b, EPS, p, True)
        want = torch.from_numpy(
            keep_mask(seed, 4 * call, R * C, p)).reshape(R, C)
        assert torch.equal((x_new != 0).cpu(), want), f"call {call}"


def test_reproducible_and_advancing():
    C, R, p, seed = 1600, 64, 0.1, 5
    ln = FusedLayerNorm(C).to("cuda").float()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    sub0 = torch.randn(R, C, device="cuda", generator=gen).to(BF16)
    res0 = torch.randn(R, C, device="cuda", generator=gen).to(BF16)

    def run():
        sub = sub0.clone().requires_grad_(True)
        res = res0.clone().requires_grad_(True)
        ln.zero_grad()
        x_new, y = ln(sub, residual=res, dropout_p=p)
        (y.float().pow(2).mean() + x_new.float().mean()).backward()
        return (x_new, y, sub.grad, res.grad, ln.weight.grad.clone(),
                ln.bias.grad.clone())

    torch.manual_seed(seed)
    first = run()
    second = run()          # no reseed: the generator has moved on
    torch.manual_seed(seed)
    again = run()
    for a, c in zip(first, again):
        assert torch.equal(a, c)
    assert not torch.equal(first[0], second[0])

    # the masks of two consecutive calls are independent draws
    M1 = recover_mask(R, C, p, seed)
    w, b = _affine(C)
    x2, _ = dropout_add_layer_norm(
        torch.ones(R, C, device="cuda"), torch.zeros(R, C, device="cuda"),
        w, b, EPS, p, True)
    M2 = x2 != 0
    assert not torch.equal(M1, M2)
    q = p * p + (1 - p) * (1 - p)
    agree = (M1 == M2).float().mean().item()
    assert abs(agree - q) <= 5 * math.sqrt(q * (1 - q) / (R * C))
    # rows do not repeat
    assert torch.unique(M1, dim=0).shape[0] == R


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    assert keep_rate_ok(recover_mask(64, 1600, p, seed=6), p)


def test_off_switches():
    C, R = 1600, 64
    torch.manual_seed(7)
    ln = FusedLayerNorm(C).to("cuda").float()
    x = torch.randn(R, C, device="cuda").to(BF16)
    r = torch.randn(R, C, device="cuda").to(BF16)
    base_new, base_y = ln(x, residual=r)
    a_new, a_y = ln(x, residual=r, dropout_p=0)
    assert torch.equal(a_new, base_new) and torch.equal(a_y, base_y)
    assert torch.is_tensor(ln(x, dropout_p=0))
    ln.eval()
    e_new, e_y = ln(x, residual=r, dropout_p=0.3)
    assert torch.equal(e_new, base_new) and torch.equal(e_y, base_y)
    n_new, n_y = ln(x, dropout_p=0.3)
    assert torch.equal(n_new, x) and torch.equal(n_y, ln(x))
    for mode in (True, False):
        ln.train(mode)
        for bad in (1.0, -0.1):
            with pytest.raises(ValueError):
                ln(x, residual=r, dropout_p=bad)


# ---------------------------------------------------------------- GPT-2
def _gpt2_pair(**pdrops):
    from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
    shape = dict(vocab_size=503, n_positions=64, n_embd=256, n_layer=3,
                 n_head=4)
    torch.manual_seed(2)
    m0 = GPT2(GPT2Config(**shape)).to("cuda")
    m1 = GPT2(GPT2Config(**shape, **pdrops)).to("cuda")
    m1.load_state_dict(m0.state_dict())
    return m0, m1


def test_gpt2_eval_ignores_dropout():
    m0, m1 = _gpt2_pair(embd_pdrop=0.1, resid_pdrop=0.1, attn_pdrop=0.1)
    m0.eval()
    m1.eval()
    idx = torch.randint(0, 503, (2, 32), device="cuda")
    with torch.no_grad():
        assert torch.equal(m0(idx)[0], m1(idx)[0])


def test_gpt2_train_differs_and_repeats_under_seed():
    _, m1 = _gpt2_pair(embd_pdrop=0.1, resid_pdrop=0.1)
    m1.train()
    idx = torch.randint(0, 503, (2, 32), device="cuda")
    with torch.no_grad():
        torch.manual_seed(9)
        a = m1(idx)[0]
        b = m1(idx)[0]
        torch.manual_seed(9)
        c = m1(idx)[0]
    assert not torch.equal(a, b)
    assert torch.equal(a, c)


@pytest.mark.parametrize("attn_pdrop", [0.0, 0.1])
def test_gpt2_train_backward_finite(attn_pdrop):
    """attn_pdrop > 0 is the SDPA fallback: only finiteness is checked."""
    _, m1 = _gpt2_pair(embd_pdrop=0.1, resid_pdrop=0.1,
                       attn_pdrop=attn_pdrop)
    m1.train()
    idx = torch.randint(0, 503, (2, 32), device="cuda")
    tgt = torch.randint(0, 503, (2, 32), device="cuda")
    _, loss = m1(idx, tgt)
    loss.backward()
    assert torch.isfinite(loss)
    for name, prm in m1.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
