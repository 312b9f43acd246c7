"""Numerics for the fused residual-add+LayerNorm CDNA4 kernels vs
plain fp32 torch reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

# the fused path must be the one under test — fail loudly if the HIP
# extension did not load on a GPU box (no silent eager fallback)
from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"



@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("C", [1600, 768, 2048])
def test_fused_ln_plain(dtype, C):
    from ray_lightning_amd.ops.fused_ln import FusedLayerNorm
    torch.manual_seed(0)
    R = 512
    x = (torch.randn(4, R // 4, C, device="cuda") * 2).to(
        dtype).requires_grad_(True)
    ln = FusedLayerNorm(C).to("cuda").float()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    y = ln(x)
    dy = torch.randn_like(y)
    y.backward(dy)

    x32 = x.detach().float().requires_grad_(True)
    w32 = ln.weight.detach().clone().requires_grad_(True)
    b32 = ln.bias.detach().clone().requires_grad_(True)
    y32 = torch.nn.functional.layer_norm(x32, (C,), w32, b32, ln.eps)
    y32.backward(dy.float())

    tol = dict(atol=5e-2, rtol=5e-2) if dtype == torch.bfloat16 else \
        dict(atol=1e-4, rtol=1e-4)
    assert torch.allclose(y.float(), y32, **tol)
    assert torch.allclose(x.grad.float(), x32.grad, **tol)
    rtol = dict(atol=5e-1, rtol=3e-2) if dtype == torch.bfloat16 else \
        dict(atol=1e-2, rtol=1e-4)
    assert torch.allclose(ln.weight.grad, w32.grad, **rtol)
    assert torch.allclose(ln.bias.grad, b32.grad, **rtol)


def test_fused_add_ln_chain():
    """x_new = residual + sub; y = ln(x_new); grads flow into both
    inputs and into x_new's other consumer."""
    from ray_lightning_amd.ops.fused_ln import FusedLayerNorm
    torch.manual_seed(1)
    C, R = 1600, 256
    res = torch.randn(R, C, device="cuda", dtype=torch.bfloat16
                      ).requires_grad_(True)
    sub = torch.randn(R, C, device="cuda", dtype=torch.bfloat16
                      ).requires_grad_(True)
    ln = FusedLayerNorm(C).to("cuda").float()
    x_new, y = ln(sub, residual=res)
    # x_new feeds a second consumer (like the next residual chain)
    loss = y.float().pow(2).mean() + x_new.float().mean()
    loss.backward()

    res32 = res.detach().float().requires_grad_(True)
    sub32 = sub.detach().float().requires_grad_(True)
    xn32 = res32 + sub32
    y32 = torch.nn.functional.layer_norm(
        xn32, (C,), ln.weight.detach().double().float(),
        ln.bias.detach().clone(), ln.eps)
    (y32.pow(2).mean() + xn32.mean()).backward()

    assert torch.allclose(x_new.float(), xn32, atol=5e-2, rtol=5e-2)
    assert torch.allclose(y.float(), y32, atol=5e-2, rtol=5e-2)
    assert torch.allclose(res.grad.float(), res32.grad, atol=5e-2,
                          rtol=5e-2)
    assert torch.allclose(sub.grad.float(), sub32.grad, atol=5e-2,
                          rtol=5e-2)


def test_gpt2_fused_chain_matches_eager_blocks():
    """GPT2.forward's cross-block fused chain == the unfused Block
    composition on the same weights."""
    from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
    torch.manual_seed(2)
    cfg = GPT2Config(vocab_size=503, n_positions=64, n_embd=256,
                     n_layer=3, n_head=4)
    m = GPT2(cfg).to("cuda")
    idx = torch.randint(0, 503, (2, 32), device="cuda")
    logits, _ = m(idx)

    # eager reference: plain Block.forward composition
    x = m.wte(idx) + m.wpe(torch.arange(32, device="cuda"))
    for block in m.h:
        x = x + block.attn(torch.nn.functional.layer_norm(
            x, (256,), block.ln_1.weight, block.ln_1.bias,
            block.ln_1.eps))
        x = x + block.mlp(torch.nn.functional.layer_norm(
            x, (256,), block.ln_2.weight, block.ln_2.bias,
            block.ln_2.eps))
    x = torch.nn.functional.layer_norm(
        x, (256,), m.ln_f.weight, m.ln_f.bias, m.ln_f.eps)
    ref = m.lm_head(x)
    assert torch.allclose(logits, ref, atol=1e-3, rtol=1e-3)


def test_ext_entry_points_check_their_operands():
    """fused_ln_fwd / fused_ln_bwd are importable entry points: operands
    the kernels cannot take raise from the host checks, before anything
    is allocated or launched, and a valid call still works afterwards."""
    ext = _ops._load_ext()
    bf, R, C, eps = torch.bfloat16, 3, 8, 1e-5
    g = torch.Generator(device="cuda").manual_seed(11)

    def rows(r=R, c=C, dtype=bf):
        return torch.randn(r, c, device="cuda", generator=g).to(dtype)

    def vec(n, dtype=torch.float32):
        return torch.rand(n, device="cuda", generator=g).add(0.5).to(dtype)

    sub, res, gamma, beta = rows(), rows(), vec(C), vec(C)
    for bad in (
        (sub, rows(R, 16), gamma, beta, eps, 0.0),
        (sub, rows(dtype=torch.float32), gamma, beta, eps, 0.0),
        (rows(C, R).t(), res, gamma, beta, eps, 0.0),
        (rows(dtype=torch.float16), None, gamma, beta, eps, 0.0),
        (rows(R, 12), None, vec(12), vec(12), eps, 0.0),
        (sub, res, vec(16), beta, eps, 0.0),
        (sub, res, vec(C, bf), beta, eps, 0.0),
        (sub, res, gamma, beta, eps, 1.0),
    ):
        with pytest.raises(RuntimeError):
            ext.fused_ln_fwd(*bad)

    dy, dext, mean, invstd = rows(), rows(), vec(R), vec(R)
    half = torch.float16
    for bad in (
        (rows(dtype=half), rows(dtype=half), None, gamma, mean, invstd),
        (dy, rows(C, R).t(), None, gamma, mean, invstd),
        (dy, sub, rows(dtype=torch.float32), gamma, mean, invstd),
        (rows(2), sub, dext, gamma, mean, invstd),
        (dy, sub, dext, gamma, vec(2), invstd),
        (dy, sub, dext, gamma, mean, vec(R, torch.float64)),
        (dy, sub, dext, vec(16), mean, invstd),
    ):
        with pytest.raises(RuntimeError):
            ext.fused_ln_bwd(*bad, 0.0, 0, 0, True)

    y, x_new, mean, invstd, seed, offset = ext.fused_ln_fwd(
        sub, res, gamma, beta, eps, 0.0)
    assert (seed, offset) == (0, 0)
    d_res, d_sub, dgamma, dbeta = ext.fused_ln_bwd(
        dy, x_new, dext, gamma, mean, invstd, 0.0, 0, 0, True)

    sub32 = sub.float().requires_grad_(True)
    res32 = res.float().requires_grad_(True)
    g32 = gamma.clone().requires_grad_(True)
    b32 = beta.clone().requires_grad_(True)
    xn32 = res32 + sub32
    y32 = torch.nn.functional.layer_norm(xn32, (C,), g32, b32, eps)
    torch.autograd.backward([xn32, y32], [dext.float(), dy.float()])
    tol = dict(atol=5e-2, rtol=5e-2)
    gb = dict(atol=5e-1, rtol=3e-2)
    assert torch.allclose(x_new.float(), xn32, **tol)
    assert torch.allclose(y.float(), y32, **tol)
    assert torch.allclose(d_res.float(), res32.grad, **tol)
    assert torch.allclose(d_sub.float(), sub32.grad, **tol)
    assert torch.allclose(dgamma, g32.grad, **gb)
    assert torch.allclose(dbeta, b32.grad, **gb)
