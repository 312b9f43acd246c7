"""ignore_index, label smoothing, z-loss and reduction of the chunked
linear + cross-entropy (torch path) against autograd through
``F.cross_entropy`` plus the z-loss term."""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_amd.ops.chunked_ce import chunked_cross_entropy

N, C, V, CHUNK = 64, 32, 97, 17


def _targets(ignore_index, seed=0):
    """About a fifth ignored, and the whole second chunk ignored."""
    g = torch.Generator().manual_seed(seed)
    hi = V - 1 if ignore_index == V - 1 else V
    t = torch.randint(0, hi, (N,), generator=g)
    t[torch.rand(N, generator=g) < 0.2] = ignore_index
    t[CHUNK:2 * CHUNK] = ignore_index
    assert (t != ignore_index).sum() > N // 2
    return t


def _inputs(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, generator=g) * 0.5).to(dtype)
    w = (torch.randn(V, C, generator=g) * 0.1).to(dtype)
    return x, w


def reference(x, w, t, ignore_index=-100, label_smoothing=0.0, z_loss=0.0,
              reduction="mean"):
    """Loss and grads by autograd on the full fp32 logits."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    logits = (x @ w.t()).float()
    loss = F.cross_entropy(logits, t, ignore_index=ignore_index,
                           label_smoothing=label_smoothing,
                           reduction=reduction)
    valid = t != ignore_index
    lse2 = torch.logsumexp(logits, dim=-1)[valid].pow(2)
    loss = loss + z_loss * (lse2.mean() if reduction == "mean"
                            else lse2.sum())
    loss.backward()
    return loss.detach(), x.grad, w.grad


OPTION_SETS = [
    dict(),
    dict(label_smoothing=0.1),
    dict(z_loss=1e-3),
    dict(reduction="sum"),
    dict(label_smoothing=0.1, z_loss=1e-3, reduction="sum"),
    dict(label_smoothing=0.1, z_loss=1e-3),
]


@pytest.mark.parametrize("opts", OPTION_SETS,
                         ids=lambda o: "-".join(o) or "plain")
@pytest.mark.parametrize("ignore_index", [-100, V - 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
def test_matches_reference(dtype, ignore_index, opts):
    x, w = _inputs(dtype)
    t = _targets(ignore_index)
    x.requires_grad_(True)
    w.requires_grad_(True)
    loss = chunked_cross_entropy(x, w, t, chunk_rows=CHUNK,
                                 ignore_index=ignore_index, **opts)
    loss.backward()
    ref, dx, dw = reference(x, w, t, ignore_index=ignore_index, **opts)
    tol = dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else \
        dict(atol=2e-2, rtol=2e-2)
    assert torch.allclose(loss, ref, **tol), (loss, ref)
    assert torch.allclose(x.grad.float(), dx.float(), **tol)
    assert torch.allclose(w.grad.float(), dw.float(), **tol)
    # ignored rows get no gradient at all
    assert torch.equal(x.grad[t == ignore_index],
                       torch.zeros_like(x.grad[t == ignore_index]))


def test_mean_uses_global_count():
    """With one chunk fully ignored, a per-chunk mean would differ:
    sum / mean must be exactly the number of valid rows."""
    x, w = _inputs(torch.float32)
    t = _targets(-100)
    s = chunked_cross_entropy(x, w, t, chunk_rows=CHUNK, reduction="sum")
    m = chunked_cross_entropy(x, w, t, chunk_rows=CHUNK, reduction="mean")
    assert torch.allclose(s / m, (t != -100).sum().float())


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_all_ignored_is_zero(reduction):
    x, w = _inputs(torch.float32)
    x.requires_grad_(True)
    w.requires_grad_(True)
    t = torch.full((N,), -100)
    loss = chunked_cross_entropy(x, w, t, chunk_rows=CHUNK,
                                 label_smoothing=0.1, z_loss=1e-3,
                                 reduction=reduction)
    loss.backward()
    assert loss.item() == 0.0
    assert torch.equal(x.grad, torch.zeros_like(x))
    assert torch.equal(w.grad, torch.zeros_like(w))


@pytest.mark.parametrize("bad", [
    dict(label_smoothing=1.0), dict(label_smoothing=-0.1),
    dict(z_loss=-1e-4), dict(reduction="none")],
    ids=["ls-1", "ls-neg", "z-neg", "reduction"])
def test_validation(bad):
    x, w = _inputs(torch.float32)
    with pytest.raises(ValueError):
        chunked_cross_entropy(x, w, _targets(-100), chunk_rows=CHUNK, **bad)


def test_defaults_unchanged():
    """No new keyword == the keywords at their defaults, bitwise, and
    both equal the plain mean CE when nothing is ignored."""
    x, w = _inputs(torch.float32)
    t = torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(3))
    out = []
    for kw in (dict(), dict(ignore_index=-100, label_smoothing=0.0,
                            z_loss=0.0, reduction="mean")):
        xa = x.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        loss = chunked_cross_entropy(xa, wa, t, CHUNK, **kw)
        loss.backward()
        out.append((loss.detach(), xa.grad, wa.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    ref, dx, dw = reference(x, w, t)
    assert torch.allclose(out[0][0], ref, atol=1e-5, rtol=1e-5)
    assert torch.allclose(out[0][1], dx, atol=1e-5, rtol=1e-5)


def test_gpt2_passes_options():
    from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config
    torch.manual_seed(1)
    cfg = GPT2Config(vocab_size=211, n_positions=32, n_embd=32, n_layer=2,
                     n_head=2, label_smoothing=0.1, z_loss=1e-4)
    m = GPT2(cfg)
    idx = torch.randint(0, 211, (2, 16))
    y = torch.randint(0, 211, (2, 16))
    y[0, :5] = -100
    y[1, 9:] = -100
    _, loss = m(idx, y)
    with torch.no_grad():
        logits, _ = m(idx)
    logits = logits.reshape(-1, 211).float()
    yf = y.reshape(-1)
    ref = F.cross_entropy(logits, yf, ignore_index=-100,
                          label_smoothing=0.1)
    ref = ref + 1e-4 * torch.logsumexp(
        logits, dim=-1)[yf != -100].pow(2).mean()
    assert torch.allclose(loss, ref, atol=1e-5, rtol=1e-5), (loss, ref)
    loss.backward()
    assert m.wte.weight.grad is not None


def test_gpt2lm_forwards_options():
    from ray_lightning_amd.models.benchmark import GPT2LM
    import inspect
    sig = inspect.signature(GPT2LM.__init__).parameters
    for name, default in (("ignore_index", -100),
                          ("label_smoothing", 0.0), ("z_loss", 0.0)):
        assert sig[name].default == default
    lm = GPT2LM(ignore_index=0, label_smoothing=0.05, z_loss=2e-4,
                bf16_weights=False)
    cfg = lm.model.cfg
    assert (cfg.ignore_index, cfg.label_smoothing, cfg.z_loss) == (
        0, 0.05, 2e-4)
