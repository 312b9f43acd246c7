"""Fused cross-entropy CDNA4 kernels (ignore_index, label smoothing,
z-loss): kernel-level numerics against fp32 torch on the same logits,
the op against the torch path, and a short GPT-2 run."""
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

from ray_lightning_amd.ops import chunked_ce  # noqa: E402
from ray_lightning_amd.ops.chunked_ce import (  # noqa: E402
    chunked_cross_entropy)

BF16, F32 = torch.bfloat16, torch.float32
GRID_CAP = 8192  # kMaxGrid in csrc/fused_ce.hip

# (V, R): the smallest shapes that reach each code path
SHAPES = [
    (7, 3),         # shorter than one vector: all head and tail
    (97, 5),        # odd, fewer elements than threads, rows misaligned
    (2051, 4),      # > 256 x 8 elements, odd: several trips plus a tail
    (4096, 2),      # fully aligned, no peel
    (50257, 3),     # the real width
    (64, GRID_CAP + 8),  # more rows than the grid: grid-stride loop
]
OPTS = [
    dict(label_smoothing=0.0, z_loss=0.0),
    dict(label_smoothing=0.1, z_loss=0.0),
    dict(label_smoothing=0.0, z_loss=1e-3),
    dict(label_smoothing=0.1, z_loss=1e-3),
]
_opt_id = {0: "plain", 1: "smooth", 2: "zloss", 3: "all"}


@pytest.fixture(autouse=True)
def _fused_on(monkeypatch):
    monkeypatch.setenv("RLA_FUSED_CE", "1")


def _ext():
    ext = _ops._load_ext()
    # no hasattr guard: a build without the kernels must fail here
    return ext.fused_ce_fwd, ext.fused_ce_bwd


def _case(V, R, dtype, ignore_index):
    """Random logits with the last row scaled to max ~ 300, targets that
    hit column 0 and the last usable column (head and tail peels), and
    one ignored row, between valid ones where there are three rows."""
    g = torch.Generator(device="cuda").manual_seed(V * 131 + R)
    z = torch.randn(R, V, device="cuda", generator=g)
    z[R - 1] *= 300.0 / z[R - 1].max()
    z = z.to(dtype)
    last = V - 2 if ignore_index == V - 1 else V - 1
    t = torch.randint(0, last + 1, (R,), device="cuda", generator=g)
    t[R - 1] = last
    if R >= 3:
        t[0] = 0
        t[1] = ignore_index
        t[2] = last
    else:
        t[0] = ignore_index
    return z, t


def _reference(z, t, ignore_index, label_smoothing, z_loss):
    """fp32 torch on the same logits: per-row loss, lse, and dlogits for
    a unit gradient on every row by autograd."""
    z32 = z.float().detach().requires_grad_(True)
    lse = torch.logsumexp(z32, dim=-1)
    rows = F.cross_entropy(z32, t, ignore_index=ignore_index,
                           label_smoothing=label_smoothing,
                           reduction="none")
    rows = rows + z_loss * lse.pow(2) * (t != ignore_index)
    rows.sum().backward()
    return rows.detach(), lse.detach(), z32.grad


@pytest.mark.parametrize("oi", range(len(OPTS)), ids=_opt_id.get)
@pytest.mark.parametrize("pad", ["m100", "last"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,R", SHAPES, ids=[f"V{v}-R{r}" for v, r in SHAPES])
def test_kernels_match_fp32_torch(V, R, dtype, pad, oi):
    fwd, bwd = _ext()
    opts = OPTS[oi]
    ignore_index = -100 if pad == "m100" else V - 1
    z, t = _case(V, R, dtype, ignore_index)
    assert z[R - 1].float().max().item() == pytest.approx(300, rel=1e-2)
    ref_rows, ref_lse, ref_dz = _reference(z, t, ignore_index, **opts)

    rows, lse, lse_lo = fwd(z, t, ignore_index, opts["label_smoothing"],
                            opts["z_loss"])
    one = torch.ones(1, device="cuda")
    dz = bwd(z, lse, lse_lo, t, one, ignore_index,
             opts["label_smoothing"], opts["z_loss"])
    assert dz.dtype == dtype and dz.data_ptr() != z.data_ptr()

    print(f"max|lse err| {(lse - ref_lse).abs().max().item():.3e}  "
          f"max|loss err| {(rows - ref_rows).abs().max().item():.3e}  "
          f"max|dz err| {(dz.float() - ref_dz).abs().max().item():.3e}")
    assert torch.allclose(lse, ref_lse, rtol=1e-5, atol=1e-5)
    assert torch.allclose(rows, ref_rows, rtol=1e-5, atol=1e-5)
    if dtype == F32:
        assert torch.allclose(dz, ref_dz, rtol=1e-5, atol=1e-6)
    else:
        # one bf16 ulp around the fp32 reference rounded once
        assert torch.allclose(dz.float(), ref_dz.to(BF16).float(),
                              rtol=2.0 ** -7, atol=1e-6)
    ign = t == ignore_index
    assert ign.any() and torch.equal(rows[ign], torch.zeros_like(rows[ign]))
    assert torch.equal(dz[ign], torch.zeros_like(dz[ign]))

    # in place == out of place, bitwise
    z2 = z.clone()
    dz2 = bwd(z2, lse, lse_lo, t, one, ignore_index,
              opts["label_smoothing"], opts["z_loss"], True)
    assert dz2.data_ptr() == z2.data_ptr()
    assert torch.equal(dz2, dz)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_gscale_is_read_on_device(dtype):
    fwd, bwd = _ext()
    z, t = _case(2051, 4, dtype, -100)
    _, _, ref_dz = _reference(z, t, -100, 0.1, 1e-3)
    rows, lse, lse_lo = fwd(z, t, -100, 0.1, 1e-3)
    g = torch.full((1,), 0.37, device="cuda")
    dz = bwd(z, lse, lse_lo, t, g, -100, 0.1, 1e-3)
    ref = ref_dz * 0.37
    if dtype == F32:
        assert torch.allclose(dz, ref, rtol=1e-5, atol=1e-6)
    else:
        assert torch.allclose(dz.float(), ref.to(BF16).float(),
                              rtol=2.0 ** -7, atol=1e-6)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_deterministic(dtype):
    fwd, bwd = _ext()
    z, t = _case(50257, 3, dtype, -100)
    one = torch.ones(1, device="cuda")

    def run():
        rows, lse, lse_lo = fwd(z, t, -100, 0.1, 1e-3)
        return rows, lse, lse_lo, bwd(z, lse, lse_lo, t, one, -100, 0.1,
                                      1e-3)
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


# ------------------------------------------------------------- op level
N, C, V, CHUNK = 300, 64, 1031, 128


def _op_inputs():
    g = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.randn(N, C, device="cuda", generator=g) * 0.5).to(BF16)
    w = (torch.randn(V, C, device="cuda", generator=g) * 0.1).to(BF16)
    t = torch.randint(0, V, (N,), device="cuda", generator=g)
    t[torch.rand(N, device="cuda", generator=g) < 0.2] = -100
    t[CHUNK:2 * CHUNK] = -100  # one chunk fully ignored
    return x, w, t


def _run_op(x, w, t, **kw):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    loss = chunked_cross_entropy(x, w, t, CHUNK, **kw)
    loss.backward()
    return loss.detach().float(), x.grad.float(), w.grad.float()


def test_op_matches_torch_path(monkeypatch):
    """Against the fp32 autograd reference on the same bf16-rounded
    inputs the fused path may be at most twice as far off as the torch
    path (+1e-6): both round dlogits to bf16 once, so their errors are
    two draws of the same rounding."""
    x, w, t = _op_inputs()
    kw = dict(label_smoothing=0.1, z_loss=1e-3, reduction="sum")
    fused = _run_op(x, w, t, **kw)
    monkeypatch.setenv("RLA_FUSED_CE", "0")
    torch_path = _run_op(x, w, t, **kw)

    x32 = x.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    logits = x32 @ w32.t()
    valid = t != -100
    ref = F.cross_entropy(logits, t, ignore_index=-100,
                          label_smoothing=0.1, reduction="sum")
    ref = ref + 1e-3 * torch.logsumexp(logits, -1)[valid].pow(2).sum()
    ref.backward()
    ref32 = (ref.detach(), x32.grad, w32.grad)

    for name, f, p, r in zip(("loss", "dx", "dW"), fused, torch_path,
                             ref32):
        ef = (f - r).abs().max().item()
        ep = (p - r).abs().max().item()
        print(f"{name}: max|fused - ref32| = {ef:.4e}   "
              f"max|torch_path - ref32| = {ep:.4e}")
        assert ef <= 2 * ep + 1e-6, (name, ef, ep)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_op_all_ignored_is_zero(dtype, reduction):
    x, w, _ = _op_inputs()
    t = torch.full((N,), -100, device="cuda")
    loss, dx, dw = _run_op(x.to(dtype), w.to(dtype), t,
                           label_smoothing=0.1, z_loss=1e-3,
                           reduction=reduction)
    assert loss.item() == 0.0
    assert torch.equal(dx, torch.zeros_like(dx))
    assert torch.equal(dw, torch.zeros_like(dw))


def _boom(*a, **k):
    raise AssertionError("fused kernel called")


class _NoFused:
    """The extension with the two CE kernels replaced by a tripwire."""

    def __init__(self, ext):
        self._ext = ext

    def __getattr__(self, name):
        if name in ("fused_ce_fwd", "fused_ce_bwd"):
            return _boom
        return getattr(self._ext, name)


def test_env_selects_path(monkeypatch):
    x, w, t = _op_inputs()
    monkeypatch.setattr(chunked_ce, "_require_ext",
                        lambda: _NoFused(_ops._load_ext()))
    with pytest.raises(AssertionError, match="fused kernel called"):
        _run_op(x, w, t)        # RLA_FUSED_CE=1: the kernels run
    monkeypatch.setenv("RLA_FUSED_CE", "0")
    loss, dx, _ = _run_op(x, w, t)   # torch path never touches them
    assert torch.isfinite(loss) and torch.isfinite(dx).all()


def test_missing_kernel_is_an_error(monkeypatch):
    class Old:
        pass
    x, w, t = _op_inputs()
    monkeypatch.setattr(chunked_ce, "_require_ext", lambda: Old())
    with pytest.raises(RuntimeError, match="rebuild with"):
        chunked_cross_entropy(x, w, t, CHUNK)


# ----------------------------------------------------------- end to end
def _train3():
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    from ray_lightning_amd.optim import ShardedFusedAdam
    torch.manual_seed(5)
    # head size 64, T = 64: the flash kernels engage
    cfg = GPT2Config(vocab_size=1031, n_positions=64, n_embd=64,
                     n_layer=2, n_head=1, label_smoothing=0.1)
    model = to_bf16_training(GPT2(cfg).cuda())
    opt = ShardedFusedAdam(model.parameters(), lr=1e-2)
    idx = torch.randint(0, 1031, (4, 64), device="cuda")
    y = torch.randint(0, 1031, (4, 64), device="cuda")
    y[:, 40:] = -100   # right-padded batch
    y[2, 10:] = -100
    losses = []
    for _ in range(3):
        _, loss = model(idx, y)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(loss.detach().item())
    return losses


def test_gpt2_trains_with_padding_and_smoothing():
    a = _train3()
    assert all(l == l and abs(l) != float("inf") for l in a), a
    assert a[-1] < a[0], a
    assert _train3() == a
