"""Document masking inside the v3 flash attention kernels (their DOCS
instantiations): numerics against fp32 torch, tile skipping, dropout on
top, determinism, the gate in ``flash_attention`` and GPT-2 end to end.

Layouts, the smallest that reach each path:
  (a) (1,1,64)  [0,1) [1,17) [17,64): boundaries inside a wave's 16 rows
      and inside a 16-row sub-tile;
  (b) (2,3,128) row 0 [0,70) [70,128): rows 70..79 share a wave with rows
      64..69, which need tile 0, so tile 0 is fully masked for them (the
      m = -1e30 hazard the forward guards); row 1 [0,64) [64,128): a
      tile-aligned boundary, loop start 1, rows differ in one launch;
  (c) (1,2,256) [0,64) [64,65) [65,200) [200,256): odd loop starts with
      buffer alternation, per-wave skips in the last workgroup, the dkv
      early stop;
  (d) (1,1,128) [0,16) [16,100) [100,128): a dkv wave (kv 0..15) that
      stops before the other waves of its workgroup do.

Bounds are those of test_flash_attn_dropout_gpu.py: o 3e-2, lse 2e-2,
grads 5e-2, absolute and relative."""
import functools
import math

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
from ray_lightning_amd.ops.flash_attn import (doc_bounds,  # noqa: E402
                                              flash_attention)

HS = 64
SCALE = 1.0 / math.sqrt(HS)
BF16 = torch.bfloat16

LAYOUTS = {
    "a": (1, 1, 64, [[1, 16, 47]]),
    "b": (2, 3, 128, [[70, 58], [64, 64]]),
    "c": (1, 2, 256, [[64, 1, 135, 56]]),
    "d": (1, 1, 128, [[16, 84, 28]]),
}


@pytest.fixture(autouse=True)
def _custom_path(monkeypatch):
    monkeypatch.setenv("RLA_FLASH", "1")
    monkeypatch.setenv("RLA_FLASH_DOCS", "1")
    monkeypatch.setenv("RLA_FLASH_DROPOUT", "1")
    monkeypatch.delenv("RLA_FLASH_SHFL", raising=False)


def _ext():
    return _ops._load_ext()


def _ids(rows):
    """ids [B, T] of rows given as lists of document lengths; the ids
    alternate 7, 3, 7, ... so that an id comes back."""
    return torch.stack([
        torch.cat([torch.full((n,), 7 if i % 2 == 0 else 3)
                   for i, n in enumerate(row)]) for row in rows]).cuda()


def _allowed(rows):
    """[B, 1, T, T] bool, built from the lengths alone (not through
    doc_bounds): same document and kv <= q."""
    out = []
    for row in rows:
        T = sum(row)
        m = torch.zeros(T, T, dtype=torch.bool)
        s = 0
        for n in row:
            m[s:s + n, s:s + n] = True
            s += n
        out.append(torch.tril(m))
    return torch.stack(out)[:, None].cuda()


def _inputs(B, H, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.randn(B, H, T, HS, device="cuda", generator=g)
             * 0.5).to(BF16) for _ in range(4)]


def _ref(q, k, v, allowed, M=None, p=0.0):
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~allowed, float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if M is not None:
        pr = pr * M / (1.0 - p)
    return pr @ v, torch.logsumexp(s, dim=-1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, ids, and the fp32 reference (o, lse, dq, dk, dv) of a
    layout, computed once."""
    B, H, T, rows = LAYOUTS[name]
    q, k, v, dy = _inputs(B, H, T, 100 + T)
    allowed = _allowed(rows)
    q32, k32, v32 = (t.float().requires_grad_(True) for t in (q, k, v))
    o, lse = _ref(q32, k32, v32, allowed)
    o.backward(dy.float())
    ref = tuple(t.detach() for t in (o, lse, q32.grad, k32.grad, v32.grad))
    return q, k, v, dy, _ids(rows), allowed, ref


def _run(q, k, v, dy, ids, p=0.0):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(q, k, v, dropout_p=p, doc_ids=ids)
    lse = [t for t in o.grad_fn.saved_tensors
           if t.dim() == 3 and t.is_floating_point()][0]
    o.backward(dy)
    return o.detach(), lse, q.grad, k.grad, v.grad


def _close(name, got, want, atol, rtol):
    err = (got.float() - want).abs().max().item()
    print(f"{name}: max abs err {err:.3e}")
    assert torch.allclose(got.float(), want, atol=atol, rtol=rtol), \
        f"{name} max err {err}"


def _is_docs_fn(o):
    return o.grad_fn is not None and \
        o.grad_fn.name() == "_FlashAttnDocsBackward"


# --------------------------------------------------------- 1. numerics
@pytest.mark.parametrize("shfl", [False, True])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_numerics_against_fp32(name, shfl, monkeypatch):
    """Max abs errors measured on MI355X are recorded in
    profiles/flash_attn_docs.md."""
    if shfl:
        monkeypatch.setenv("RLA_FLASH_SHFL", "1")
    q, k, v, dy, ids, _allowed_, ref = _case(name)
    o, lse, dq, dk, dv = _run(q, k, v, dy, ids)
    _close("o", o, ref[0], 3e-2, 3e-2)
    _close("lse", lse, ref[1], 2e-2, 2e-2)
    _close("dq", dq, ref[2], 5e-2, 5e-2)
    _close("dk", dk, ref[3], 5e-2, 5e-2)
    _close("dv", dv, ref[4], 5e-2, 5e-2)


# --------------------------------- 2. one document is the plain kernel
@pytest.mark.parametrize("name", ["b", "c"])
def test_one_document_is_the_plain_kernel(name):
    q, k, v, dy, ids, _a, _r = _case(name)
    got = _run(q, k, v, dy, torch.full_like(ids, 5))
    q1, k1, v1 = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(q1, k1, v1)
    assert not _is_docs_fn(o)
    lse = [t for t in o.grad_fn.saved_tensors if t.dim() == 3][0]
    o.backward(dy)
    for n, a, b in zip(("o", "lse", "dq", "dk", "dv"), got,
                       (o.detach(), lse, q1.grad, k1.grad, v1.grad)):
        assert torch.equal(a, b), n


# --------------------------- 3. tiles are skipped, not just masked
# An MFMA multiplies whole 16 x 64 fragments, so a NaN row of K, V, dO or
# Q reaches every result of a wave that processes its TILE, masked or
# not (0 * NaN). The checks therefore put NaN on all rows of the other
# documents that lie in tiles the checked rows' waves must skip, and
# demand finite results equal to the clean run's. In layout (c) the
# last document [200,256) shares tile [192,256) with rows 192..199 of
# the document before it: those 8 rows cannot be NaN for any tiled
# kernel (rows 200..255 need that tile for themselves), so NaN covers
# [0,192), all three other documents but those rows; rows 200..207
# share their WAVE with 192..199, which walks tiles 64 and 128, and
# pass only because the forward zeroes such lanes by a select.
def _nan_rows(t, lo, hi):
    t = t.clone()
    t[:, :, lo:hi] = float("nan")
    return t


@pytest.mark.parametrize("use_permlane", [True, False])
@pytest.mark.parametrize("T,rows,nan_kv,check_q,nan_q,check_kv", [
    (128, [[64, 64]], (0, 64), (64, 128), (64, 128), (0, 64)),
    (256, [[64, 1, 135, 56]], (0, 192), (200, 256), (64, 256), (0, 64)),
], ids=["T128", "layout_c"])
def test_tiles_are_skipped(T, rows, nan_kv, check_q, nan_q, check_kv,
                           use_permlane):
    ext = _ext()
    B, H = 1, (1 if T == 128 else 2)
    q, k, v, dy = _inputs(B, H, T, 300 + T)
    start, end = doc_bounds(_ids(rows))
    o, lse = ext.flash_attn_fwd_v3_docs(q, k, v, start, SCALE, use_permlane)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    dq, dk, dv = ext.flash_attn_bwd_v3_docs(dy, q, k, v, o, lse, start, end,
                                            SCALE, use_permlane)

    # forward: K / V of the other documents are never multiplied
    o2, lse2 = ext.flash_attn_fwd_v3_docs(
        q, _nan_rows(k, *nan_kv), _nan_rows(v, *nan_kv), start, SCALE,
        use_permlane)
    sl = slice(*check_q)
    assert torch.isfinite(o2[:, :, sl]).all()
    assert torch.isfinite(lse2[:, :, sl]).all()
    assert torch.equal(o2[:, :, sl], o[:, :, sl])
    assert torch.equal(lse2[:, :, sl], lse[:, :, sl])
    # and the NaN did reach the rows that attend it
    assert torch.isnan(o2[:, :, nan_kv[0]:nan_kv[1]]).all()

    # backward: dO / Q of the later documents are never multiplied
    _dq, dk2, dv2 = ext.flash_attn_bwd_v3_docs(
        _nan_rows(dy, *nan_q), _nan_rows(q, *nan_q), k, v, o, lse, start,
        end, SCALE, use_permlane)
    sl = slice(*check_kv)
    assert torch.isfinite(dk2[:, :, sl]).all()
    assert torch.isfinite(dv2[:, :, sl]).all()
    assert torch.equal(dk2[:, :, sl], dk[:, :, sl])
    assert torch.equal(dv2[:, :, sl], dv[:, :, sl])
    assert torch.isnan(dv2[:, :, nan_q[0]:nan_q[1]]).all()


# ------------------------------------ 4. dropout and documents together
def _one_hot_block(B, H, T, c):
    x = torch.zeros(B, H, T, HS, device="cuda", dtype=BF16)
    x[:, :, 64 * c:64 * c + 64, :] = torch.eye(HS, device="cuda",
                                               dtype=BF16)
    return x


@pytest.mark.parametrize("use_permlane", [True, False])
def test_dropout_and_documents_together(use_permlane, monkeypatch):
    """With q = k = 0, P is uniform over the allowed run of each row; a
    one-hot V block reads the kept columns off o, a one-hot dO block
    reads them off dV."""
    if not use_permlane:
        monkeypatch.setenv("RLA_FLASH_SHFL", "1")
    ext = _ext()
    B, H, T, rows = LAYOUTS["b"]
    p, seed = 0.5, 228
    q, k, v, dy, ids, allowed, _r = _case("b")
    start, end = doc_bounds(ids)
    want = torch.from_numpy(
        keep_mask(seed, 0, B * H * T * T, p).reshape(B, H, T, T)
    ).cuda() & allowed
    z = torch.zeros(B, H, T, HS, device="cuda", dtype=BF16)
    run = (torch.arange(T, device="cuda")[None] - start + 1).float()
    lse0 = torch.log(run)[:, None].expand(B, H, T).contiguous()
    fwd = torch.zeros(B, H, T, T, device="cuda", dtype=torch.bool)
    dkv = torch.zeros_like(fwd)
    for c in range(T // 64):
        blk = _one_hot_block(B, H, T, c)
        torch.manual_seed(seed)
        o, _lse, s, off = ext.flash_attn_fwd_v3_docs_dropout(
            z, z, blk, start, SCALE, p, use_permlane)
        assert (s, off) == (seed, 0)
        fwd[..., 64 * c:64 * c + 64] = o != 0
        _dq, _dk, dv = ext.flash_attn_bwd_v3_docs_dropout(
            blk, z, z, z, z, lse0, start, end, SCALE, p, seed, 0,
            use_permlane)
        dkv[:, :, 64 * c:64 * c + 64, :] = (dv != 0).transpose(-1, -2)
    assert torch.equal(fwd, want), "forward mask"
    assert torch.equal(dkv, want), "dkv mask"

    # numerics given that mask
    torch.manual_seed(seed)
    o, lse, dq, dk, dv = _run(q, k, v, dy, ids, p=p)
    q32, k32, v32 = (t.float().requires_grad_(True) for t in (q, k, v))
    ref, lse_ref = _ref(q32, k32, v32, allowed, want.float(), p)
    ref.backward(dy.float())
    s = 1.0 / (1.0 - p)
    _close("o", o, ref.detach(), 3e-2 * s, 3e-2)
    _close("lse", lse, lse_ref.detach(), 2e-2, 2e-2)
    _close("dq", dq, q32.grad, 5e-2 * s, 5e-2)
    _close("dk", dk, k32.grad, 5e-2 * s, 5e-2)
    _close("dv", dv, v32.grad, 5e-2 * s, 5e-2)


# ------------------------------------------------------ 5. determinism
def test_run_to_run_determinism():
    q, k, v, dy, ids, _a, _r = _case("c")
    first = _run(q, k, v, dy, ids)
    again = _run(q, k, v, dy, ids)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


# ------------------------------------------------------------- 6. gate
def test_gate_usable_call_takes_the_docs_kernels():
    q, k, v, _dy, ids, _a, _r = _case("b")
    q = q.clone().requires_grad_(True)
    assert _is_docs_fn(flash_attention(q, k, v, doc_ids=ids))
    assert _is_docs_fn(flash_attention(q, k, v, doc_ids=doc_bounds(ids)))
    assert _is_docs_fn(flash_attention(q, k, v, dropout_p=0.1,
                                       doc_ids=ids))
    assert not _is_docs_fn(flash_attention(q, k, v))
    assert not _is_docs_fn(flash_attention(q, k, v, doc_ids=None))


def test_gate_default_is_what_the_module_records(monkeypatch):
    monkeypatch.delenv("RLA_FLASH_DOCS")
    q, k, v, _dy, ids, _a, _r = _case("b")
    q = q.clone().requires_grad_(True)
    assert _is_docs_fn(flash_attention(q, k, v, doc_ids=ids)) == \
        fa._DOCS_DEFAULT


@pytest.mark.parametrize("case", ["RLA_FLASH_DOCS=0", "T32", "fp32",
                                  "RLA_FLASH=0"])
def test_gate_fallbacks_still_mask(case, monkeypatch):
    T, dtype, rows = 64, BF16, [[1, 16, 47], [40, 24]]
    if case == "T32":
        T, rows = 32, [[10, 22], [1, 31]]
    elif case == "fp32":
        dtype = torch.float32
    else:
        name, val = case.split("=")
        monkeypatch.setenv(name, val)
    g = torch.Generator(device="cuda").manual_seed(4)
    q, k, v = ((torch.randn(2, 2, T, HS, device="cuda", generator=g)
                * 0.5).to(dtype) for _ in range(3))
    q.requires_grad_(True)
    o = flash_attention(q, k, v, doc_ids=_ids(rows))
    assert not _is_docs_fn(o)
    assert not torch.allclose(o, flash_attention(q, k, v), atol=3e-2,
                              rtol=3e-2)
    ref, _ = _ref(q.detach().float(), k.float(), v.float(), _allowed(rows))
    _close("o", o.detach(), ref, 3e-2, 3e-2)


def test_saved_tensors():
    B, H, T, _rows = LAYOUTS["b"]
    q, k, v, _dy, ids, _a, _r = _case("b")
    q = q.clone().requires_grad_(True)
    for p in (0.0, 0.1):
        o = flash_attention(q, k, v, dropout_p=p, doc_ids=ids)
        n = B * H * T
        assert sorted(t.numel() for t in o.grad_fn.saved_tensors) == \
            sorted([n * HS] * 4 + [n] + [B * T] * 2)


# ------------------------------------- 7. entry points check operands
def test_ext_entry_points_check_the_bounds():
    ext = _ext()
    B, H, T = 2, 1, 64
    q, k, v, dy = _inputs(B, H, T, 8)
    start, end = doc_bounds(_ids([[1, 16, 47], [40, 24]]))
    o, lse = ext.flash_attn_fwd_v3_docs(q, k, v, start, SCALE, True)
    ext.flash_attn_bwd_v3_docs(dy, q, k, v, o, lse, start, end, SCALE, True)
    o2, lse2, seed, off = ext.flash_attn_fwd_v3_docs_dropout(
        q, k, v, start, SCALE, 0.1, True)
    ext.flash_attn_bwd_v3_docs_dropout(dy, q, k, v, o2, lse2, start, end,
                                       SCALE, 0.1, seed, off, True)

    def bads(t):
        strided = torch.stack([t, t], dim=-1)[..., 0]
        assert not strided.is_contiguous()
        return [t.long(), t.float(), t[:, :32].contiguous(), t[:1],
                torch.cat([t, t]), t.reshape(-1), t.cpu(), strided]

    for bad in bads(start):
        with pytest.raises(RuntimeError):
            ext.flash_attn_fwd_v3_docs(q, k, v, bad, SCALE, True)
        with pytest.raises(RuntimeError):
            ext.flash_attn_fwd_v3_docs_dropout(q, k, v, bad, SCALE, 0.1,
                                               True)
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_v3_docs(dy, q, k, v, o, lse, bad, end,
                                       SCALE, True)
    for bad in bads(end):
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_v3_docs(dy, q, k, v, o, lse, start, bad,
                                       SCALE, True)
        with pytest.raises(RuntimeError):
            ext.flash_attn_bwd_v3_docs_dropout(dy, q, k, v, o2, lse2, start,
                                               bad, SCALE, 0.1, seed, off,
                                               True)
    # the other operands go through the checks of the plain entry points
    with pytest.raises(RuntimeError):
        ext.flash_attn_fwd_v3_docs(q, k, v.float(), start, SCALE, True)
    with pytest.raises(RuntimeError):
        ext.flash_attn_bwd_v3_docs(dy[:, :, :32], q, k, v, o, lse, start,
                                   end, SCALE, True)


# ------------------------------------------------------------ 8. GPT-2
def test_gpt2_end_to_end(monkeypatch):
    from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                               to_bf16_training)
    calls = []
    real = fa._FlashAttnDocs.apply
    monkeypatch.setattr(fa._FlashAttnDocs, "apply",
                        lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(2)
    cfg = GPT2Config(vocab_size=503, n_positions=128, n_embd=256,
                     n_layer=2, n_head=4)
    model = to_bf16_training(GPT2(cfg).cuda())
    rows = [[70, 58], [70, 58]]
    ids = _ids(rows)
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = torch.randint(0, 503, (2, 128), device="cuda", generator=g)
    tgt = torch.randint(0, 503, (2, 128), device="cuda", generator=g)

    model.train()
    _, loss = model(idx, tgt, doc_ids=ids)
    assert len(calls) == 2       # every layer took the DOCS kernels
    loss.backward()
    assert torch.isfinite(loss)
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name

    model.eval()
    with torch.no_grad():
        packed = model(idx, doc_ids=ids)[0]
        assert len(calls) == 4
        for s, n in ((0, 70), (70, 58)):
            alone = model(idx[:, s:s + n])[0]     # T = 70 / 58: SDPA
            _close(f"logits[{s}:{s + n}]", packed[:, s:s + n],
                   alone.float(), 3e-2, 3e-2)
        assert len(calls) == 4
        assert not torch.allclose(packed[:, 70:], model(idx)[0][:, 70:],
                                  atol=3e-2, rtol=3e-2)
