"""Split-KV decode attention kernel (csrc/decode_attn.hip) on MI355X:
numerics against fp32 torch from the same bf16 inputs, the in-launch
append, bitwise repeatability and independence of the batch, the env
gate, and the operand checks of the host path.

Out-of-range device ``pos`` values are not run on the GPU: the twin's
CPU test covers that contract and the kernel's guard is read, not
provoked."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

# the custom path must be the one under test — fail loudly if the HIP
# extension did not load on a GPU box (no silent eager fallback)
from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import decode_attn as da  # noqa: E402
from ray_lightning_amd.ops.decode_attn import decode_attention  # noqa: E402

EXT = _ops._load_ext()
C = int(EXT.decode_attn_chunk())
HS = 64
SCALE = 1.0 / math.sqrt(HS)
BF16 = torch.bfloat16
DEV = "cuda"
# the project's bound for attention outputs against fp32
# (tests/test_flash_attn_dropout_gpu.py)
ATOL = RTOL = 3e-2


def _case(B, H, Tmax, pos_list, seed=0):
    """bf16 operands with NaN in every cache slot >= pos[b]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, 3 * H * HS, generator=g).to(DEV, BF16)
    kc = torch.randn(B, H, Tmax, HS, generator=g).to(DEV, BF16)
    vc = torch.randn(B, H, Tmax, HS, generator=g).to(DEV, BF16)
    for b, p in enumerate(pos_list):
        kc[b, :, p:] = math.nan
        vc[b, :, p:] = math.nan
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    return qkv, kc, vc, pos


def _reference(qkv, kc, vc, pos_list):
    """fp32 softmax attention from the same bf16 values."""
    B, H, Tmax, _ = kc.shape
    q, k, v = qkv.float().view(B, 3, H, HS).unbind(1)
    out = torch.zeros(B, H, HS, device=qkv.device)
    for b, p in enumerate(pos_list):
        keys = torch.cat([kc[b, :, :p].float(), k[b][:, None]], dim=1)
        vals = torch.cat([vc[b, :, :p].float(), v[b][:, None]], dim=1)
        s = torch.einsum("hd,htd->ht", q[b], keys) * SCALE
        out[b] = torch.einsum("ht,htd->hd", torch.softmax(s, dim=-1), vals)
    return out.reshape(B, H * HS)


def _check(qkv, kc, vc, pos, pos_list, max_pos, name):
    kc0, vc0 = kc.clone(), vc.clone()
    ref = _reference(qkv, kc0, vc0, pos_list)
    o = decode_attention(qkv, kc, vc, pos, max_pos=max_pos)
    assert o.dtype == BF16 and o.shape == ref.shape
    assert torch.isfinite(o).all()
    err = (o.float() - ref).abs().max().item()
    print(f"{name}: max abs err {err:.3e}")
    assert torch.allclose(o.float(), ref, atol=ATOL, rtol=RTOL), \
        f"{name} max err {err}"
    # the caches change at slot pos[b] only, to the k / v parts of qkv
    B, H, Tmax, _ = kc.shape
    new = qkv.view(B, 3, H, HS)
    for cache, before, part in ((kc, kc0, 1), (vc, vc0, 2)):
        changed = (cache.view(torch.int16) != before.view(torch.int16)) \
            .any(dim=3).any(dim=1)
        want = torch.zeros(B, Tmax, dtype=torch.bool, device=DEV)
        for b, p in enumerate(pos_list):
            want[b, p] = True
            assert torch.equal(
                cache[b, :, p].view(torch.int16),
                new[b, part].contiguous().view(torch.int16))
        assert torch.equal(changed, want)
    return o


@pytest.fixture(autouse=True)
def _kernel_on(monkeypatch):
    monkeypatch.setenv("RLA_DECODE_ATTN", "1")


SINGLE = [(C, 0), (C, 1), (C, C - 1),
          (2 * C, C - 1), (2 * C, C), (2 * C, C + 1)]


@pytest.mark.parametrize("Tmax,p", SINGLE,
                         ids=[f"T{t}p{p}" for t, p in SINGLE])
def test_one_row_at_the_chunk_edges(Tmax, p):
    """One key taken from qkv alone; the last slot of a chunk; the new
    token first or last in a chunk; a chunk that holds only it."""
    qkv, kc, vc, pos = _case(1, 1, Tmax, [p], seed=p)
    _check(qkv, kc, vc, pos, [p], None, f"B1H1T{Tmax}p{p}")


def test_ragged_rows_and_batch_independence():
    """Rows of different lengths in one launch, some with empty chunks;
    every row computed alone (B = 1, its own max_pos) has the bits it
    has inside the batch."""
    pos_list = [0, C + 37, 4 * C - 1]
    qkv, kc, vc, pos = _case(3, 2, 4 * C, pos_list, seed=3)
    kc0, vc0 = kc.clone(), vc.clone()
    o = _check(qkv, kc, vc, pos, pos_list, 4 * C - 1, "ragged")
    # the same call twice: the same bits
    kc2, vc2 = kc0.clone(), vc0.clone()
    o2 = decode_attention(qkv, kc2, vc2, pos, max_pos=4 * C - 1)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16))
    assert torch.equal(kc2.view(torch.int16), kc.view(torch.int16))
    for b, p in enumerate(pos_list):
        alone = decode_attention(
            qkv[b:b + 1].contiguous(), kc0[b:b + 1].clone(),
            vc0[b:b + 1].clone(), pos[b:b + 1].contiguous(), max_pos=p)
        assert torch.equal(alone.view(torch.int16),
                           o[b:b + 1].view(torch.int16)), f"row {b}"


def test_gpt2_xl_heads_and_length():
    pos_list = [1023, 517]
    qkv, kc, vc, pos = _case(2, 25, 1024, pos_list, seed=5)
    _check(qkv, kc, vc, pos, pos_list, 1023, "B2H25T1024")


def test_gate_off_runs_the_twin(monkeypatch):
    pos_list = [0, C + 37, 4 * C - 1]
    qkv, kc, vc, pos = _case(3, 2, 4 * C, pos_list, seed=3)
    monkeypatch.setenv("RLA_DECODE_ATTN", "0")
    called = []
    monkeypatch.setattr(da, "_twin", lambda *a, _f=da._twin:
                        (called.append(1), _f(*a))[1])
    _check(qkv, kc, vc, pos, pos_list, 4 * C - 1, "twin")
    assert called


def test_operand_checks_raise_before_any_launch():
    B, H, Tmax = 2, 2, 2 * C
    qkv, kc, vc, pos = _case(B, H, Tmax, [3, 5])
    kc0, vc0 = kc.clone(), vc.clone()
    wide = torch.zeros(B, H, Tmax, 2 * HS, dtype=BF16, device=DEV)
    bad = [
        ("fp16 qkv", (qkv.to(torch.float16), kc, vc, pos, Tmax - 1)),
        ("non-contiguous cache", (qkv, wide[..., ::2], vc, pos, Tmax - 1)),
        ("int64 pos", (qkv, kc, vc, pos.long(), Tmax - 1)),
        ("pos on the CPU", (qkv, kc, vc, pos.cpu(), Tmax - 1)),
        ("max_pos = Tmax", (qkv, kc, vc, pos, Tmax)),
        ("negative max_pos", (qkv, kc, vc, pos, -1)),
        ("B mismatch", (qkv[:1].contiguous(), kc, vc, pos[:1].contiguous(),
                        Tmax - 1)),
        ("H mismatch", (qkv[:, :3 * HS].contiguous(), kc, vc, pos,
                        Tmax - 1)),
        ("cache shapes differ", (qkv, kc, vc[:, :, :C].contiguous(), pos,
                                 Tmax - 1)),
    ]
    for name, (a, b, c, d, mp) in bad:
        with pytest.raises(RuntimeError):
            EXT.decode_attn_fwd(a, b, c, d, mp, SCALE)
        print("raised:", name)
    torch.cuda.synchronize()
    # nothing was launched: the caches still hold their bits
    assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vc0.view(torch.int16))
