"""MFMA split-KV append attention kernel (csrc/append_attn.hip) on
MI355X: numerics against fp32 torch from the same bf16 inputs, the
in-launch append of T rows, inactive rows, bitwise repeatability and
independence of the batch, and the operand checks of the host path."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops.append_attn import append_attention  # noqa: E402

EXT = _ops._load_ext()
C = int(EXT.append_attn_chunk())
HS = 64
SCALE = 1.0 / math.sqrt(HS)
BF16 = torch.bfloat16
DEV = "cuda"
TMAX = 3 * C
# the bound tests/test_decode_attn_gpu.py holds for this quantity
ATOL = RTOL = 3e-2


@pytest.fixture(autouse=True)
def _kernel_on(monkeypatch):
    monkeypatch.setenv("RLA_APPEND_ATTN", "1")


def _case(B, H, T, pos_list, seed=0):
    """bf16 operands with NaN in every cache slot >= pos[b] of a row with
    pos[b] >= 0."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * HS, generator=g).to(DEV, BF16)
    kc = torch.randn(B, H, TMAX, HS, generator=g).to(DEV, BF16)
    vc = torch.randn(B, H, TMAX, HS, generator=g).to(DEV, BF16)
    for b, p in enumerate(pos_list):
        if p >= 0:
            kc[b, :, p:] = math.nan
            vc[b, :, p:] = math.nan
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    return qkv, kc, vc, pos


def _check(qkv, kc, vc, pos, live, max_pos, name):
    """``live[b]`` is row b's pos, or None for a row that must stay as it
    is and return zeros."""
    B, T = qkv.shape[:2]
    H = kc.shape[1]
    kc0, vc0 = kc.clone(), vc.clone()
    o = append_attention(qkv, kc, vc, pos, max_pos=max_pos)
    assert o.dtype == BF16 and o.shape == (B, T, H * HS)
    q, k, v = (x.transpose(1, 2)                           # [B, H, T, HS]
               for x in qkv.view(B, T, 3, H, HS).unbind(2))
    slots = torch.arange(TMAX, device=DEV)
    for b, p in enumerate(live):
        got = o[b].float().view(T, H, HS).transpose(0, 1)
        want = torch.zeros(TMAX, dtype=torch.bool, device=DEV)
        if p is None:
            assert not got.any()
        else:
            keys = torch.cat([kc0[b, :, :p], k[b]], dim=1).float()
            vals = torch.cat([vc0[b, :, :p], v[b]], dim=1).float()
            s = torch.einsum("htd,hsd->hts", q[b].float(), keys) * SCALE
            s = s.masked_fill(
                slots[None, :p + T] > p + slots[:T, None], -math.inf)
            ref = torch.softmax(s, dim=-1) @ vals
            err = (got - ref).abs().max().item()
            print(f"{name} row {b}: max abs err {err:.3e}")
            assert torch.allclose(got, ref, atol=ATOL, rtol=RTOL), \
                f"{name} row {b} max err {err}"
            want[p:p + T] = True
            for cache, new in ((kc, k), (vc, v)):
                assert torch.equal(cache[b, :, p:p + T].view(torch.int16),
                                   new[b].contiguous().view(torch.int16))
        for cache, before in ((kc, kc0), (vc, vc0)):
            same = (cache[b].view(torch.int16) ==
                    before[b].view(torch.int16)).all(dim=2).all(dim=0)
            assert same[~want].all(), f"{name} row {b}: a slot moved"
    return o


def _pos_sets(T):
    edge = [0, 1, C - 1, C, C + 1, 2 * C - T // 2]
    return [(1, 1, [p]) for p in edge] + \
        [(3, 2, [0, C + 1, 2 * C - T // 2]), (3, 2, [C, 1, C - 1])]


CASES = [(B, H, T, pl) for T in (1, 2, 15, 16, 17, 33, 65)
         for B, H, pl in _pos_sets(T)]


@pytest.mark.parametrize(
    "B,H,T,pos_list", CASES,
    ids=[f"B{B}H{H}T{T}p{'_'.join(map(str, pl))}" for B, H, T, pl in CASES])
def test_against_fp32(B, H, T, pos_list):
    """pos = C-1 and 2C - T/2 put the new rows across a chunk boundary,
    T > 16 a query tile boundary inside them."""
    qkv, kc, vc, pos = _case(B, H, T, pos_list, seed=T)
    _check(qkv, kc, vc, pos, pos_list, max(pos_list), "fp32")


@pytest.mark.parametrize("bad,max_pos", [(-1, C), (C + 9, C)])
def test_inactive_row(bad, max_pos):
    """pos = -1, and pos > max_pos (in a cache large enough to hold the
    row anyway): nothing of the row moves, its output is zero."""
    pos_list = [5, bad, C - 3]
    qkv, kc, vc, pos = _case(3, 2, 17, pos_list, seed=1)
    _check(qkv, kc, vc, pos, [5, None, C - 3], max_pos, "inactive")


def test_same_bits_alone_in_a_batch_and_twice():
    T, pos_list = 33, [1, C - 7, 2 * C + 5]
    qkv, kc, vc, pos = _case(3, 2, T, pos_list, seed=3)
    kc0, vc0 = kc.clone(), vc.clone()
    o = _check(qkv, kc, vc, pos, pos_list, 2 * C + 5, "batch")
    kc2, vc2 = kc0.clone(), vc0.clone()
    o2 = append_attention(qkv, kc2, vc2, pos, max_pos=2 * C + 5)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16))
    assert torch.equal(kc2.view(torch.int16), kc.view(torch.int16))
    for b, p in enumerate(pos_list):
        alone = append_attention(
            qkv[b:b + 1].contiguous(), kc0[b:b + 1].clone(),
            vc0[b:b + 1].clone(), pos[b:b + 1].contiguous(), max_pos=p)
        assert torch.equal(alone.view(torch.int16),
                           o[b:b + 1].view(torch.int16)), f"row {b}"


def test_operand_checks_raise_before_any_launch():
    B, H, T = 2, 2, 4
    qkv, kc, vc, pos = _case(B, H, T, [3, 5])
    kc0, vc0 = kc.clone(), vc.clone()
    wide = torch.zeros(B, H, TMAX, 2 * HS, dtype=BF16, device=DEV)
    bad = [
        ("fp16 qkv", (qkv.to(torch.float16), kc, vc, pos, 5)),
        ("non-contiguous cache", (qkv, wide[..., ::2], vc, pos, 5)),
        ("max_pos + T > Tmax", (qkv, kc, vc, pos, TMAX - T + 1)),
        ("negative max_pos", (qkv, kc, vc, pos, -1)),
        ("int64 pos", (qkv, kc, vc, pos.long(), 5)),
        ("2-d qkv", (qkv[:, 0].contiguous(), kc, vc, pos, 5)),
        ("cache shapes differ", (qkv, kc, vc[:, :, :C].contiguous(), pos, 5)),
    ]
    for name, (a, b, c, d, mp) in bad:
        with pytest.raises(RuntimeError):
            EXT.append_attn_fwd(a, b, c, d, mp, SCALE)
        print("raised:", name)
    torch.cuda.synchronize()
    assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vc0.view(torch.int16))
