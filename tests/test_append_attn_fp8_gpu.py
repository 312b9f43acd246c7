"""The fp8-cache variant of the MFMA append kernel (csrc/append_attn.hip) on
MI355X: against fp64 attention over the dequantized cache as the call leaves
it, and bit for bit against ``quantize_kv``. The torch composition ``_fp8``
is taken away, so every call here that passes ran the kernel."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import append_attn as aa  # noqa: E402
from ray_lightning_amd.ops import decode_attn as da  # noqa: E402
from skinny_common import tiny_models  # noqa: E402

EXT = _ops._load_ext()
C = aa.append_attn_chunk()
HS, BF16, FP8, DEV = 64, torch.bfloat16, torch.float8_e4m3fn, "cuda"
TMAX = 3 * C
SCALE = 1.0 / math.sqrt(HS)
# the project's attention bound (tests/test_decode_attn_gpu.py)
ATOL = RTOL = 3e-2
_FP8 = aa._fp8


@pytest.fixture(autouse=True)
def _kernel_on(monkeypatch):
    monkeypatch.setenv("RLA_APPEND_ATTN", "1")
    monkeypatch.setattr(aa, "_fp8", None)  # a call of the composition fails


def _case(B, H, T, pos_list, seed=0):
    """Binade spread per position; NaN code and scale from pos[b] on."""
    g = torch.Generator().manual_seed(seed)
    spread = lambda *s: torch.randn(*s, HS, generator=g) * torch.exp2(
        torch.randint(-3, 4, (*s, 1), generator=g).float())
    out = [spread(B, T, 3 * H).view(B, T, -1).to(DEV, BF16)]
    for _ in range(2):
        codes, scale = da.quantize_kv(spread(B, H, TMAX).to(DEV, BF16))
        for b, p in enumerate(pos_list):
            codes.view(torch.uint8)[b, :, max(p, 0):] = 0x7F
            scale[b, :, max(p, 0):] = math.nan
        out += [codes, scale]
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    return out[0], out[1], out[3], out[2], out[4], pos


def _check(case, live, max_pos, name):
    """``live[b]``: row b's pos, or None for a row that must not move."""
    qkv, k, v, ks, vs, pos = case
    B, T = qkv.shape[:2]
    H = k.shape[1]
    before = [t.clone() for t in (k, v, ks, vs)]
    o = aa.append_attention(qkv, k, v, pos, max_pos, k_scale=ks, v_scale=vs)
    assert o.dtype == BF16 and o.shape == (B, T, H * HS)
    # slots pos .. pos+T-1 hold quantize_kv of the new rows; nothing else moved
    new = qkv.view(B, T, 3, H, HS)
    for cache, scale, c0, s0, part in ((k, ks, before[0], before[2], 1),
                                       (v, vs, before[1], before[3], 2)):
        want_c, want_s = c0.view(torch.uint8).clone(), s0.clone()
        codes, s = da.quantize_kv(new[:, :, part].transpose(1, 2))
        for b, p in enumerate(live):
            if p is not None:
                want_c[b, :, p:p + T] = codes[b].view(torch.uint8)
                want_s[b, :, p:p + T] = s[b]
        assert torch.equal(cache.view(torch.uint8), want_c), name
        assert torch.equal(scale.view(torch.int32), want_s.view(torch.int32))
    # fp64 attention over the dequantized cache as the call left it
    q = new[:, :, 0].transpose(1, 2).double()              # [B, H, T, HS]
    ref = torch.zeros(B, T, H, HS, dtype=torch.float64, device=DEV)
    steps = torch.arange(TMAX, device=DEV)
    for b, p in enumerate(live):
        if p is not None:
            n = p + T
            keys = k[b, :, :n].double() * ks[b, :, :n, None].double()
            vals = v[b, :, :n].double() * vs[b, :, :n, None].double()
            s = torch.einsum("htd,hsd->hts", q[b], keys) * SCALE
            s = s.masked_fill(steps[None, :n] > p + steps[:T, None], -math.inf)
            ref[b] = (torch.softmax(s, dim=-1) @ vals).transpose(0, 1)
    got = o.double().view(B, T, H, HS)
    print(f"{name}: max abs err {(got - ref).abs().max().item():.3e}")
    assert torch.allclose(got, ref, atol=ATOL, rtol=RTOL), name
    return o


@pytest.mark.parametrize("T,p", [(T, p) for T in (1, 16, 17, 33)
                                 for p in (0, 1, C - 1, C, 2 * C - T // 2)])
def test_against_fp64(T, p):
    """New rows across a chunk edge, a tile edge inside them, no history."""
    _check(_case(1, 1, T, [p], seed=T + p), [p], p, f"T{T}p{p}")


def _ragged(name):
    pos_list, T, mp = [0, C + 1, 2 * C + 5], 33, 2 * C + 5
    case = _case(3, 2, T, pos_list, seed=3)
    copies = [[t.clone() for t in case] for _ in range(2)]
    return pos_list, mp, copies, _check(case, pos_list, mp, name)


def test_ragged_same_bits_twice_and_alone():
    pos_list, mp, (again, alone), o = _ragged("ragged")
    qkv, k, v, ks, vs, pos = again
    o2 = aa.append_attention(qkv, k, v, pos, mp, k_scale=ks, v_scale=vs)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16))
    for b, p in enumerate(pos_list):
        qkv, k, v, ks, vs, pos = (t[b:b + 1].contiguous() for t in alone)
        ob = aa.append_attention(qkv, k, v, pos, p, k_scale=ks, v_scale=vs)
        assert torch.equal(ob.view(torch.int16),
                           o[b:b + 1].view(torch.int16)), f"row {b}"


@pytest.mark.parametrize("bad,max_pos", [(-1, C), (C + 9, C)])
def test_inactive_row(bad, max_pos):
    """Nothing of the row moves, scales included; its output is zero."""
    case = _case(3, 2, 17, [5, bad, C - 3], seed=1)
    o = _check(case, [5, None, C - 3], max_pos, "inactive")
    assert not o[1].any()


@pytest.mark.parametrize("exp", [-3, 0, 5])
def test_every_e4m3_code_dequantizes_exactly(exp):
    """Slot 0 (cached-row path) and both new rows (new-row path) carry the
    same dequantized codes; q = 0, pos = 1: (t + 2) * v / (t + 2) = v."""
    code = torch.arange(256, dtype=torch.uint8)
    code[(code & 0x7F) == 0x7F] = 0
    v8 = code.view(1, 4, 1, HS).to(DEV).view(FP8)
    vs = torch.full((1, 4, 1), 2.0 ** exp, device=DEV)
    row = da.dequantize_kv(v8, vs)[:, :, 0]                     # [1, 4, 64] bf16
    assert torch.equal(da.dequantize_kv(*da.quantize_kv(row)), row)
    H, T = 4, 2
    k = torch.zeros(1, H, C, HS, dtype=torch.uint8, device=DEV).view(FP8)
    v = k.clone()
    v.view(torch.uint8)[:, :, :1] = v8.view(torch.uint8)
    ks = torch.ones(1, H, C, device=DEV)
    vsc = ks.clone()
    vsc[:, :, :1] = vs
    qkv = torch.zeros(1, T, 3, H, HS, dtype=BF16, device=DEV)
    qkv[:, :, 2] = row
    pos = torch.ones(1, dtype=torch.int32, device=DEV)
    o = aa.append_attention(qkv.view(1, T, -1), k, v, pos, 1, k_scale=ks,
                            v_scale=vsc)
    # a code of -0 adds to the accumulator's +0
    want = (row.float() + 0.0).to(BF16).view(1, 1, -1).expand(1, T, -1)
    assert torch.equal(o.view(torch.int16), want.contiguous().view(torch.int16))


def test_gate_off_runs_the_composition(monkeypatch):
    monkeypatch.setenv("RLA_APPEND_ATTN", "0")
    called = []
    monkeypatch.setattr(aa, "_fp8", lambda *a: (called.append(1), _FP8(*a))[1])
    _ragged("composition")
    assert called


def test_operand_checks_raise_before_any_launch():
    qkv, k, v, ks, vs, pos = _case(2, 2, 4, [3, 5])
    before = [t.clone() for t in (k, v, ks, vs)]
    kb = torch.zeros(2, 2, TMAX, HS, dtype=BF16, device=DEV)
    # scales without fp8 caches, one scale only, scale shape, scale dtype
    bad = [(kb, kb.clone(), ks, vs), (k, v, ks, None),
           (k, v, ks[:, :, :C].contiguous(), vs), (k, v, ks, vs.to(BF16))]
    for a, b, c, d in bad:
        with pytest.raises(RuntimeError):
            EXT.append_attn_fwd(qkv, a, b, pos, 5, SCALE, c, d)
    torch.cuda.synchronize()
    for t, t0 in zip((k, v, ks, vs), before):
        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8))


def test_generate_kernel_against_composition(monkeypatch):
    """A chunked prefill's logit error against fp32, e_kernel <= 2 * e_twin
    (tests/test_kv_fp8_gpu.py). A drafted run returns no logits: its tokens
    are the fp32 argmax where the margin exceeds 4 * e_twin
    (tests/test_spec_decode_gpu.py)."""
    m16, m32 = tiny_models(256, DEV)
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (3, 12), generator=g)
    idx[2] = torch.tensor([7, 8, 9] * 4)
    idx, lens, new = idx.to(DEV), [5, 1, 12], 32

    def refs(out):
        with torch.no_grad():
            return [m32(out[b, :n + new][None])[0][0, n - 1:n - 1 + new].float()
                    for b, n in enumerate(lens)]

    def chunked():
        out, logits = m16.generate(idx, new, prompt_lens=lens, kv_fp8=True,
                                   temperature=0.0, return_logits=True,
                                   prefill_chunk=4)
        return max((logits[b] - r).abs().max().item()
                   for b, r in enumerate(refs(out)))

    e_kernel = chunked()
    out = m16.generate(idx, new, prompt_lens=lens, kv_fp8=True,
                       temperature=0.0, draft_tokens=3, seed=1)
    monkeypatch.setenv("RLA_APPEND_ATTN", "0")
    monkeypatch.setattr(aa, "_fp8", _FP8)
    e_twin = chunked()
    print(f"e_kernel {e_kernel:.3e}  e_twin {e_twin:.3e}")
    assert e_kernel <= 2 * e_twin
    for b, ref in enumerate(refs(out)):
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4 * e_twin
        tok = out[b, lens[b]:lens[b] + new]
        assert torch.equal(tok[clear], ref.argmax(dim=-1)[clear])
