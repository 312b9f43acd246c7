"""The fp8 KV cache kernels (csrc/decode_attn.hip) on MI355X against fp64
attention over the dequantized cache as the call leaves it, and bit for
bit against ``quantize_kv``. Out-of-range device ``pos`` is not run on the
GPU: the twin's CPU test covers that contract."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from ray_lightning_amd import ops as _ops
assert _ops._load_ext() is not None, "HIP extension failed to load"

from ray_lightning_amd.ops import decode_attn as da  # noqa: E402
from ray_lightning_amd.ops import skinny_linear as sl  # noqa: E402
from skinny_common import tiny_models  # noqa: E402

EXT = _ops._load_ext()
C = int(EXT.decode_attn_chunk())
HS, BF16, FP8, DEV = 64, torch.bfloat16, torch.float8_e4m3fn, "cuda"
SCALE = 1.0 / math.sqrt(HS)
# the project's attention bound (tests/test_decode_attn_gpu.py)
ATOL = RTOL = 3e-2
_TWIN = da._twin


@pytest.fixture(autouse=True)
def _kernel_on(monkeypatch):
    monkeypatch.setenv("RLA_DECODE_ATTN", "1")
    monkeypatch.setattr(da, "_twin", None)  # a call of the twin fails


def _case(B, H, Tmax, pos_list, seed=0):
    """Quantized random caches, NaN code and NaN scale from pos[b] on."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * H * HS, generator=g).to(DEV, BF16)
    out = [qkv]
    for _ in range(2):
        x = torch.randn(B, H, Tmax, HS, generator=g) * torch.exp2(
            torch.randint(-3, 4, (B, H, Tmax, 1), generator=g).float())
        codes, scale = da.quantize_kv(x.to(DEV, BF16))
        for b, p in enumerate(pos_list):
            codes.view(torch.uint8)[b, :, p:] = 0x7F
            scale[b, :, p:] = math.nan
        out += [codes, scale]
    pos = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    return out[0], out[1], out[3], out[2], out[4], pos


def _reference(qkv, k, v, ks, vs, pos_list):
    """fp64 attention over the dequantized slots 0 .. pos[b]."""
    B, H = k.shape[:2]
    q = qkv.double().view(B, 3, H, HS)[:, 0]
    out = torch.zeros(B, H, HS, dtype=torch.float64, device=DEV)
    for b, p in enumerate(pos_list):
        keys = k[b, :, :p + 1].double() * ks[b, :, :p + 1, None].double()
        vals = v[b, :, :p + 1].double() * vs[b, :, :p + 1, None].double()
        s = torch.einsum("hd,htd->ht", q[b], keys) * SCALE
        out[b] = torch.einsum("ht,htd->hd", torch.softmax(s, dim=-1), vals)
    return out.reshape(B, H * HS)


def _check(case, pos_list, max_pos, name):
    qkv, k, v, ks, vs, pos = case
    before = [t.clone() for t in (k, v, ks, vs)]
    o = da.decode_attention(qkv, k, v, pos, max_pos, k_scale=ks, v_scale=vs)
    ref = _reference(qkv, k, v, ks, vs, pos_list)
    assert o.dtype == BF16 and torch.isfinite(o).all()
    err = (o.double() - ref).abs().max().item()
    print(f"{name}: max abs err {err:.3e}")
    assert torch.allclose(o.double(), ref, atol=ATOL, rtol=RTOL), name
    # slot pos[b] holds quantize_kv of the qkv row; nothing else changed
    B, H = k.shape[:2]
    new = qkv.view(B, 3, H, HS)
    for cache, scale, c0, s0, part in ((k, ks, before[0], before[2], 1),
                                       (v, vs, before[1], before[3], 2)):
        want_c, want_s = c0.view(torch.uint8).clone(), s0.clone()
        codes, s = da.quantize_kv(new[:, part])
        for b, p in enumerate(pos_list):
            want_c[b, :, p] = codes[b].view(torch.uint8)
            want_s[b, :, p] = s[b]
        assert torch.equal(cache.view(torch.uint8), want_c), name
        assert torch.equal(scale.view(torch.int32), want_s.view(torch.int32))
    return o


SINGLE = [(C, 0), (C, 1), (C, 15), (C, 16), (C, 17), (C, C - 1),
          (2 * C, C - 1), (2 * C, C), (2 * C, C + 1)]


@pytest.mark.parametrize("Tmax,p", SINGLE)
def test_one_row_at_the_chunk_and_wave_load_edges(Tmax, p):
    _check(_case(1, 1, Tmax, [p], seed=p), [p], None, f"T{Tmax}p{p}")


def test_ragged_rows_and_batch_independence():
    pos_list, mp = [0, C + 37, 4 * C - 1], 4 * C - 1
    case = _case(3, 2, 4 * C, pos_list, seed=3)
    again = [t.clone() for t in case]
    alone = [t.clone() for t in case]
    o = _check(case, pos_list, mp, "ragged")
    qkv, k, v, ks, vs, pos = again
    o2 = da.decode_attention(qkv, k, v, pos, mp, k_scale=ks, v_scale=vs)
    assert torch.equal(o2.view(torch.int16), o.view(torch.int16))
    for t2, t1 in zip(again[1:5], case[1:5]):
        assert torch.equal(t2.view(torch.uint8), t1.view(torch.uint8))
    for b, p in enumerate(pos_list):
        qkv, k, v, ks, vs, pos = (t[b:b + 1].contiguous() for t in alone)
        ob = da.decode_attention(qkv, k, v, pos, p, k_scale=ks, v_scale=vs)
        assert torch.equal(ob.view(torch.int16),
                           o[b:b + 1].view(torch.int16)), f"row {b}"


def test_odd_head_count():
    pos_list = [2 * C - 1, C + 5]
    _check(_case(2, 25, 2 * C, pos_list, seed=5), pos_list, 2 * C - 1, "H25")


@pytest.mark.parametrize("exp", [-3, 0, 5])
def test_every_e4m3_code_dequantizes_exactly(exp):
    """Slot 0 and the new token carry the same dequantized row of codes;
    with q = 0 and pos = 1 the output is v / 2 + v / 2, exactly v."""
    code = torch.arange(256, dtype=torch.uint8)
    code[(code & 0x7F) == 0x7F] = 0
    v8 = code.view(1, 4, 1, HS).to(DEV).view(FP8)
    vs = torch.full((1, 4, 1), 2.0 ** exp, device=DEV)
    row = da.dequantize_kv(v8, vs)                        # [1, 4, 1, 64] bf16
    newq, news = da.quantize_kv(row[:, :, 0])
    assert torch.equal(da.dequantize_kv(newq, news), row[:, :, 0])
    H, Tmax = 4, C
    k = torch.zeros(1, H, Tmax, HS, dtype=torch.uint8, device=DEV).view(FP8)
    v = k.clone()
    v.view(torch.uint8)[:, :, :1] = v8.view(torch.uint8)
    ks = torch.ones(1, H, Tmax, device=DEV)
    vsc = ks.clone()
    vsc[:, :, :1] = vs
    qkv = torch.zeros(1, 3, H, HS, dtype=BF16, device=DEV)
    qkv[:, 2] = row[:, :, 0]
    pos = torch.ones(1, dtype=torch.int32, device=DEV)
    o = da.decode_attention(qkv.view(1, -1), k, v, pos, 1, k_scale=ks,
                            v_scale=vsc)
    # a code of -0 adds to the accumulator's +0
    want = (row[:, :, 0].float() + 0.0).to(BF16).view(1, -1)
    assert torch.equal(o.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("T", [1, 17, C + 1])
def test_fill_kernel(T):
    B, H, Tmax = 2, 3, 2 * C
    g = torch.Generator().manual_seed(T)
    qkv = (torch.randn(B, T, 3, H, HS, generator=g) * torch.exp2(
        torch.randint(-8, 9, (B, T, 3, H, 1), generator=g).float()))
    qkv[1, T // 2, 1, 2] = 0                               # an all-zero k row
    qkv = qkv.to(DEV, BF16)
    k = torch.full((B, H, Tmax, HS), 0x5A, dtype=torch.uint8,
                   device=DEV).view(FP8)
    v = k.clone()
    ks = torch.full((B, H, Tmax), -7.0, device=DEV)
    vs = ks.clone()
    da.kv_cache_fill(qkv.view(B, T, -1), k, v, ks, vs)
    for cache, scale, part in ((k, ks, 1), (v, vs, 2)):
        codes, s = da.quantize_kv(qkv[:, :, part].transpose(1, 2))
        assert torch.equal(cache[:, :, :T].view(torch.uint8),
                           codes.view(torch.uint8))
        assert torch.equal(scale[:, :, :T], s)
        assert (cache[:, :, T:].view(torch.uint8) == 0x5A).all()
        assert (scale[:, :, T:] == -7.0).all()
    assert ks[1, 2, T // 2] == 1 and \
        (k[1, 2, T // 2].view(torch.uint8) == 0).all()


def _block_step(m16, seed=0):
    """Block 0's decode_layer over a random fp8 cache, pos [5, 1, 12]."""
    g = torch.Generator().manual_seed(seed)
    B, H, Tmax = 3, 2, C
    x = torch.randn(B, 128, generator=g).to(DEV, BF16)
    res = torch.randn(B, 128, generator=g).to(DEV, BF16)
    kv = torch.randn(2, B, H, Tmax, HS, generator=g).to(DEV, BF16)
    pos = torch.tensor([5, 1, 12], dtype=torch.int32, device=DEV)
    (k, ks), (v, vs) = da.quantize_kv(kv[0]), da.quantize_kv(kv[1])
    blk = m16.h[0]
    out = sl.decode_layer(x, res, blk.ln_1, blk.attn.c_attn, k, v, pos, 12,
                          blk.attn.c_proj, blk.ln_2, blk.mlp.c_fc,
                          blk.mlp.c_proj, ks, vs)
    return out, (x, res), (k, v, ks, vs)


def _block_reference(blk, x, res, caches):
    """The block in fp64, attending the cache as the call left it."""
    F = torch.nn.functional
    ln = lambda m, t: F.layer_norm(t, t.shape[-1:], m.weight.double(),
                                   m.bias.double(), m.eps)
    lin = lambda m, t: F.linear(t, m.weight.double(), m.bias.double())
    x1 = x.double() + res.double()
    qkv = lin(blk.attn.c_attn, ln(blk.ln_1, x1))
    x_mid = x1 + lin(blk.attn.c_proj,
                     _reference(qkv, *caches, [5, 1, 12]))
    hid = F.gelu(lin(blk.mlp.c_fc, ln(blk.ln_2, x_mid)), approximate="tanh")
    return x_mid, lin(blk.mlp.c_proj, hid)


@pytest.mark.parametrize("weights_fp8", [False, True])
def test_decode_layer_one_call_against_composed(weights_fp8, monkeypatch):
    """The one C++ call against the block composed in Python on the twin
    (RLA_DECODE_ATTN=0): the caches bit for bit, and e_one_call <=
    2 * e_composed against fp64, as tests/test_skinny_linear_gpu.py."""
    monkeypatch.setenv("RLA_SKINNY_LINEAR", "1")
    m16, _ = tiny_models(256, DEV)
    if weights_fp8:
        m16.quantize_weights_fp8()
    asked = []
    monkeypatch.setattr(sl, "_ext_with", lambda s, _f=sl._ext_with:
                        (asked.append(s), _f(s))[1])
    one, (x, res), caches = _block_step(m16)
    assert ("decode_layer_fp8_fwd" if weights_fp8 else "decode_layer_fwd") \
        in asked
    monkeypatch.setenv("RLA_DECODE_ATTN", "0")
    monkeypatch.setattr(da, "_twin", _TWIN)
    composed, _, caches0 = _block_step(m16)
    for a, b in zip(caches, caches0):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    ref = _block_reference(m16.h[0], x, res, caches)
    for i in range(2):  # x_mid, mlp_out
        e_one = (one[i].double() - ref[i]).abs().max().item()
        e_comp = (composed[i].double() - ref[i]).abs().max().item()
        assert torch.isfinite(one[i]).all() and e_one <= 2 * e_comp


def _fp8_errors(m16, m32, idx, lens, new):
    """Largest logit error of a greedy kv_fp8 run against fp32."""
    out, logits = m16.generate(idx, new, prompt_lens=lens, temperature=0.0,
                               return_logits=True, kv_fp8=True)
    e = 0.0
    with torch.no_grad():
        for b, n in enumerate(lens):
            ref = m32(out[b, :n + new][None])[0][0, n - 1:n - 1 + new]
            e = max(e, (logits[b] - ref.float()).abs().max().item())
    return e


@pytest.mark.parametrize("skinny", ["0", "1"])
def test_generate_kernels_against_twins(skinny, monkeypatch):
    """The kernels against the same call on the twins, both against the
    fp32 model: e_kernel <= 2 * e_twin, as tests/test_generate_gpu.py."""
    monkeypatch.setenv("RLA_SKINNY_LINEAR", skinny)
    m16, m32 = tiny_models(256, DEV)
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 256, (3, 12), generator=g).to(DEV)
    calls = []
    monkeypatch.setattr(da, "_load_ext", lambda: _Spy(calls))
    e_kernel = _fp8_errors(m16, m32, idx, [5, 1, 12], 32)
    if skinny == "0":
        assert calls.count("decode_attn_fwd") == 2 * 31
    assert calls.count("kv_cache_fill") == 2
    monkeypatch.setenv("RLA_DECODE_ATTN", "0")
    monkeypatch.setattr(da, "_twin", _TWIN)
    del calls[:]
    e_twin = _fp8_errors(m16, m32, idx, [5, 1, 12], 32)
    assert not calls
    print(f"skinny {skinny}: e_kernel {e_kernel:.3e}  e_twin {e_twin:.3e}")
    assert e_kernel <= 2 * e_twin


class _Spy:
    """The extension, recording calls made through ops/decode_attn.py."""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        fn = getattr(EXT, name)
        if name not in ("decode_attn_fwd", "kv_cache_fill"):
            return fn
        return lambda *a: (self._calls.append(name), fn(*a))[1]


def test_operand_checks_raise_before_any_launch():
    pos_list = [3, 5]
    qkv, k, v, ks, vs, pos = _case(2, 2, 2 * C, pos_list)
    before = [t.clone() for t in (k, v, ks, vs)]
    kb = torch.zeros(2, 2, 2 * C, HS, dtype=BF16, device=DEV)
    bad = [
        ("scales without an fp8 cache", (kb, kb.clone(), ks, vs)),
        ("one scale only", (k, v, ks, None)),
        ("scale shape", (k, v, ks[:, :, :C].contiguous(), vs)),
        ("scale dtype", (k, v, ks, vs.to(BF16))),
    ]
    for name, (a, b, c, d) in bad:
        with pytest.raises(RuntimeError):
            EXT.decode_attn_fwd(qkv, a, b, pos, 2 * C - 1, SCALE, c, d)
    with pytest.raises(RuntimeError):  # T > Tmax
        EXT.kv_cache_fill(torch.zeros(2, 2 * C + 1, 3 * 2 * HS, dtype=BF16,
                                      device=DEV), k, v, ks, vs)
    torch.cuda.synchronize()
    for t, t0 in zip((k, v, ks, vs), before):
        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8))


def test_gate_off_runs_the_twin(monkeypatch):
    pos_list = [0, C + 37, 4 * C - 1]
    case = _case(3, 2, 4 * C, pos_list, seed=3)
    monkeypatch.setenv("RLA_DECODE_ATTN", "0")
    called = []
    monkeypatch.setattr(da, "_twin", lambda *a: (called.append(1),
                                                 _TWIN(*a))[1])
    _check(case, pos_list, 4 * C - 1, "twin")
    assert called
