"""Document-masked attention for packed rows, the parts that need no
GPU: the bounds helper, the SDPA fallback of ``flash_attention(...,
doc_ids=)``, ``GPT2.forward(..., doc_ids=)`` and ``document_ids``.

Tolerance: the fallback and the document run alone are the same fp32
SDPA math on the same numbers, in a different reduction order; the
worst absolute difference measured is 1.2e-7, so ``atol = rtol = 1e-5``
leaves two decimal orders."""
import pytest
import torch

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config, document_ids
from ray_lightning_amd.ops import flash_attn as fa
from ray_lightning_amd.ops.flash_attn import doc_bounds, flash_attention

TOL = dict(atol=1e-5, rtol=1e-5)


def _ids(lengths, first=0):
    """ids of one row: consecutive documents of these lengths."""
    return torch.cat([torch.full((n,), first + i, dtype=torch.int64)
                      for i, n in enumerate(lengths)])


# ------------------------------------------------------------- bounds
def test_bounds_length_one_document_at_zero():
    start, end = doc_bounds(torch.tensor([[5, 7, 7, 7, 2, 2]]))
    assert start.tolist() == [[0, 1, 1, 1, 4, 4]]
    assert end.tolist() == [[0, 3, 3, 3, 5, 5]]
    assert start.dtype == end.dtype == torch.int32


def test_bounds_returning_id_starts_a_new_document():
    start, end = doc_bounds(torch.tensor([[1, 1, 2, 1, 1, 1, 2]]))
    assert start.tolist() == [[0, 0, 2, 3, 3, 3, 6]]
    assert end.tolist() == [[1, 1, 2, 5, 5, 5, 6]]


def test_bounds_rows_differ():
    start, end = doc_bounds(torch.tensor([[0, 0, 0, 1, 1],
                                          [3, 4, 4, 4, 4]],
                                         dtype=torch.int32))
    assert start.tolist() == [[0, 0, 0, 3, 3], [0, 1, 1, 1, 1]]
    assert end.tolist() == [[2, 2, 2, 4, 4], [0, 4, 4, 4, 4]]
    assert start.is_contiguous() and end.is_contiguous()


def test_bounds_one_document():
    start, end = doc_bounds(torch.full((2, 9), 4))
    assert (start == 0).all() and (end == 8).all()


def test_bounds_match_a_python_loop():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 3, (3, 40), generator=g)
    start, end = doc_bounds(ids)
    for b in range(3):
        s = 0
        for t in range(40):
            if t and ids[b, t] != ids[b, t - 1]:
                s = t
            assert start[b, t] == s
        e = 39
        for t in reversed(range(40)):
            if t < 39 and ids[b, t] != ids[b, t + 1]:
                e = t
            assert end[b, t] == e


# ---------------------------------------------------------- attention
LAYOUT = [[70, 58], [64, 64]]


def _qkv(B=2, H=3, T=128, hs=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, T, hs, generator=g) for _ in range(3)]


def test_each_document_equals_the_document_alone():
    q, k, v = _qkv()
    ids = torch.stack([_ids(row) for row in LAYOUT])
    o = flash_attention(q, k, v, doc_ids=ids)
    worst = 0.0
    for b, row in enumerate(LAYOUT):
        s = 0
        for n in row:
            sl = slice(s, s + n)
            alone = flash_attention(q[b:b + 1, :, sl], k[b:b + 1, :, sl],
                                    v[b:b + 1, :, sl])
            worst = max(worst, (o[b:b + 1, :, sl] - alone).abs().max().item())
            torch.testing.assert_close(o[b:b + 1, :, sl], alone, **TOL)
            s += n
    print(f"worst abs diff {worst:.3e}")
    # and the masking did something
    assert not torch.allclose(o, flash_attention(q, k, v), **TOL)


def test_precomputed_pair_is_accepted():
    q, k, v = _qkv()
    ids = torch.stack([_ids(row) for row in LAYOUT])
    assert torch.equal(flash_attention(q, k, v, doc_ids=doc_bounds(ids)),
                       flash_attention(q, k, v, doc_ids=ids))


def test_gradients_stay_inside_the_document():
    q, k, v = _qkv(B=1, H=1)
    q.requires_grad_(True)
    k.requires_grad_(True)
    ids = _ids([70, 58])[None]
    o = flash_attention(q, k, v, doc_ids=ids)
    o[:, :, 70:].sum().backward()
    assert (k.grad[:, :, :70] == 0).all() and (q.grad[:, :, :70] == 0).all()
    assert k.grad[:, :, 70:].abs().sum() > 0


def test_none_is_todays_call():
    q, k, v = _qkv()
    assert torch.equal(flash_attention(q, k, v, doc_ids=None),
                       flash_attention(q, k, v))
    assert torch.equal(flash_attention(q, k, v, 0.0, None),
                       flash_attention(q, k, v))


@pytest.mark.parametrize("bad", [
    torch.zeros(2, 64, dtype=torch.int64),        # T
    torch.zeros(3, 128, dtype=torch.int64),       # B
    torch.zeros(2, 3, 128, dtype=torch.int64),    # rank
    torch.zeros(2, 128, dtype=torch.float32),     # dtype
    torch.zeros(2, 128, dtype=torch.bfloat16),
])
def test_bad_ids_raise(bad):
    q, k, v = _qkv()
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_ids=bad)


def test_bad_pair_raises():
    q, k, v = _qkv()
    start, end = doc_bounds(torch.zeros(2, 128, dtype=torch.int64))
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_ids=(start, end[:, :64]))
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_ids=(start.float(), end))
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_ids=(start,))


def test_gate_helper_follows_the_environment(monkeypatch):
    monkeypatch.delenv("RLA_FLASH_DOCS", raising=False)
    assert fa._docs_kernels_enabled() == fa._DOCS_DEFAULT
    monkeypatch.setenv("RLA_FLASH_DOCS", "0")
    assert not fa._docs_kernels_enabled()
    monkeypatch.setenv("RLA_FLASH_DOCS", "1")
    assert fa._docs_kernels_enabled()


# --------------------------------------------------------------- GPT-2
def _tiny_gpt2():
    torch.manual_seed(1)
    cfg = GPT2Config(vocab_size=97, n_positions=32, n_embd=64, n_layer=2,
                     n_head=2)
    return GPT2(cfg).eval()


def test_gpt2_packed_row_equals_documents_alone():
    model = _tiny_gpt2()
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 97, (2, 32), generator=g)
    layout = [[13, 19], [1, 20, 11]]
    ids = torch.stack([_ids(row) for row in layout])
    with torch.no_grad():
        packed = model(idx, doc_ids=ids)[0]
        plain = model(idx)[0]
        for b, row in enumerate(layout):
            s = 0
            for n in row:
                alone = model(idx[b:b + 1, s:s + n])[0]
                torch.testing.assert_close(packed[b:b + 1, s:s + n], alone,
                                           **TOL)
                s += n
    # without doc_ids the second document sees the first
    assert not torch.allclose(packed[0, 13:], plain[0, 13:], **TOL)
    torch.testing.assert_close(packed[0, :13], plain[0, :13], **TOL)


def test_gpt2_loss_takes_doc_ids():
    model = _tiny_gpt2()
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 97, (2, 32), generator=g)
    tgt = torch.randint(0, 97, (2, 32), generator=g)
    ids = torch.stack([_ids([13, 19]), _ids([32])])
    _, a = model(idx, tgt, doc_ids=ids)
    _, b = model(idx, tgt)
    assert torch.isfinite(a) and a != b
    with pytest.raises(ValueError):
        model(idx, tgt, doc_ids=ids[:, :16])


def test_block_forward_takes_doc_ids():
    model = _tiny_gpt2()
    x = torch.randn(1, 32, 64, generator=torch.Generator().manual_seed(4))
    ids = _ids([13, 19])[None]
    with torch.no_grad():
        y = model.h[0](x, doc_ids=ids)
        alone = model.h[0](x[:, 13:])
    torch.testing.assert_close(y[:, 13:], alone, **TOL)


# -------------------------------------------------------- document_ids
def test_document_ids_eos_first_middle_last():
    eos = 9
    idx = torch.tensor([[eos, 1, 2, eos, 3, 4, 5, eos],
                        [1, 2, 3, 4, 5, 6, 7, 8]])
    ids = document_ids(idx, eos)
    # the EOS belongs to the document it ends
    assert ids.tolist() == [[0, 1, 1, 1, 2, 2, 2, 2],
                            [0, 0, 0, 0, 0, 0, 0, 0]]
    start, end = doc_bounds(ids)
    assert start.tolist()[0] == [0, 1, 1, 1, 4, 4, 4, 4]
    assert end.tolist()[0] == [0, 3, 3, 3, 7, 7, 7, 7]


def test_gpt2lm_derives_doc_ids_from_eos():
    from ray_lightning_amd.models.benchmark import GPT2LM
    assert GPT2LM.__init__.__defaults__[-1] is None   # default: off

    seen = []

    class Recorder(torch.nn.Module):
        def forward(self, idx, targets=None, doc_ids=None):
            seen.append(doc_ids)
            return None, torch.zeros(())

    # the module without its 124M-parameter model
    lm = GPT2LM.__new__(GPT2LM)
    torch.nn.Module.__init__(lm)
    lm.model = Recorder()
    lm.log = lambda *a, **k: None
    x = torch.tensor([[1, 9, 2, 3]])
    lm.doc_eos_id = None
    lm.training_step((x, x), 0)
    lm.doc_eos_id = 9
    lm.training_step((x, x), 0)
    assert seen[0] is None
    assert seen[1].tolist() == [[0, 0, 1, 1]]
