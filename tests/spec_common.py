"""Plain-Python reference for ops/spec_decode.py, shared by
test_spec_decode_cpu.py (torch twin) and test_spec_decode_gpu.py (HIP
kernel). Tokens are checked against ``sample_tokens`` row by row; commit
and draft against ``ref_commit`` / ``ref_draft``, written from the
contract's text."""
import torch

from sample_common import make_rows
from ray_lightning_amd.ops import spec_decode as sd
from ray_lightning_amd.ops.sample import sample_tokens

SAMPLERS = [dict(temperature=0.0), dict(temperature=1.0, top_k=40),
            dict(temperature=0.7, top_p=0.9),
            dict(temperature=1.0, top_k=40, top_p=0.9)]


def ref_draft(h, ngram, n, pad):
    if not h:
        return [pad] * (1 + n)
    col, e = len(h), list(h)
    for g in range(min(ngram, col - 1), 0, -1):
        for s in range(col - 1 - g, -1, -1):
            if h[s:s + g] == h[col - g:col]:
                for j in range(n):
                    e.append(e[s + g + j])
                return e[col - 1:]
    return [h[-1]] * (1 + n)


def ref_commit(row, toks, out_row, limit, eos, pad):
    """Updates ``row`` (fin, em, col, pos) and ``out_row``; returns n."""
    T, L = len(toks) - 1, len(out_row)
    a = T
    if not row["fin"]:
        a = 0
        while a < T and toks[a] == row["draft"][a]:
            a += 1
    n = max(0, min(a + 1, limit - row["em"]))
    for j in range(n):
        x = pad if row["fin"] else toks[j]
        row["fin"] = row["fin"] or x == eos
        if row["col"] + j < L:
            out_row[row["col"] + j] = x
    row["col"] += n
    row["em"] += n
    row["pos"] += n - (T + 1)
    return n


def check_step(dev, logits, rows, L, limit, sampler, eos=None, pad=0,
               ngram=3, next_T=4):
    """One ``spec_step`` on ``rows`` (dicts with h, draft, fin, em)
    against the reference; every output and state tensor exactly.
    Returns the tensors of the call."""
    B, T1, V = logits.shape
    logits = logits.to(dev)
    if dev != "cpu":
        assert sd._kernel_shape(logits), "the kernel does not serve this"
    seeds = (torch.arange(B, dtype=torch.int64) * 7919 - 3).to(dev)
    out = torch.full((B, L), 77, dtype=torch.int64)
    for b, r in enumerate(rows):
        out[b, :len(r["h"])] = torch.tensor(r["h"], dtype=torch.int64)
        r.update(col=len(r["h"]), pos=len(r["h"]) - 1 + T1)
    t = dict(
        draft=torch.tensor([r["draft"] for r in rows],
                           dtype=torch.int64).view(B, T1 - 1).to(dev),
        emitted=torch.tensor([r["em"] for r in rows]).to(dev),
        finished=torch.tensor([r["fin"] for r in rows]).to(dev),
        col=torch.tensor([r["col"] for r in rows]).to(dev),
        pos=torch.tensor([r["pos"] for r in rows],
                         dtype=torch.int32).to(dev),
        out=out.to(dev), done=torch.zeros(B, dtype=torch.int32).to(dev))
    want_tok = torch.stack([torch.cat([
        sample_tokens(logits[b, i][None], seeds[b:b + 1], r["em"] + i,
                      **sampler) for i in range(T1)])
        for b, r in enumerate(rows)]).cpu()
    want_out, want_n, want_next = out.tolist(), [], []
    for b, r in enumerate(rows):
        want_n.append(ref_commit(r, want_tok[b].tolist(), want_out[b],
                                 limit, eos, pad))
        want_next.append(ref_draft(want_out[b][:min(r["col"], L)], ngram,
                                   next_T, pad))
    tok, n_commit, next_idx = sd.spec_step(
        logits, t["draft"], seeds, t["emitted"], limit, eos=eos, pad=pad,
        finished=t["finished"], out=t["out"], col=t["col"], pos=t["pos"],
        done=t["done"], ngram=ngram, next_T=next_T, **sampler)
    assert torch.equal(tok.cpu(), want_tok)
    assert n_commit.tolist() == want_n
    assert next_idx.tolist() == want_next
    assert t["out"].tolist() == want_out
    for name, key in (("emitted", "em"), ("finished", "fin"),
                      ("col", "col"), ("pos", "pos")):
        assert t[name].tolist() == [r[key] for r in rows], name
    assert not t["done"].any()
    t.update(tok=tok, n_commit=n_commit, next_idx=next_idx)
    return t


def token_case(dev, V, B, T1, dtype):
    logits = make_rows(V, B * T1, dtype).view(B, T1, V)
    g = torch.Generator().manual_seed(V + T1)
    for sampler in SAMPLERS:
        rows = [dict(h=[1, 2, 3], fin=False, em=3 + 5 * b,
                     draft=torch.randint(0, V, (T1 - 1,),
                                         generator=g).tolist())
                for b in range(B)]
        check_step(dev, logits, rows, 40, 1000, sampler,
                      next_T=min(T1, 15))


def dominant(toks, V=64):
    """fp32 logits [B, T1, V] whose greedy tokens are ``toks``."""
    toks = torch.tensor(toks)
    return torch.zeros(*toks.shape, V).scatter_(2, toks[..., None], 10.0)


EOS, PAD, LIMIT, WIDTH = 9, 2, 10, 1030


def state_rows():
    """(rows, greedy tokens) of one batch, T = 4: the commit and the draft
    cases of the contract, one per row. A row at the limit commits
    nothing, so its history is the one written here."""
    g = torch.Generator().manual_seed(3)

    def rnd(n, k):
        return torch.randint(20, 20 + k, (n,), generator=g).tolist()

    def row(h, toks, draft, fin=False, em=0):
        return dict(h=h, draft=draft, fin=fin, em=em), toks

    at = dict(toks=[1] * 5, draft=[1] * 4, em=LIMIT)
    cases = [
        row(rnd(7, 3), [5, 6, 7, 8, 3], [4, 6, 7, 8]),            # a = 0
        row(rnd(7, 3), [5, 6, 7, 8, 3], [5, 6, 4, 8]),            # a = 2
        row(rnd(255, 3), [5, 6, 7, 8, 3], [5, 6, 7, 8]),          # a = T
        row(rnd(257, 3), [5, EOS, 7, 8, 3], [5, EOS, 7, 8]),      # EOS inside
        row(rnd(9, 3), [5, 6, 7, 8, 3], [0, 0, 0, 0], fin=True),  # finished
        row(rnd(9, 3), [5, 6, 7, 8, 3], [5, 6, 7, 8], em=LIMIT),  # at limit
        row(rnd(9, 3), [5, 6, 7, 8, 3], [5, 6, 7, 8], em=LIMIT - 2),
        row(rnd(WIDTH - 2, 3), [5, 6, 7, 8, 3], [5, 6, 7, 8]),    # past out
        row(list(range(100, 140)), **at),                         # no match
        row([5, 6, 7, 30, 31, 8, 5, 6, 7], **at),                 # 3-gram
        row([5, 6, 7, 30, 31, 9, 8, 7], **at),                    # 1-gram only
        row([5, 6, 7, 30, 5, 6, 7, 31, 40, 5, 6, 7], **at),       # later wins
        row([5, 6, 7, 30, 40, 6, 7, 31, 41, 5, 6, 7], **at),      # longer wins
        row([30, 1, 2, 1, 2], **at),                              # periodic
        row([4, 4], **at),                                        # len 2
        row(rnd(255, 2), **at), row(rnd(257, 2), **at),
        row(rnd(1023, 2), **at),
        # one match only, at the front and behind a wave boundary
        row([5, 6, 7, 8] + list(range(100, 1116)) + [5, 6, 7], **at),
        row(list(range(100, 165)) + [5, 6, 7, 8]
            + list(range(200, 1151)) + [5, 6, 7], **at),
    ]
    return [c[0] for c in cases], [c[1] for c in cases]


def bad_operands(dev):
    B, T1, V = 2, 3, 64
    i64 = dict(dtype=torch.int64, device=dev)
    ok = dict(logits=torch.zeros(B, T1, V, device=dev),
              draft=torch.zeros(B, T1 - 1, **i64),
              seeds=torch.zeros(B, **i64), emitted=torch.zeros(B, **i64),
              limit=4, temperature=1.0, top_k=None, top_p=None,
              finished=torch.zeros(B, dtype=torch.bool, device=dev),
              eos=None, pad=0, out=torch.zeros(B, 8, **i64),
              col=torch.ones(B, **i64),
              pos=torch.zeros(B, dtype=torch.int32, device=dev), ngram=3,
              next_T=2)
    bad = {
        "logits_2d": dict(logits=ok["logits"][:, 0]),
        "logits_int": dict(logits=ok["logits"].long()),
        "logits_strided": dict(logits=ok["logits"][:, :, ::2]),
        "T1_17": dict(logits=torch.zeros(B, 17, V, device=dev),
                      draft=torch.zeros(B, 16, **i64)),
        "draft_width": dict(draft=torch.zeros(B, T1, **i64)),
        "draft_int32": dict(draft=ok["draft"].int()),
        "seeds_short": dict(seeds=ok["seeds"][:1]),
        "emitted_int32": dict(emitted=ok["emitted"].int()),
        "finished_uint8": dict(finished=ok["finished"].to(torch.uint8)),
        "col_short": dict(col=ok["col"][:1]),
        "pos_int64": dict(pos=ok["pos"].long()),
        "out_int32": dict(out=ok["out"].int()),
        "out_too_long": dict(out=torch.zeros(B, 16385, **i64)),
        "limit_neg": dict(limit=-1),
        "ngram_0": dict(ngram=0), "ngram_9": dict(ngram=9),
        "next_T_16": dict(next_T=16), "next_T_neg": dict(next_T=-1),
        "eos_wide": dict(eos=2 ** 31), "pad_neg": dict(pad=-1),
        "temperature_neg": dict(temperature=-1.0),
        "top_k_zero": dict(top_k=0), "top_p_zero": dict(top_p=0.0),
    }
    if dev != "cpu":
        bad["seeds_cpu"] = dict(seeds=ok["seeds"].cpu())
    return ok, bad


def call(kw):
    kw = dict(kw)
    return sd.spec_step(kw.pop("logits"), kw.pop("draft"), kw.pop("seeds"),
                        kw.pop("emitted"), kw.pop("limit"), **kw)
