"""fp64 reference for ops/sample.py, shared by test_sample_cpu.py (torch
twin) and test_sample_gpu.py (HIP kernel).

A token ``t`` passes iff it is in the reference's kept set and
``cdf_excl(t) - DELTA <= u <= cdf_incl(t) + DELTA`` with ``u = x / 2^32``.
DELTA = 2^-14 is derived, not measured: the exponent argument is at most
40 in magnitude before the mass is zero and carries about three fp32
roundings plus one ulp of the exp2, so a weight is off by at most about
2^-17 relative, a ratio of sums of such positive terms by about 2^-16;
4x headroom. The 2^-40 floor of a mass adds at most V * 2^-40 < 2^-24.
"""
import numpy as np
import torch

from philox_ref import philox4x32_10

DELTA = 2.0 ** -14
FLT_MAX = float(np.finfo(np.float32).max)
VS = [1, 5, 1023, 1025, 4097, 50257, 65536]


def canon(row):
    l = row.double().numpy().copy()
    l[np.isnan(l)] = -np.inf
    l[l == np.inf] = FLT_MAX
    return l


class Ref:
    """Kept set and index-order CDF of one row."""
    def __init__(self, row, temperature, top_k, top_p):
        l = canon(row)
        self.l, self.V = l, l.size
        self.empty = not np.isfinite(l.max())
        self.greedy = temperature == 0
        if self.empty or self.greedy:
            return
        kept = np.ones(l.size, bool)
        if top_k is not None and top_k < l.size:
            kept = l >= np.sort(l)[::-1][top_k - 1]
        p = np.where(kept, np.exp((l - l.max()) / temperature), 0.0)
        p /= p.sum()
        if top_p is not None and top_p < 1.0:
            order = np.argsort(-l, kind="stable")
            ls, ps = l[order], p[order]
            above = np.cumsum(ps) - ps
            start = np.r_[True, ls[1:] != ls[:-1]]
            above = np.maximum.accumulate(np.where(start, above, -1.0))
            keep = np.zeros(l.size, bool)
            keep[order] = above < top_p
            kept &= keep
            p = np.where(kept, p, 0.0)
            p /= p.sum()
        self.kept = kept
        self.incl = np.cumsum(p)
        self.excl = self.incl - p

    def check(self, tok, seed, step):
        if self.empty or self.greedy:  # argmax: the first maximum
            assert tok == (0 if self.empty else int(np.argmax(self.l)))
            return
        seed &= 2 ** 64 - 1
        x = int(philox4x32_10((seed & 0xFFFFFFFF, seed >> 32),
                              (step & 0xFFFFFFFF, step >> 32, 0, 0))[0])
        u = x / 2.0 ** 32
        assert 0 <= tok < self.V and self.kept[tok], (tok, u)
        assert self.excl[tok] - DELTA <= u <= self.incl[tok] + DELTA, \
            (tok, u, self.excl[tok], self.incl[tok])


def midpoint_top_p(row, temperature, top_k, rank):
    """The midpoint of two consecutive cumulative masses of the sorted
    fp64 distribution over 2^-10 apart, at ``rank`` or the nearest below."""
    ref = Ref(row, temperature, top_k, None)
    ps = np.sort(ref.incl - ref.excl)[::-1]
    c = np.cumsum(ps)
    for j in range(min(rank, ps.size - 1), 0, -1):
        if ps[j] > 2.0 ** -10:
            return float((c[j - 1] + c[j]) / 2)
    raise AssertionError("no gap above 2^-10 in the head of the row")


def make_rows(V, B, dtype, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + V)
    rows = (4 * torch.randn(B, V, generator=g)).to(dtype)
    if B > 1 and V >= 8:
        rows[1, V // 2:] = -torch.inf   # half the row at -inf
        rows[1, 3] = torch.nan
    return rows


def configs(rows):
    """(temperature, top_k, top_p, logits) cases of one [B, V] batch.
    Top-p cases repeat row 0, whose midpoints they use."""
    B, V = rows.shape
    tie7 = rows.clone()
    if V >= 8:  # the 8th largest equals the 7th: both stay
        for r in tie7:
            idx = canon(r).argsort()[::-1]
            r[int(idx[7])] = r[int(idx[6])]
    tmax = rows.clone()
    if V >= 5:  # two maxima: greedy takes the lower index
        tmax[:, 1] = tmax[:, 4] = 30.0
    same = rows[:1].repeat(B, 1)
    out = [(1.0, None, None, rows), (1.0, 1, None, rows),
           (0.7, 7, None, tie7), (1.0, V, None, rows),
           (1.0, V + 5, 1.0, rows), (0.0, None, None, tmax),
           (0.0, 5, 0.5, tmax)]
    if V >= 5:
        for t, k, rank in ((1.0, None, 1), (0.7, None, 3), (1.0, None, 50),
                           (1.0, 40, 3), (0.7, 7, 1)):
            out.append((t, k, midpoint_top_p(same[0], t, k, rank), same))
    return out


def run_cases(sample_tokens, rows, dev):
    """Every config, 16 steps each, against the reference."""
    B = rows.shape[0]
    seeds = torch.arange(B, dtype=torch.int64) * 7919 - 3
    got = []
    for t, k, p, logits in configs(rows):
        refs = [Ref(r, t, k, p) for r in logits]
        on_dev = logits.to(dev)
        for step in range(16):
            step = step * (2 ** 29 + 1)      # both counter words move
            tok = sample_tokens(on_dev, seeds.to(dev), step, temperature=t,
                                top_k=k, top_p=p).cpu()
            assert tok.dtype == torch.int64 and tok.shape == (B,)
            for b in range(B):
                refs[b].check(int(tok[b]), int(seeds[b]), step)
            got.append(tok)
    return torch.stack(got)


def check_rows_alone(sample_tokens, rows, dev):
    """Two calls agree, and row b of the batch equals the row alone."""
    seeds = torch.tensor([11, -5, 2 ** 40])[:len(rows)]
    kw = dict(temperature=0.7, top_k=40, top_p=0.9)
    x = rows.to(dev)
    both = sample_tokens(x, seeds.to(dev), 3, **kw)
    assert torch.equal(both, sample_tokens(x, seeds.to(dev), 3, **kw))
    for b in range(len(rows)):
        alone = sample_tokens(x[b:b + 1].clone(), seeds[b:b + 1].to(dev), 3,
                              **kw)
        assert torch.equal(alone, both[b:b + 1])


def check_epilogue(sample_tokens, dev):
    g = torch.Generator().manual_seed(5)
    logits = (4 * torch.randn(4, 300, generator=g)).to(dev)
    logits[1, 17] = 60.0                      # row 1 emits 17 = eos
    seeds = torch.arange(4, dtype=torch.int64, device=dev)
    finished = torch.tensor([True, False, False, False], device=dev)
    out = torch.full((4, 6), -1, dtype=torch.int64, device=dev)
    col = torch.tensor([2, 5, 6, -1], dtype=torch.int64, device=dev)
    tok = sample_tokens(logits, seeds, 0, finished=finished, eos=17, pad=9,
                        out=out, col=col)
    plain = sample_tokens(logits, seeds, 0)
    assert tok.tolist() == [9, 17, int(plain[2]), int(plain[3])]
    assert finished.tolist() == [True, True, False, False]
    want = torch.full((4, 6), -1, dtype=torch.int64)
    want[0, 2], want[1, 5] = 9, 17            # cols 6 and -1: no store
    assert torch.equal(out.cpu(), want)


def bad_operands(dev):
    B, V = 2, 64
    ok = dict(logits=torch.zeros(B, V, device=dev),
              seeds=torch.zeros(B, dtype=torch.int64, device=dev), step=0,
              temperature=1.0, top_k=None, top_p=None, finished=None,
              out=None, col=None)
    fin = torch.zeros(B, dtype=torch.bool, device=dev)
    o = torch.zeros(B, 4, dtype=torch.int64, device=dev)
    c = torch.zeros(B, dtype=torch.int64, device=dev)
    bad = {
        "logits_1d": dict(logits=torch.zeros(V, device=dev)),
        "logits_int": dict(logits=ok["logits"].long()),
        "seeds_int32": dict(seeds=ok["seeds"].int()),
        "seeds_short": dict(seeds=ok["seeds"][:1]),
        "temperature_neg": dict(temperature=-1.0),
        "top_k_zero": dict(top_k=0),
        "top_p_zero": dict(top_p=0.0),
        "top_p_above_one": dict(top_p=1.5),
        "finished_alone": dict(finished=fin),
        "out_int32": dict(finished=fin, out=o.int(), col=c),
        "col_short": dict(finished=fin, out=o, col=c[:1]),
        "finished_uint8": dict(finished=fin.to(torch.uint8), out=o, col=c),
    }
    return ok, bad
