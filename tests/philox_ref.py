"""numpy Philox4x32-10 and the keep mask the fused dropout+LayerNorm
kernels define (ops/csrc/fused_ln.hip): element ``i`` of the flattened
tensor is kept iff word ``i & 3`` of
``philox(key=seed, counter=(offset // 4, i >> 2))`` is ``>= floor(p * 2**32)``.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(key, ctr):
    """key: (k0, k1) ints; ctr: four uint64 arrays holding 32-bit words.
    Returns the four output words as uint64 arrays."""
    k0, k1 = int(key[0]), int(key[1])
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO,
                          (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO)
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep_mask(seed, offset, numel, p):
    """Boolean keep mask, flat, for ``numel`` (a multiple of 4) elements."""
    assert numel % 4 == 0
    g = np.arange(numel // 4, dtype=np.uint64)
    o = np.uint64(offset // 4)
    words = philox4x32_10(
        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF),
        (np.full_like(g, o & _LO), np.full_like(g, o >> _S32),
         g & _LO, g >> _S32))
    thr = np.uint64(min(int(p * 2.0 ** 32), 0xFFFFFFFF))
    return (np.stack(words, axis=1) >= thr).reshape(-1)
