// Counter-based dropout mask shared by the fused dropout+LayerNorm
// kernels (fused_ln.hip) and the flash attention dropout kernels
// (flash_attn.hip).
//
// keep(i) for flat element i of the dropped tensor is
//   word[i & 3] of Philox4x32-10(key = seed, counter = (offset/4, i>>2))
//   >= floor(p * 2^32)
// i.e. one Philox call per aligned group of four elements, one 32-bit
// word per element: a pure function of (seed, offset, i). The counter
// layout is the one torch's own Philox consumers use (offset/4 in the
// low 64 bits, the "subsequence" i>>2 in the high 64), so advancing the
// generator's offset by 4 per call keeps every (key, counter) pair
// unique among all users of that generator. tests/philox_ref.py is the
// same function in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

namespace {

struct DropArgs {
  uint32_t k0, k1;   // Philox key = seed
  uint32_t o0, o1;   // counter low half = offset / 4
  uint32_t thr;      // drop iff word < thr
  float scale;       // 1 / (1-p)
};

__device__ __forceinline__ uint4 philox4x32_10(uint32_t k0, uint32_t k1,
                                               uint4 c) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  #pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32x32->64 multiply gives the hi and lo words together
    const uint64_t p0 = (uint64_t)kM0 * c.x;
    const uint64_t p1 = (uint64_t)kM1 * c.z;
    c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1,
                   (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

inline DropArgs make_drop_args(double p, uint64_t seed, uint64_t offset) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "fused_dropout_ln: p must be in [0, 1)");
  DropArgs d;
  d.k0 = (uint32_t)seed;
  d.k1 = (uint32_t)(seed >> 32);
  const uint64_t ctr = offset >> 2;
  d.o0 = (uint32_t)ctr;
  d.o1 = (uint32_t)(ctr >> 32);
  d.thr = (uint32_t)std::min<uint64_t>((uint64_t)(p * 4294967296.0),
                                       0xFFFFFFFFull);
  d.scale = (float)(1.0 / (1.0 - p));
  return d;
}

}  // namespace
