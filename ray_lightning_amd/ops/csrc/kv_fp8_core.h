// The KV cache's fp8 format in integer arithmetic, shared by the decode
// kernel's append and the fill kernel of decode_attn.hip and by the append
// kernel of append_attn.hip. docs/DESIGN.md
// §20 has the contract; in short, for a row x[0 .. 63] of bf16:
//
//   scale = 2^ceil(log2(absmax / 448)), 1 for an all-zero row
//   code  = RNE_e4m3(x / scale)        OCP float8_e4m3fn, |x / scale| <= 448
//
// which is ops/decode_attn.py's quantize_kv bit for bit. Everything works
// on the operands' bit patterns: dividing by a power of two is a
// subtraction of exponents, so subnormal inputs and scales need no
// floating-point mode, and the functions compile for the host as well
// (that is how they were checked against torch over every bf16 value).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KV_HD __host__ __device__ __forceinline__
#else
#define KV_HD inline
#endif

// Biased exponent `se` of the scale, scale = 2^(se - 127), for an absmax
// given as the bits of |x| widened to fp32 (bf16 bits << 16). May be <= 0:
// the scale is then an fp32 subnormal. 448 = 1.75 * 2^8, so with
// absmax = m * 2^e, 1 <= m < 2, ceil(log2(absmax / 448)) is e - 8 for
// m <= 1.75 and e - 7 above. Call it for finite, non-zero absmax only.
KV_HD int kv_scale_exp(unsigned amax) {
  int E = (int)(amax >> 23);
  unsigned M = amax & 0x7fffffu;
  if (E == 0) {  // bf16 subnormal: bring the leading one to bit 23
    int shift = 0;
    while (!(M & 0x800000u)) {
      M <<= 1;
      ++shift;
    }
    M &= 0x7fffffu;
    E = 1 - shift;
  }
  return E - 8 + (M > 0x600000u ? 1 : 0);
}

// The fp32 bits of the scale: 1 for absmax = 0, NaN for a row that holds
// an infinity or a NaN (so that its output shows NaN).
KV_HD unsigned kv_scale_bits(unsigned amax) {
  if (amax == 0) return 0x3f800000u;
  if (amax >= 0x7f800000u) return 0x7fc00000u;
  const int se = kv_scale_exp(amax);
  return se >= 1 ? (unsigned)se << 23 : 1u << (se + 22);  // se >= -22
}

// One bf16 value (its 16 bits) divided by 2^(se - 127) and rounded to
// nearest even e4m3. The caller guarantees |x / scale| <= 448, so the
// exponent never passes 8 and nothing saturates.
KV_HD unsigned kv_quant(unsigned x, int se) {
  const unsigned sign = (x >> 8) & 0x80u;
  int E = (int)((x >> 7) & 0xffu);
  unsigned sig = x & 0x7fu;  // 8-bit significand: sig * 2^(E - 134)
  if (E != 0) {
    sig |= 0x80u;
  } else {  // zero, or a bf16 subnormal: bring the leading one to bit 7
    if (sig == 0) return sign;
    E = 1;
    while (!(sig & 0x80u)) {
      sig <<= 1;
      --E;
    }
  }
  // x / scale = sig * 2^(e - 7). From e = -6 up the code is normal: three
  // mantissa bits, so four are dropped, and exponent field (e + 7); below,
  // the e4m3 subnormals are multiples of 2^-9.
  const int e = E - se;
  int drop = 4, base = 0;
  if (e >= -6) base = (e + 6) * 8;
  else drop = 4 + (-6 - e);
  if (drop > 9) return sign;  // under half the smallest subnormal
  unsigned r = sig >> drop;
  const unsigned rem = sig & ((1u << drop) - 1u), half = 1u << (drop - 1);
  r += (rem > half || (rem == half && (r & 1u))) ? 1u : 0u;
  // r carries the implicit one (8 .. 16) for a normal code: 16 steps into
  // the next exponent by plain addition
  return sign | (unsigned)(base + (int)r);
}

#if defined(__HIPCC__)
// ---- a row of 64 bf16 held by 4 lanes, 16 values each (two uint4 a, b):
// the layout of the decode kernel's append, the fill kernel and the append
// kernel's new rows ------------------------------------------------------

// largest |x| of 16 bf16 values, as fp32 bits (non-finite values sort on
// top, which is what kv_scale_bits wants)
__device__ __forceinline__ unsigned kv_amax16(const uint4& a, const uint4& b) {
  const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned m = 0;
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    m = max(m, (w[i] << 16) & 0x7fff0000u);
    m = max(m, w[i] & 0x7fff0000u);
  }
  return m;
}

// 16 bf16 values as 16 e4m3 codes under scale 2^(se - 127), low byte first
__device__ __forceinline__ uint4 kv_quant16(const uint4& a, const uint4& b,
                                            int se) {
  const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned o[4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = kv_quant(w[2 * i] & 0xffffu, se) |
           kv_quant(w[2 * i] >> 16, se) << 8 |
           kv_quant(w[2 * i + 1] & 0xffffu, se) << 16 |
           kv_quant(w[2 * i + 1] >> 16, se) << 24;
  return uint4{o[0], o[1], o[2], o[3]};
}

// The row's absmax as fp32 bits. Its 4 lanes are `stride` and 2 * `stride`
// apart (1: adjacent lanes); every lane of the wave runs the shuffles.
__device__ __forceinline__ unsigned kv_row_amax(const uint4& a, const uint4& b,
                                                int stride = 1) {
  unsigned amax = kv_amax16(a, b);
  amax = max(amax, (unsigned)__shfl_xor((int)amax, stride, 64));
  amax = max(amax, (unsigned)__shfl_xor((int)amax, 2 * stride, 64));
  return amax;
}

// This lane's 16 codes of the row with that absmax. A zero row has scale 1
// (its codes are signed zeros); a non-finite one gets the NaN code next to
// its NaN scale.
__device__ __forceinline__ uint4 kv_quant_row(const uint4& a, const uint4& b,
                                              unsigned amax) {
  if (amax >= 0x7f800000u)
    return uint4{0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu};
  return kv_quant16(a, b, amax == 0 ? 127 : kv_scale_exp(amax));
}
#endif
