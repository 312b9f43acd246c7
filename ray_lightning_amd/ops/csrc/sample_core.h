// The sampling pipeline of one row of logits in one workgroup, shared by
// sample.hip (one row per sequence) and spec_decode.hip (T + 1 rows per
// sequence): top-k, top-p (nucleus) and a counter-based Philox draw.
// bf16 or fp32 rows of V <= 65536 elements, gfx950. docs/DESIGN.md §16
// has the contract; in short, for a row with its seed and step:
//
//   K   = { i : l_i >= the top_k-th largest logit }         (ties kept)
//   w_i = exp2((l_i - max l) * c),  c = fp32(log2 e / temperature)
//   m_i = floor(w_i * 2^40) as a 64-bit integer, 0 outside K
//   P   = clamp(llrint(top_p * M), 1, M),  M = sum m_i
//   N   = { i in K : sum of m_j over l_j > l_i  <  P }      (ties kept)
//   x   = word 0 of Philox4x32-10(seed, (step_lo, step_hi, 0, 0))
//   r   = floor(M_N * x / 2^32),  M_N = sum of m_i over N
//   token = lowest i in N whose inclusive mass prefix (index order) > r
//
// Every sum, histogram, scan and comparison of mass is 64-bit integer
// arithmetic, so no result depends on an order of summation: given the
// fp32 weights the token is exact, repeatable bit for bit, and a function
// of the row's logits, its seed and step alone.
//
// Shape of the kernel:
//  - one workgroup of 1024 threads per row; thread t owns IPT consecutive
//    elements, held in registers for the whole kernel (bf16 stays packed,
//    two to a register). IPT is 1, 4, 16 or 64, picked on the host. 64
//    fp32 elements do not fit a thread's 128 registers: that size holds
//    nothing and reads the row again, from L2, in every pass.
//  - the thread ranges are laid over the row so that every granule of
//    min(16, IPT * element size) bytes is aligned: the range of thread 0
//    starts up to one granule before the row. A granule that lies wholly
//    inside the row is one vector load; the two threads whose ranges
//    straddle an end load element by element, inside the row only.
//    Elements outside the row read as -inf, which no step can select.
//  - a value maps to a monotone 32-bit key. The top-k threshold is a radix
//    select over the key, 11 + 11 + 10 bits, on count histograms in LDS
//    (2048 bins); the top-p threshold is the same descent on histograms of
//    integer mass (64-bit LDS atomics, 16 KB), stopping in the first bin
//    from the top whose inclusive mass reaches P. The bins are searched by
//    a block-wide exclusive scan, two bins per thread from the top.
//  - the same scan, over per-thread sums of kept mass in index order,
//    finds the one thread whose range holds r; it walks its elements.
//  - no spins, no flags, nothing between workgroups; every loop bound is
//    a constant.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "philox_dropout.h"

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

constexpr int kSmThreads = 1024;
constexpr int kSmWaves = kSmThreads / 64;
constexpr int kSmBins = 2048;
constexpr int kSmMaxV = 65536;
constexpr uint32_t kSmNegInfKey = 0x007FFFFFu;  // sm_key(-inf)

// what every row of a launch shares
struct SampleCfg {
  double top_p;            // 1.0: no nucleus
  int V;
  uint32_t top_k;          // 0: keep all
  float c;                 // log2 e / temperature; unused when greedy
  int greedy;
};

struct SampleLds {
  union {
    unsigned long long mass[kSmBins];
    uint32_t count[kSmBins];
  } hist;
  unsigned long long wave_sum[kSmWaves];
  unsigned long long rem;
  uint32_t red[kSmWaves];
  uint32_t sel;
};

// monotone: a < b as floats (no NaN, -0 folded into +0) iff key(a) < key(b)
__device__ __forceinline__ uint32_t sm_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}

__device__ __forceinline__ float sm_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// floor(exp2((v - vmax) * c) * 2^40), 0 below the threshold key
__device__ __forceinline__ unsigned long long sm_mass(float v, uint32_t thr,
                                                      float vmax, float c) {
  if (sm_key(v) < thr) return 0;
  const float d = v - vmax;
  const float w = d == 0.f ? 1.f : __builtin_amdgcn_exp2f(d * c);
  return (unsigned long long)(w * 1099511627776.0f);
}

// A thread's IPT elements of the row, as loaded. 64 fp32 elements next to
// the working set do not fit the 128 registers a thread of 1024 has
// (profiles/fused_sample.md), so that one size holds nothing and reads
// each element again, from L2, in every pass.
template <bool BF16, int IPT>
struct SampleRow {
  static constexpr bool HOLD = BF16 || IPT < 64;
  // how far a pass over the elements unrolls: a held row is indexed by
  // constants only
  static constexpr int UNROLL = HOLD ? IPT : 4;
  static constexpr int ES = BF16 ? 2 : 4;
  static constexpr int GB = IPT * ES < 16 ? IPT * ES : 16;  // granule bytes
  static constexpr int VEC = GB / ES;                       // ... elements
  static constexpr int NG = IPT / VEC;
  static constexpr int NW = (IPT * ES + 3) / 4;
  static constexpr uint32_t kNegInf = BF16 ? 0xFF80u : 0xFF800000u;
  uint32_t w[HOLD ? NW : 1];
  const uint32_t* row32;  // !HOLD only, with first and V
  int first, V;

  // element e of the thread is row element first + e; row is the row's
  // first byte and row + first * ES is GB-aligned. Nothing outside the
  // row is dereferenced. The thread whose range straddles the row's
  // start and the one that straddles its end go element by element,
  // through their own IPT elements of stage (LDS, two such ranges): a
  // rolled loop there costs the other threads no registers.
  __device__ __forceinline__ void load(const char* row, int first, int V,
                                       uint32_t* stage) {
    if constexpr (!HOLD) {
      row32 = reinterpret_cast<const uint32_t*>(row);
      this->first = first;
      this->V = V;
      return;
    }
    if (first >= 0 && first + IPT <= V) {  // all but a thread or two
      const char* base = row + (long)first * ES;
      #pragma unroll
      for (int g = 0; g < NG; ++g) {
        const char* p = base + g * GB;
        if constexpr (GB == 16) {
          const uint4 r = *reinterpret_cast<const uint4*>(p);
          w[4 * g] = r.x; w[4 * g + 1] = r.y;
          w[4 * g + 2] = r.z; w[4 * g + 3] = r.w;
        } else if constexpr (GB == 8) {
          const uint2 r = *reinterpret_cast<const uint2*>(p);
          w[2 * g] = r.x; w[2 * g + 1] = r.y;
        } else if constexpr (GB == 4) {
          w[g] = *reinterpret_cast<const uint32_t*>(p);
        } else {
          w[g] = *reinterpret_cast<const unsigned short*>(p);
        }
      }
    } else if (first >= V) {  // wholly behind the row
      #pragma unroll
      for (int i = 0; i < NW; ++i)
        w[i] = BF16 ? (kNegInf << 16 | kNegInf) : kNegInf;
    } else {
      uint32_t* mine = stage + (first < 0 ? 0 : NW);
      #pragma unroll 1
      for (int j = 0; j < IPT; ++j) {
        const int i = first + j;
        const bool in = i >= 0 && i < V;
        if constexpr (BF16)
          reinterpret_cast<unsigned short*>(mine)[j] =
              in ? reinterpret_cast<const unsigned short*>(row)[i]
                 : (unsigned short)kNegInf;
        else
          mine[j] = in ? reinterpret_cast<const uint32_t*>(row)[i] : kNegInf;
      }
      #pragma unroll
      for (int i = 0; i < NW; ++i) w[i] = mine[i];
    }
  }

  // Called at the head of every pass over the elements: the compiler
  // must take the words as new, so it decodes them again in that pass
  // and does not keep 64 decoded values and keys alive next to them.
  __device__ __forceinline__ void pin() {
    if constexpr (!HOLD) {  // forget what the last pass read
      asm volatile("" : "+v"(row32));
      return;
    }
    #pragma unroll
    for (int i = 0; i < NW; ++i) asm volatile("" : "+v"(w[i]));
  }

  // NaN counts as -inf, +inf as the largest finite float, -0 as +0
  __device__ __forceinline__ float value(int e) const {
    uint32_t bits;
    if constexpr (!HOLD) {
      const int i = first + e;
      bits = kNegInf;
      if (i >= 0 && i < V) bits = row32[i];  // inside the row only
    } else if constexpr (BF16)
      bits = (e & 1) ? (w[e / 2] & 0xFFFF0000u) : (w[e / 2] << 16);
    else
      bits = w[e];
    const float v = __uint_as_float(bits);
    if (v != v) return -INFINITY;
    if (v == 0.f) return 0.f;
    return fminf(v, FLT_MAX);
  }
};

template <bool MAX>
__device__ __forceinline__ uint32_t sm_block_reduce(uint32_t v,
                                                    uint32_t* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d);
    v = MAX ? max(v, o) : min(v, o);
  }
  if (lane == 0) red[wave] = v;
  __syncthreads();
  v = red[lane & (kSmWaves - 1)];
  #pragma unroll
  for (int d = kSmWaves / 2; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d);
    v = MAX ? max(v, o) : min(v, o);
  }
  __syncthreads();  // red is free again
  return v;
}

// Exclusive prefix of v over the workgroup in thread order; total gets
// the sum of all. Integer, so exact.
__device__ __forceinline__ unsigned long long sm_block_scan(
    unsigned long long v, unsigned long long* wave_sum,
    unsigned long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
  #pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
  #pragma unroll
  for (int i = 0; i < kSmWaves; ++i) {
    const unsigned long long x = wave_sum[i];
    if (i < wave) before += x;
    all += x;
  }
  __syncthreads();  // wave_sum is free again
  total = all;
  return before + incl - v;
}

// Radix descent over the key, 11 + 11 + 10 bits from the top. With
// MASS = false the histograms count elements and the result is the key
// of the target-th largest element; with MASS = true they hold the mass
// above the threshold thr and the result is the largest key k such that
// the mass of keys >= k reaches target. 1 <= target <= the total.
template <bool MASS, class Row, int IPT>
__device__ uint32_t sm_descend(Row& row, unsigned long long target,
                               uint32_t thr, float vmax, float c,
                               SampleLds& s) {
  const int t = threadIdx.x;
  uint32_t prefix = 0;
  int hi_shift = 32;  // the bits above those of this pass
  #pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int bits = pass == 2 ? 10 : 11;
    const int shift = hi_shift - bits;
    const uint32_t mask = (1u << bits) - 1;
    if constexpr (MASS) {
      s.hist.mass[t] = 0;
      s.hist.mass[t + kSmThreads] = 0;
    } else {
      s.hist.count[t] = 0;
      s.hist.count[t + kSmThreads] = 0;
    }
    __syncthreads();
    row.pin();
    #pragma unroll Row::UNROLL
    for (int e = 0; e < IPT; ++e) {
      const float v = row.value(e);
      const uint32_t key = sm_key(v);
      if ((uint32_t)((uint64_t)key >> hi_shift) != prefix) continue;
      const uint32_t bin = (key >> shift) & mask;
      if constexpr (MASS) {
        const unsigned long long m = sm_mass(v, thr, vmax, c);
        if (m) atomicAdd(&s.hist.mass[bin], m);
      } else {
        atomicAdd(&s.hist.count[bin], 1u);
      }
    }
    __syncthreads();
    // thread t owns bins 2047 - 2t and 2046 - 2t: thread order is the
    // order from the top
    const int top = kSmBins - 1 - 2 * t;
    const unsigned long long h1 =
        MASS ? s.hist.mass[top] : s.hist.count[top];
    const unsigned long long h0 =
        MASS ? s.hist.mass[top - 1] : s.hist.count[top - 1];
    unsigned long long total;
    const unsigned long long above =
        sm_block_scan(h1 + h0, s.wave_sum, total);
    if (above < target && target <= above + h1 + h0) {  // one thread
      const bool in_top = target <= above + h1;
      s.sel = in_top ? top : top - 1;
      s.rem = in_top ? target - above : target - above - h1;
    }
    __syncthreads();
    prefix = (prefix << bits) | s.sel;
    target = s.rem;
    hi_shift = shift;
  }
  return prefix;
}

// The token of the row at rowp, by a whole workgroup of kSmThreads
// threads: exactly one thread calls emit(token); which one depends on the
// row. seed is read once the draw needs it. Every branch that ends the
// call early is uniform over the workgroup.
template <bool BF16, int IPT, class Emit>
__device__ __forceinline__ void sm_sample_row(
    const char* rowp, const SampleCfg& a, const int64_t* seedp,
    uint32_t step_lo, uint32_t step_hi, SampleLds& s, Emit emit) {
  using Row = SampleRow<BF16, IPT>;
  const int t = threadIdx.x;
  // thread 0's range starts this many elements before the row
  const int lead =
      (int)(reinterpret_cast<uintptr_t>(rowp) % Row::GB) / Row::ES;
  const int first = t * IPT - lead;
  Row row;
  row.load(rowp, first, a.V, s.hist.count);

  uint32_t kmax = 0;
  row.pin();
  #pragma unroll Row::UNROLL
  for (int e = 0; e < IPT; ++e) kmax = max(kmax, sm_key(row.value(e)));
  kmax = sm_block_reduce<true>(kmax, s.red);
  if (kmax <= kSmNegInfKey) {  // uniform: nothing above -inf in this row
    if (t == 0) emit((int64_t)0);
    return;
  }
  if (a.greedy) {  // uniform
    // elements outside the row are -inf, below kmax
    uint32_t best = 0xFFFFFFFFu;
    row.pin();
    #pragma unroll Row::UNROLL
    for (int e = IPT - 1; e >= 0; --e)
      if (sm_key(row.value(e)) == kmax) best = (uint32_t)(first + e);
    best = sm_block_reduce<false>(best, s.red);
    if (t == 0) emit((int64_t)best);
    return;
  }
  const float vmax = sm_unkey(kmax);

  uint32_t thr = 0;
  if (a.top_k != 0 && a.top_k < (uint32_t)a.V)
    thr = sm_descend<false, Row, IPT>(row, a.top_k, 0, vmax, a.c, s);
  if (a.top_p < 1.0) {
    unsigned long long mine = 0, M;
    row.pin();
    #pragma unroll Row::UNROLL
    for (int e = 0; e < IPT; ++e)
      mine += sm_mass(row.value(e), thr, vmax, a.c);
    sm_block_scan(mine, s.wave_sum, M);
    // M >= 2^40: the largest element weighs 1
    long long P = llrint(a.top_p * (double)M);
    P = P < 1 ? 1 : (P > (long long)M ? (long long)M : P);
    const uint32_t thr_p = sm_descend<true, Row, IPT>(
        row, (unsigned long long)P, thr, vmax, a.c, s);
    thr = max(thr, thr_p);
  }

  unsigned long long mine = 0, MN;
  row.pin();
  #pragma unroll Row::UNROLL
  for (int e = 0; e < IPT; ++e)
    mine += sm_mass(row.value(e), thr, vmax, a.c);
  const unsigned long long before = sm_block_scan(mine, s.wave_sum, MN);
  const int64_t seed = *seedp;
  const uint32_t x =
      philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32),
                    make_uint4(step_lo, step_hi, 0u, 0u)).x;
  const unsigned long long r =
      __umul64hi(MN, (unsigned long long)x << 32);  // < MN
  if (before <= r && r < before + mine) {  // one thread
    unsigned long long acc = before;
    int tok = -1;
    row.pin();
    #pragma unroll Row::UNROLL
    for (int e = 0; e < IPT; ++e) {
      acc += sm_mass(row.value(e), thr, vmax, a.c);
      if (tok < 0 && acc > r) tok = first + e;  // mass > 0: inside the row
    }
    emit((int64_t)tok);
  }
}

// Elements per thread for rows of V elements that follow each other from
// ptr on, 0 when even 64 do not hold one. The thread ranges start at a
// granule boundary at or before the row, so a row that is not
// granule-aligned needs V plus its lead; the worst row decides.
inline long sm_items_per_thread(uintptr_t ptr, long V, long elem_size) {
  for (long ipt : {1L, 4L, 16L, 64L}) {
    const long gb = std::min(16L, ipt * elem_size);
    const long lead =
        (V * elem_size) % gb == 0 ? (long)(ptr % gb) / elem_size
                                  : gb / elem_size - 1;
    if (V + lead <= kSmThreads * ipt) return ipt;
  }
  return 0;
}

}  // namespace

#pragma clang attribute pop
