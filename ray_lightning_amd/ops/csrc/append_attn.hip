// Multi-token (append) attention over a KV cache, split along the KV
// range, with the T new tokens' k/v appended to the cache in the same
// launch. bf16, head size 64, gfx950.
//
//   o[b, t, h] = softmax(q_t . K^T * scale) . V
//                over positions 0 .. pos[b] + t,          t = 0 .. T-1
//
// Positions 0 .. pos[b]-1 come from the caches [B, H, Tmax, 64];
// position pos[b] + j is new token j and comes from qkv [B, T, 3*H*64]
// (c_attn's output: q, then k, then v per token), never from the cache.
//
// With T query rows the same K/V bytes feed T dot products, so this is an
// MFMA kernel (16x16x32 bf16, the fragment maps of mfma_probe.hip):
//  - grid (KV chunks, query tiles of 16, B*H). Chunk c owns positions
//    [c*128, (c+1)*128) whatever the batch holds, so a row computes the
//    same bits alone and in a batch. Each of the 4 waves owns 32 of them.
//  - S^T = K . Q^T: a K row of 64 bf16 is two A-fragments' worth of
//    16-byte pieces and a Q row two B-fragments', so both go from global
//    memory to the MFMA registers in 16-byte vectors with nothing in
//    between. The C layout leaves one query column per lane (q = lane &
//    15) and 8 of the wave's 32 positions in its registers: the softmax
//    over positions is lane-local plus two cross-lane steps.
//  - O^T = V^T . P^T: P^T is used as the B-fragment exactly where the
//    softmax left it. The MFMA sums over k, so any order of the 32
//    positions serves as long as A uses the same one; lane group g,
//    element i stands for position 16*(i>>2) + 4*g + (i&3), which is the
//    C layout of S^T. No permlane or LDS redistribution of P is needed.
//    The matching V^T A-fragments (8 positions of one column d per lane)
//    are a transposing read: each wave writes its 32 V rows row-major to
//    its own 4 KiB of LDS (16-byte granules XOR-swizzled by row) and reads
//    them back with ds_read_b64_tr_b16, two reads per fragment.
//  - scale * log2 e multiplies the fp32 scores, as in the flash kernels
//    (rounding a pre-scaled Q to bf16 would cost every score 2^-9).
//    P is rounded to bf16 for the MFMA; max, sum and O stay fp32.
//  - the 4 waves' (O, max, sum) are folded in wave order through LDS into
//    one fp32 partial per (query row, chunk): 64 accumulators, max, sum.
//    A second kernel folds a row's partials in chunk order and rounds to
//    bf16 once. No atomics, no flags, no spins: every loop bound is a
//    host number or a constant.
//  - append: a position >= pos[b] is always loaded from qkv, and the
//    workgroup of query tile 0 whose chunk owns that slot stores the
//    16-byte vectors it loaded (every 16 bytes of a chunk's K and of its V
//    are loaded by exactly one lane). Cache reads stay below pos[b], so
//    within the launch every slot has one writer and no reader. Tile 0
//    therefore walks every chunk that holds a new row, also those above
//    its own 16 queries (where the mask leaves it the neutral partial).
//  - a chunk wholly above pos[b] + (last query of the tile) is left at
//    once with the neutral partial (0, -inf, 0); a chunk wholly below
//    pos[b] skips the per-element mask.
//
// fp8 cache (append_attn_partial_kernel<true>, docs/DESIGN.md §21): K and V
// are OCP float8_e4m3fn codes with one fp32 power-of-two scale per (b, h,
// position), [B, H, Tmax]. The geometry, the softmax, the mask, the folds
// and the combine kernel are the ones above; what differs is how operands
// reach the MFMA registers and what the append does:
//  - a cached K row is 64 bytes: lane (row qi, group g) loads one 16-byte
//    vector, codes 16g .. 16g+15, which feeds both MFMAs of the subtile
//    (the first 8 codes are kk = 0). Q's B-fragments load the same
//    permutation, q[16g + 8kk ..];
//  - a wave's 32 V rows are 2 KiB, two 16-byte loads per lane; the 16 codes
//    become two bf16 granules of the same swizzled image;
//  - a load holds one position's codes, so a lane fetches one scale per
//    load (4 bytes, behind the same kv < pos[b] as the codes), and
//    v_cvt_scalef32_pk_bf16_fp8 turns two codes into two scaled bf16: the
//    operands are exactly the dequantized values;
//  - new rows come from qkv as bf16 in the same element order. The 4 lanes
//    that share a row take its absmax, form scale and codes as quantize_kv
//    does (kv_fp8_core.h) and convert the codes back like cached ones, so
//    every tile attends what tile 0 stores: codes as 16-byte vectors, the
//    scale from one lane per row. One writer per byte, and neither codes
//    nor scales at or past pos[b] are read.
//
// pos is read on the device only. A row whose pos[b] lies outside
// [0, max_pos] is inactive: it is replaced by -1 before any use, every
// chunk is then "above" it, no address is formed from it, nothing is
// stored and its output rows are zero.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>
#include <type_traits>

#include "kv_fp8_core.h"

// what a pair of fp8 caches and their scales must be (decode_attn.hip)
void kv_fp8_check(const char* who, const torch::Tensor& k_cache,
                  const torch::Tensor& v_cache, const torch::Tensor& k_scale,
                  const torch::Tensor& v_scale, const at::Device& dev);

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kAaThreads = 256;
constexpr int kAaWaves = kAaThreads / 64;
constexpr int kAaHs = 64;                       // head size
constexpr int kAaQTile = 16;                    // query rows per workgroup
constexpr int kAaChunk = 128;                   // KV positions per workgroup
constexpr int kAaWaveKv = kAaChunk / kAaWaves;  // ... per wave: one MFMA k
constexpr int kAaPartial = kAaHs + 2;           // floats: 64 acc, max, sum
constexpr int kAaOPad = kAaHs + 4;              // LDS row of the wave fold
static_assert(kAaWaveKv == 32, "a wave's positions are one MFMA k block");

// byte offset of (row, 16-byte granule) in a wave's row-major V image:
// rows of 128 bytes, the granule XORed with a row function so that the 16
// rows one transposing read touches spread over the banks. A lane of that
// read addresses 8 bytes inside one granule, so it only has to apply the
// same function.
__device__ __forceinline__ int aa_swz(int row, int granule) {
  return row * 128 + ((granule ^ ((((row >> 1) * 3) ^ (row >> 3)) & 7)) << 4);
}

// V^T A-fragment of columns d = col16 .. col16+15 from a wave's image:
// lane (g = lane >> 4, j = lane & 15) receives column col16 + j of rows
// 4g .. 4g+3 (first read) and 16+4g .. 16+4g+3 (second). Within a group
// of 16 lanes, lanes 4r .. 4r+3 address the four 8-byte pieces of row r
// and lane j receives column j of the four rows (scripts/probe_tr16.py).
__device__ __forceinline__ bf16x8 aa_read_vt(const char* img, int col16,
                                             int lane) {
  const int j = lane & 15;
  const int row = 4 * (lane >> 4) + (j >> 2);
  const int cb = (col16 + 4 * (j & 3)) * 2;  // byte column in the row
  const unsigned base =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)img;
  const unsigned a0 = base + (unsigned)(aa_swz(row, cb >> 4) + (cb & 15));
  const unsigned a1 =
      base + (unsigned)(aa_swz(row + 16, cb >> 4) + (cb & 15));
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  typedef __attribute__((ext_vector_type(4))) unsigned uint4v;
  uint2v r0, r1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n"
      "ds_read_b64_tr_b16 %1, %3\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1)
      : "v"(a0), "v"(a1)
      : "memory");
  return __builtin_bit_cast(bf16x8, uint4v{r0[0], r0[1], r1[0], r1[1]});
}

// 8 e4m3 codes (two words, low byte first) times their position's scale,
// as bf16: v_cvt_scalef32_pk_bf16_fp8 turns two codes into two scaled bf16.
// The scale is a power of two and a code has 4 significant bits, so the
// products are exact: the MFMA operands are dequantize_kv's values.
__device__ __forceinline__ bf16x8 aa_dq8(unsigned w0, unsigned w1,
                                         float scale) {
  const auto a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, false);
  const auto b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, true);
  const auto c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, false);
  const auto d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// FP8: the caches are e4m3 codes with one fp32 scale per position (file
// header, "fp8 cache"); k_scale / v_scale are not read otherwise.
template <bool FP8>
using aa_cache_t = std::conditional_t<FP8, unsigned char, unsigned short>;

template <bool FP8>
__global__ __launch_bounds__(kAaThreads) void append_attn_partial_kernel(
    const unsigned short* __restrict__ qkv,    // [B, T, 3*H*64]
    aa_cache_t<FP8>* __restrict__ k_cache,     // [B, H, Tmax, 64]
    aa_cache_t<FP8>* __restrict__ v_cache,     // [B, H, Tmax, 64]
    float* __restrict__ k_scale,             // [B, H, Tmax]
    float* __restrict__ v_scale,             // [B, H, Tmax]
    const int* __restrict__ pos,             // [B]
    float* __restrict__ ws,                  // [B*H, T, gridDim.x, 66]
    int H, int T, int Tmax, int max_pos, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) char lds_v[kAaWaves][kAaWaveKv * 128];
  __shared__ __attribute__((aligned(16))) float
      lds_o[kAaWaves][kAaQTile][kAaOPad];
  __shared__ float lds_ml[kAaWaves][2][kAaQTile];

  const int chunk = blockIdx.x;
  const int t0 = blockIdx.y * kAaQTile;
  const int bh = blockIdx.z;
  const int b = bh / H;
  const int h = bh - b * H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;    // MFMA lane group
  const int qi = lane & 15;   // this lane's query column / fragment row
  const int n_chunks = gridDim.x;

  // cached tokens of this row; -1 makes every position invalid
  const int pb = pos[b];
  const int p = (pb >= 0 && pb <= max_pos) ? pb : -1;
  // the last position this workgroup loads: its last query's own token,
  // and for tile 0 the last new row, which it has to store
  const int t_last = min(t0 + kAaQTile, T) - 1;
  const int hi = p < 0 ? -1 : p + (t0 == 0 ? T - 1 : t_last);
  const int kv0 = chunk * kAaChunk;
  float* __restrict__ part =
      ws + (((long)bh * T + t0) * n_chunks + chunk) * kAaPartial;
  const long part_row = (long)n_chunks * kAaPartial;  // query row stride

  if (kv0 > hi) {  // uniform: nothing of this row and tile in here
    for (int i = threadIdx.x; i < kAaQTile * kAaPartial; i += kAaThreads) {
      const int q = i / kAaPartial;
      const int e = i - q * kAaPartial;
      if (t0 + q < T) part[q * part_row + e] = e == kAaHs ? -INFINITY : 0.f;
    }
    return;
  }

  // from here 0 <= p <= max_pos and kv0 <= hi <= max_pos + T - 1 < Tmax
  const long C = (long)H * kAaHs;
  const unsigned short* __restrict__ new_rows =
      qkv + (long)b * T * 3 * C + h * kAaHs;  // q of token 0; + C: k, + 2C: v
  const long cache_row = (long)bh * Tmax * kAaHs;
  const bool store = t0 == 0;

  // ---- all loads first: Q^T, K fragments, the V rows -------------------
  // Q^T B-fragments: column qi = query t0 + qi, k = 32*kk + 8*g .. The MFMA
  // sums over k, so any order of the 64 elements serves as long as K uses
  // the same one: over an fp8 cache k = 16*g + 8*kk .. (K loads below).
  bf16x8 qf[2];
  {
    const int t = t0 + qi;
    #pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[kk] = bf16x8{};
      if (t < T)
        qf[kk] = *reinterpret_cast<const bf16x8*>(
            new_rows + (long)t * 3 * C +
            (FP8 ? g * 16 + kk * 8 : kk * 32 + g * 8));
    }
  }
  bf16x8 kraw[2][2];
  if constexpr (!FP8) {
    // K A-fragments: row qi of subtile s is position kv0 + 32*wave + 16*s +
    // qi, k = 32*kk + 8*g ..
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kv = kv0 + wave * kAaWaveKv + s * 16 + qi;
      #pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int e = kk * 32 + g * 8;
        kraw[s][kk] = bf16x8{};
        if (kv <= hi) {
          const unsigned short* a =
              kv < p ? k_cache + cache_row + (long)kv * kAaHs + e
                     : new_rows + (long)(kv - p) * 3 * C + C + e;
          kraw[s][kk] = *reinterpret_cast<const bf16x8*>(a);
        }
      }
    }
    // V rows, row-major: row 8*i + (lane >> 3) of the wave, granule lane & 7
    bf16x8 vraw[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kv = kv0 + wave * kAaWaveKv + i * 8 + (lane >> 3);
      const int e = (lane & 7) * 8;
      vraw[i] = bf16x8{};
      if (kv <= hi) {
        const unsigned short* a =
            kv < p ? v_cache + cache_row + (long)kv * kAaHs + e
                   : new_rows + (long)(kv - p) * 3 * C + 2 * C + e;
        vraw[i] = *reinterpret_cast<const bf16x8*>(a);
      }
    }

    // ---- the append (tile 0), and V into the wave's LDS image ------------
    if (store) {
      #pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kv = kv0 + wave * kAaWaveKv + s * 16 + qi;
        #pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if (kv >= p && kv <= hi)  // p <= kv <= p + T - 1 < Tmax
            *reinterpret_cast<bf16x8*>(k_cache + cache_row +
                                       (long)kv * kAaHs + kk * 32 + g * 8) =
                kraw[s][kk];
      }
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kv = kv0 + wave * kAaWaveKv + i * 8 + (lane >> 3);
        if (kv >= p && kv <= hi)
          *reinterpret_cast<bf16x8*>(v_cache + cache_row + (long)kv * kAaHs +
                                     (lane & 7) * 8) = vraw[i];
      }
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<bf16x8*>(
          lds_v[wave] + aa_swz(i * 8 + (lane >> 3), lane & 7)) = vraw[i];
  } else {
    // ---- fp8 cache: codes and scales in, bf16 operands out ---------------
    // K: row qi of subtile s, one 16-byte load of codes 16*g .. 16*g+15 that
    // feeds both MFMAs of the subtile (the first 8 are kk = 0). V: row
    // 16*i + (lane >> 2) of the wave, codes 16*(lane & 3) .. Every load
    // holds one position's codes, so a lane needs one scale per load, behind
    // the same kv < p as the codes.
    const long scale_row = (long)bh * Tmax;
    const int vrow = lane >> 2, vsub = lane & 3;
    uint4 kc[2], vc[2];
    float ksc[2], vsc[2];
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kv = kv0 + wave * kAaWaveKv + s * 16 + qi;
      kc[s] = uint4{};
      ksc[s] = 1.f;
      if (kv < p) {
        kc[s] = *reinterpret_cast<const uint4*>(k_cache + cache_row +
                                                (long)kv * kAaHs + g * 16);
        ksc[s] = k_scale[scale_row + kv];
      }
    }
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int kv = kv0 + wave * kAaWaveKv + i * 16 + vrow;
      vc[i] = uint4{};
      vsc[i] = 1.f;
      if (kv < p) {
        vc[i] = *reinterpret_cast<const uint4*>(v_cache + cache_row +
                                                (long)kv * kAaHs + vsub * 16);
        vsc[i] = v_scale[scale_row + kv];
      }
    }
    // New rows (uniform: a chunk wholly below p holds none): bf16 from qkv
    // in the same element order, quantized as quantize_kv does. The 4 lanes
    // of a K row are 16 and 32 apart, those of a V row adjacent; every lane
    // runs the absmax shuffles. Every tile attends the codes tile 0 stores.
    if (kv0 + kAaChunk > p) {
      #pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kv = kv0 + wave * kAaWaveKv + s * 16 + qi;
        const bool fresh = kv >= p && kv <= hi;  // p <= kv <= p + T - 1 < Tmax
        uint4 a{}, c{};
        if (fresh) {
          const unsigned short* src =
              new_rows + (long)(kv - p) * 3 * C + C + g * 16;
          a = *reinterpret_cast<const uint4*>(src);
          c = *reinterpret_cast<const uint4*>(src + 8);
        }
        const unsigned amax = kv_row_amax(a, c, 16);
        if (fresh) {
          kc[s] = kv_quant_row(a, c, amax);
          ksc[s] = __builtin_bit_cast(float, kv_scale_bits(amax));
          if (store) {
            *reinterpret_cast<uint4*>(k_cache + cache_row + (long)kv * kAaHs +
                                      g * 16) = kc[s];
            if (g == 0) k_scale[scale_row + kv] = ksc[s];
          }
        }
      }
      #pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kv = kv0 + wave * kAaWaveKv + i * 16 + vrow;
        const bool fresh = kv >= p && kv <= hi;
        uint4 a{}, c{};
        if (fresh) {
          const unsigned short* src =
              new_rows + (long)(kv - p) * 3 * C + 2 * C + vsub * 16;
          a = *reinterpret_cast<const uint4*>(src);
          c = *reinterpret_cast<const uint4*>(src + 8);
        }
        const unsigned amax = kv_row_amax(a, c);
        if (fresh) {
          vc[i] = kv_quant_row(a, c, amax);
          vsc[i] = __builtin_bit_cast(float, kv_scale_bits(amax));
          if (store) {
            *reinterpret_cast<uint4*>(v_cache + cache_row + (long)kv * kAaHs +
                                      vsub * 16) = vc[i];
            if (vsub == 0) v_scale[scale_row + kv] = vsc[i];
          }
        }
      }
    }
    // codes times scale in registers: K into the A-fragments, V as the two
    // bf16 granules 2*vsub, 2*vsub+1 of its row in the wave's image
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      kraw[s][0] = aa_dq8(kc[s].x, kc[s].y, ksc[s]);
      kraw[s][1] = aa_dq8(kc[s].z, kc[s].w, ksc[s]);
    }
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      char* img = lds_v[wave];
      *reinterpret_cast<bf16x8*>(img + aa_swz(i * 16 + vrow, 2 * vsub)) =
          aa_dq8(vc[i].x, vc[i].y, vsc[i]);
      *reinterpret_cast<bf16x8*>(img + aa_swz(i * 16 + vrow, 2 * vsub + 1)) =
          aa_dq8(vc[i].z, vc[i].w, vsc[i]);
    }
  }
  __syncthreads();

  // ---- S^T = K . Q^T: st[s][r] is position kv0 + 32*wave + 16*s + 4*g +
  // r of query column qi
  f32x4 st[2];
  #pragma unroll
  for (int s = 0; s < 2; ++s) {
    st[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        kraw[s][0], qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    st[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kraw[s][1], qf[1],
                                                    st[s], 0, 0, 0);
  }
  #pragma unroll
  for (int s = 0; s < 2; ++s)
    #pragma unroll
    for (int r = 0; r < 4; ++r) st[s][r] *= scale_log2e;
  // query t attends positions <= p + t; a chunk wholly below p holds none
  // above (uniform test). A query column past T attends nothing.
  if (kv0 + kAaChunk > p) {
    const int lim = t0 + qi < T ? p + t0 + qi : -1;
    #pragma unroll
    for (int s = 0; s < 2; ++s)
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kv0 + wave * kAaWaveKv + s * 16 + g * 4 + r > lim)
          st[s][r] = -INFINITY;
  }

  // ---- the wave's softmax over its 32 positions, per query column ------
  float m = -INFINITY;
  #pragma unroll
  for (int s = 0; s < 2; ++s)
    #pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, st[s][r]);
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l = 0.f;
  bf16x8 pf;  // P^T B-fragment: element 4*s + r, see the head of the file
  #pragma unroll
  for (int s = 0; s < 2; ++s)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      // a masked score is -inf and, if all of the column are, m is too
      const float pr = st[s][r] == -INFINITY
                           ? 0.f
                           : __builtin_amdgcn_exp2f(st[s][r] - m);
      l += pr;
      pf[4 * s + r] = (__bf16)pr;
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  // ---- O^T = V^T . P^T: o[n][r] is column d = 16*n + 4*g + r of query qi
  #pragma unroll
  for (int n = 0; n < 4; ++n) {
    const bf16x8 vt = aa_read_vt(lds_v[wave], 16 * n, lane);
    const f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        vt, pf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    *reinterpret_cast<f32x4*>(&lds_o[wave][qi][16 * n + 4 * g]) = o;
  }
  if (g == 0) {
    lds_ml[wave][0][qi] = m;
    lds_ml[wave][1][qi] = l;
  }
  __syncthreads();

  // ---- fold the 4 waves in wave order; thread: query q, columns dd+16*j
  {
    const int q = threadIdx.x >> 4;
    const int dd = threadIdx.x & 15;
    if (t0 + q < T) {
      float M = lds_ml[0][0][q];
      #pragma unroll
      for (int w = 1; w < kAaWaves; ++w) M = fmaxf(M, lds_ml[w][0][q]);
      float f[kAaWaves];
      float L = 0.f;
      #pragma unroll
      for (int w = 0; w < kAaWaves; ++w) {
        const float mw = lds_ml[w][0][q];
        f[w] = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L = fmaf(lds_ml[w][1][q], f[w], L);
      }
      float* __restrict__ pq = part + q * part_row;
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        float A = 0.f;
        #pragma unroll
        for (int w = 0; w < kAaWaves; ++w)
          A = fmaf(lds_o[w][q][dd + 16 * j], f[w], A);
        pq[dd + 16 * j] = A;
      }
      if (dd == 0) {
        pq[kAaHs] = M;
        pq[kAaHs + 1] = L;
      }
    }
  }
}

// o[b, t, h, d] = sum_c acc_c[d] * 2^(m_c - M) / sum_c l_c * 2^(m_c - M),
// the chunks taken in order. A neutral partial adds +0 to both sums, so
// the chunks past a row's own (there because another row of the batch is
// longer) do not change its bits. All partials neutral: zero.
__global__ __launch_bounds__(kAaHs) void append_attn_combine_kernel(
    const float* __restrict__ ws,    // [B*H, T, n_chunks, 66]
    unsigned short* __restrict__ o,  // [B, T, H*64]
    int H, int T, int n_chunks) {
  const int t = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh - b * H;
  const int d = threadIdx.x;
  const float* __restrict__ part =
      ws + ((long)bh * T + t) * n_chunks * kAaPartial;
  float M = -INFINITY;
  for (int c = 0; c < n_chunks; ++c)
    M = fmaxf(M, part[(long)c * kAaPartial + kAaHs]);
  float L = 0.f, A = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const float* pc = part + (long)c * kAaPartial;
    const float mc = pc[kAaHs];
    const float fc = mc == -INFINITY ? 0.f : exp2f(mc - M);
    L = fmaf(pc[kAaHs + 1], fc, L);
    A = fmaf(pc[d], fc, A);
  }
  const float r = L > 0.f ? A / L : 0.f;
  const __hip_bfloat16 ob = __float2bfloat16(r);
  o[((long)b * T + t) * H * kAaHs + h * kAaHs + d] =
      *reinterpret_cast<const unsigned short*>(&ob);
}

}  // namespace

#pragma clang attribute pop

long append_attn_chunk() { return kAaChunk; }

// every check happens here, before anything is allocated or launched
// With scales the caches are fp8.
torch::Tensor append_attn_fwd(torch::Tensor qkv, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor pos,
                              int64_t max_pos, double scale,
                              c10::optional<torch::Tensor> k_scale,
                              c10::optional<torch::Tensor> v_scale) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  const bool fp8 = k_scale.has_value();
  TORCH_CHECK(fp8 == v_scale.has_value(),
              "append_attn_fwd: k_scale and v_scale come together or not "
              "at all");
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
              qkv.dim() == 3 && qkv.is_contiguous(),
              "append_attn_fwd: qkv must be a contiguous bf16 GPU tensor "
              "[B, T, 3*H*64]");
  if (fp8)
    kv_fp8_check("append_attn_fwd", k_cache, v_cache, *k_scale, *v_scale,
                 qkv.device());
  for (const torch::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(fp8 || (c->is_cuda() && c->device() == qkv.device() &&
                        c->scalar_type() == at::kBFloat16 && c->dim() == 4 &&
                        c->is_contiguous() && c->size(3) == kAaHs),
                "append_attn_fwd: k_cache and v_cache must be contiguous "
                "bf16 [B, H, Tmax, 64] on qkv's device");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "append_attn_fwd: k_cache and v_cache differ in shape");
  const int64_t B = qkv.size(0), T = qkv.size(1), H = k_cache.size(1),
                Tmax = k_cache.size(2);
  TORCH_CHECK(k_cache.size(0) == B, "append_attn_fwd: caches hold ",
              k_cache.size(0), " rows, qkv ", B);
  TORCH_CHECK(H > 0 && qkv.size(2) == 3 * H * kAaHs,
              "append_attn_fwd: a qkv token is ", qkv.size(2),
              " wide, the caches' H = ", H, " needs ", 3 * H * kAaHs);
  TORCH_CHECK(pos.is_cuda() && pos.device() == qkv.device() &&
              pos.scalar_type() == at::kInt && pos.dim() == 1 &&
              pos.size(0) == B && pos.is_contiguous(),
              "append_attn_fwd: pos must be a contiguous int32 [B] on "
              "qkv's device");
  TORCH_CHECK(T >= 1, "append_attn_fwd: T = ", T, ", at least one new "
              "token per row is needed");
  TORCH_CHECK(max_pos >= 0 && max_pos + T <= Tmax,
              "append_attn_fwd: max_pos = ", max_pos, " with T = ", T,
              " new tokens does not fit Tmax = ", Tmax);
  TORCH_CHECK(std::isfinite(scale), "append_attn_fwd: scale not finite");
  const int64_t n_chunks = (max_pos + T - 1) / kAaChunk + 1;
  const int64_t q_tiles = (T + kAaQTile - 1) / kAaQTile;
  TORCH_CHECK(qkv.numel() < kLimit && k_cache.numel() < kLimit &&
              B * H * T * n_chunks * kAaPartial < kLimit,
              "append_attn_fwd: 2^31 elements or more in an operand");
  TORCH_CHECK(B * H <= 65535 && T <= 65535,
              "append_attn_fwd: B*H = ", B * H, " or T = ", T,
              " exceeds the grid's extent");
  for (const torch::Tensor* t : {&qkv, &k_cache, &v_cache})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "append_attn_fwd: operands must be 16-byte aligned");

  auto o = torch::empty({B, T, H * kAaHs}, qkv.options());
  if (B == 0) return o;
  auto ws = torch::empty({B * H, T, n_chunks, kAaPartial},
                         qkv.options().dtype(at::kFloat));
  const float scale_log2e = (float)(scale * 1.4426950408889634);
  auto stream = at::hip::getCurrentHIPStream().stream();
  const dim3 grid((unsigned)n_chunks, (unsigned)q_tiles, (unsigned)(B * H));
  if (fp8)
    hipLaunchKernelGGL(
        append_attn_partial_kernel<true>, grid, dim3(kAaThreads), 0, stream,
        reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
        reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
        reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
        k_scale->data_ptr<float>(), v_scale->data_ptr<float>(),
        pos.data_ptr<int>(), ws.data_ptr<float>(), (int)H, (int)T, (int)Tmax,
        (int)max_pos, scale_log2e);
  else
    hipLaunchKernelGGL(
        append_attn_partial_kernel<false>, grid, dim3(kAaThreads), 0, stream,
        reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
        reinterpret_cast<unsigned short*>(k_cache.data_ptr()),
        reinterpret_cast<unsigned short*>(v_cache.data_ptr()),
        (float*)nullptr, (float*)nullptr, pos.data_ptr<int>(),
        ws.data_ptr<float>(), (int)H, (int)T, (int)Tmax, (int)max_pos,
        scale_log2e);
  hipLaunchKernelGGL(append_attn_combine_kernel,
                     dim3((unsigned)T, (unsigned)(B * H)), dim3(kAaHs), 0,
                     stream, ws.data_ptr<float>(),
                     reinterpret_cast<unsigned short*>(o.data_ptr()), (int)H,
                     (int)T, (int)n_chunks);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "append_attn_fwd: ", hipGetErrorString(e));
  return o;
}
