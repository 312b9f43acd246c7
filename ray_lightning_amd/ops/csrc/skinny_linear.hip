// Skinny linear layers of a decode step: y[M, N] = act(h . W[N, K]^T + bias)
// for M <= 64 rows, with the pointwise neighbours of the layer taken into
// the prologue and the epilogue. bf16 in and out, fp32 inside, gfx950.
//
//   h = x                                   (plain)
//   h = LN(x)                               (ln)
//   h = LN(x_new), x_new = bf16(x + res)    (add_ln; x_new is written out)
//   act = identity | tanh-GELU
//
// With M <= 64 the op is one read of W: 2*N*K bytes against 2*M*(N+K) of
// activations. So the kernel is shaped as a stream of W with the matrix
// unit doing the dot products on the side:
//  - swapped operands. v_mfma_f32_16x16x32_bf16 takes 16 rows of W as the
//    A operand (lane: row lane & 15, k = 8 * (lane >> 4) .. + 7 of the
//    32-wide k-step) and 16 rows of x as the B operand (same map), so both
//    are 16-byte loads of 8 consecutive k from row-major memory. The
//    accumulator is y^T: lane (g = lane >> 4, c = lane & 15) holds
//    y[m = c][n = 4g .. 4g+3] of the tile. M up to 64 is 1, 2 or 4 such B
//    tiles (MT); the A fragment of a k-step is loaded once and used for
//    all of them, so W crosses HBM once whatever M is.
//  - a workgroup owns 16 * RT rows of W and all of K. Its WAVES waves
//    split K: with S = K / 32 k-steps, wave w takes the contiguous steps
//    [w * (S / WAVES) + min(w, S % WAVES), + S / WAVES + (w < S % WAVES)),
//    a function of K alone. A wave issues the W loads of U k-steps (8, or
//    4 at MT = 4) before the first MFMA that uses them. The waves' fp32
//    accumulators are folded through LDS in wave order 0 .. WAVES-1, then
//    bias, GELU, one rounding to bf16 and the store.
//  - x is small and L2-resident; its fragments are read from global
//    memory per k-step and never staged whole. With LN every workgroup
//    first computes the M means and reciprocal standard deviations itself
//    (one wave per row, two passes over fp32 of the bf16 row, butterfly
//    sums) into LDS, and then normalises each fragment as it is loaded:
//    h = bf16((v - mean) * rstd * gamma + beta). In add_ln v is
//    bf16(x + res), formed again wherever it is needed; workgroup 0 alone
//    stores it as x_new, which therefore must not alias x or res.
//  - rows m >= M and weight rows n >= N are never read: their fragments
//    are zero. y is stored as 8-byte vectors when N % 4 == 0 and element
//    by element otherwise (rows of y are then only 2-byte aligned).
//  - a row's bits depend on neither M nor the other rows: MFMA columns
//    are independent, the K partition and the fold order are fixed by K,
//    and the statistics of a row are one wave's work.
// No atomics, no flags; every loop bound is a host number or a constant.
//
// fp8 weights (skinny_linear_fp8_kernel): W is OCP float8_e4m3fn [N, K]
// with one fp32 power-of-two scale per row, x and y stay bf16. The same
// kernel shape with three differences:
//  - the A fragment crosses HBM as bytes and becomes bf16 in registers,
//    v_cvt_scalef32_pk_bf16_fp8 with a scale operand of 1.0, one VALU
//    instruction per two elements; every e4m3 value is exact in bf16, so
//    the MFMA is the bf16 one and x is not quantized.
//  - load layout, two candidates kept as template parameters (the choice
//    per shape class is sl_split below, the measurement
//    profiles/skinny_linear_fp8.md). Narrow: a lane loads the 8 bytes of
//    its 8 k of one k-step, the bf16 fragment map at half the width.
//    Wide: a lane loads 16 bytes, k = 16 * (lane >> 4) .. + 15 of a pair
//    of k-steps, and feeds two MFMAs: MFMA h of the pair takes bytes 8h
//    .. 8h + 7, so its lane group g covers k = 16g + 8h .. + 7 of the 64,
//    and the x fragment (and gamma, beta) is read at the same permuted
//    offset; the two MFMAs together cover the pair's 64 k once. A wave
//    with an odd step count ends on one narrow step. UK k-steps of W are
//    in flight per wave and row tile (half that at MT = 4), and steps
//    past the wave's count are skipped, not fed zeros.
//  - the folded fp32 sum is multiplied by scale[n] (exact: a power of
//    two), then bias, GELU and the one rounding. scale[n >= N] is never
//    read.
// The K partition, the fold order and the statistics are the bf16
// kernel's, so a row's bits are again independent of M and of the other
// rows; they differ from the bf16 kernel's on the dequantized weight only
// through the order of the fp32 sums inside a pair.
//
// decode_layer_fwd enqueues one GPT-2 block of a decode step from one
// host call: [add + LN1 + c_attn], decode attention (decode_attn.hip, as
// it stands, over a bf16 cache or, with k_scale / v_scale, an fp8 one),
// [c_proj], [add + LN2 + c_fc + GELU], [c_proj].
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>
#include <tuple>

// defined in decode_attn.hip; with scales the caches are float8_e4m3fn
torch::Tensor decode_attn_fwd(torch::Tensor qkv, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor pos,
                              int64_t max_pos, double scale,
                              c10::optional<torch::Tensor> k_scale,
                              c10::optional<torch::Tensor> v_scale);

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int kSlMaxM = 64;
// K-splitting waves per workgroup, and 16-row weight tiles per workgroup:
// two from kSlWideN weight rows on, where 16-row workgroups are more than
// the machine needs, one below. profiles/skinny_linear.md has the
// alternatives measured. Neither changes a row's bits.
constexpr int kSlWaves = 8;
constexpr int kSlWideN = 4096;

int64_t sl_row_tiles(int64_t N) { return N >= kSlWideN ? 2 : 1; }

// How one launch splits the work. `wide` and `uk` are the fp8 kernel's
// load layout and k-steps in flight and rest at 0 for bf16 weights.
struct SlSplit {
  int64_t waves, row_tiles, wide, uk;
};

// The built-in split. fp8 weights (profiles/skinny_linear_fp8.md): the
// wide loads at every shape, the bf16 kernel's row tiles (four lost at
// every shape and are not built), and 16 k-steps in flight where a wave
// has more than 16 (K >= 4096), 8 below, where a wave of GPT-2-XL's
// K = 1600 has 6 or 7 in all. None of the three changes a row's bits
// except `wide`, which orders the sums inside a pair.
SlSplit sl_split(int64_t N, int64_t K, bool fp8) {
  if (!fp8) return {kSlWaves, sl_row_tiles(N), 0, 0};
  return {kSlWaves, sl_row_tiles(N), 1, K >= 4096 ? 16 : 8};
}

enum { kSlPlain = 0, kSlLn = 1, kSlAddLn = 2 };

struct SlArgs {
  const __bf16* x;      // [M, K]
  const __bf16* res;    // [M, K], add_ln only
  __bf16* x_new;        // [M, K], add_ln only
  const __bf16* w;      // [N, K]
  const __bf16* bias;   // [N] or null
  const float* gamma;   // [K], ln / add_ln
  const float* beta;    // [K], ln / add_ln
  __bf16* y;            // [M, N]
  int M, N, K;
  float eps;
  int gelu;
  const unsigned char* w8;  // [N, K] e4m3 bytes, fp8 kernels only
  const float* scale;       // [N], fp8 kernels only
};

// 8 consecutive elements of the LayerNorm input at element offset `off`,
// as fp32: x, or bf16(x + res) in add_ln
template <int MODE>
__device__ __forceinline__ void sl_row8(const SlArgs& a, long off,
                                        float* f) {
  const bf16x8 xv = *reinterpret_cast<const bf16x8*>(a.x + off);
  if (MODE == kSlAddLn) {
    const bf16x8 rv = *reinterpret_cast<const bf16x8*>(a.res + off);
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = (float)(__bf16)((float)xv[j] + (float)rv[j]);
  } else {
    #pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)xv[j];
  }
}

__device__ __forceinline__ float sl_wave_sum(float v) {
  #pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// LayerNorm statistics of the M rows into LDS: wave w owns rows w,
// w + WAVES, ...; workgroup 0 stores x_new in add_ln. Ends in a barrier.
template <int WAVES, int MODE>
__device__ __forceinline__ void sl_row_stats(const SlArgs& a, int wave,
                                             int lane, float* lds_mean,
                                             float* lds_rstd) {
  if (MODE != kSlPlain) {
    const float inv_k = 1.f / (float)a.K;
    for (int m = wave; m < a.M; m += WAVES) {
      const long row = (long)m * a.K;
      float s = 0.f;
      for (int k = lane * 8; k < a.K; k += 512) {
        float f[8];
        sl_row8<MODE>(a, row + k, f);
        if (MODE == kSlAddLn && blockIdx.x == 0) {
          bf16x8 o;
          #pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (__bf16)f[j];
          *reinterpret_cast<bf16x8*>(a.x_new + row + k) = o;
        }
        #pragma unroll
        for (int j = 0; j < 8; ++j) s += f[j];
      }
      const float mean = sl_wave_sum(s) * inv_k;
      float q = 0.f;
      for (int k = lane * 8; k < a.K; k += 512) {
        float f[8];
        sl_row8<MODE>(a, row + k, f);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = f[j] - mean;
          q = fmaf(d, d, q);
        }
      }
      const float rstd = 1.f / sqrtf(sl_wave_sum(q) * inv_k + a.eps);
      if (lane == 0) {
        lds_mean[m] = mean;
        lds_rstd[m] = rstd;
      }
    }
    __syncthreads();
  }
}

// 8 consecutive gamma and beta
__device__ __forceinline__ void sl_ln_params(const float* gamma,
                                             const float* beta, float* gm,
                                             float* bt) {
  #pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + 4 * h);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(beta + 4 * h);
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      gm[4 * h + j] = gv[j];
      bt[4 * h + j] = bv[j];
    }
  }
}

// the B fragment: 8 consecutive elements of h at element offset off + k
template <int MODE>
__device__ __forceinline__ bf16x8 sl_x_frag(const SlArgs& a, long off, int k,
                                            float mean, float rstd,
                                            const float* gm,
                                            const float* bt) {
  if (MODE == kSlPlain)
    return *reinterpret_cast<const bf16x8*>(a.x + off + k);
  float f[8];
  sl_row8<MODE>(a, off + k, f);
  bf16x8 xf;
  #pragma unroll
  for (int j = 0; j < 8; ++j)
    xf[j] = (__bf16)((f[j] - mean) * rstd * gm[j] + bt[j]);
  return xf;
}

// After the barrier that follows the waves' accumulator stores: the sum
// over the waves in wave order, the row scale (fp8 weights), bias, GELU,
// one rounding to bf16 and the store.
template <int MT, int WAVES, int RT, bool SCALED>
__device__ __forceinline__ void sl_fold_store(
    const SlArgs& a, const float (*lds_red)[RT * MT * 64][4], int n0) {
  constexpr int kItems = RT * MT * 64;
  const bool vec_store = (a.N & 3) == 0;
  for (int i = threadIdx.x; i < kItems; i += WAVES * 64) {
    float v[4];
    #pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = lds_red[0][i][r];
    #pragma unroll
    for (int w = 1; w < WAVES; ++w)
      #pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += lds_red[w][i][r];
    const int l = i & 63;
    const int tile = i >> 6;
    const int rt = tile / MT;
    const int t = tile - rt * MT;
    const int m = 16 * t + (l & 15);
    const int n = n0 + 16 * rt + 4 * (l >> 4);
    if (m >= a.M || n >= a.N) continue;
    bf16x4 o;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float e = v[r];
      if (SCALED && n + r < a.N) e *= a.scale[n + r];
      if (a.bias != nullptr && n + r < a.N) e += (float)a.bias[n + r];
      if (a.gelu) {
        const float u3 = 0.7978845608028654f * (e + 0.044715f * e * e * e);
        e = 0.5f * e * (1.f + tanhf(u3));
      }
      o[r] = (__bf16)e;
    }
    __bf16* dst = a.y + (long)m * a.N + n;
    if (vec_store) {  // N % 4 == 0: n + 3 < N and dst is 8-byte aligned
      *reinterpret_cast<bf16x4*>(dst) = o;
    } else {
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < a.N) dst[r] = o[r];
    }
  }
}

template <int MT, int WAVES, int RT, int MODE>
__global__ __launch_bounds__(WAVES * 64) void skinny_linear_kernel(SlArgs a) {
  constexpr int U = MT == 4 ? 4 : 8;  // k-steps of W in flight per wave
  constexpr int kItems = RT * MT * 64;
  __shared__ float lds_mean[kSlMaxM];
  __shared__ float lds_rstd[kSlMaxM];
  __shared__ __attribute__((aligned(16))) float lds_red[WAVES][kItems][4];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int c = lane & 15;
  const int n0 = blockIdx.x * (16 * RT);

  sl_row_stats<WAVES, MODE>(a, wave, lane, lds_mean, lds_rstd);

  // ---- this wave's k-steps, a function of K alone ----------------------
  const int S = a.K >> 5;
  const int base = S / WAVES, rem = S - base * WAVES;
  const int s_begin = wave * base + min(wave, rem);
  const int s_count = base + (wave < rem ? 1 : 0);

  const __bf16* wrow[RT];
  bool wok[RT];
  #pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int n = n0 + 16 * rt + c;
    wok[rt] = n < a.N;
    wrow[rt] = a.w + (long)(wok[rt] ? n : 0) * a.K + g * 8;
  }
  long xoff[MT];
  bool xok[MT];
  float mean[MT], rstd[MT];
  #pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + c;
    xok[t] = m < a.M;
    xoff[t] = (long)(xok[t] ? m : 0) * a.K + g * 8;
    mean[t] = (MODE != kSlPlain && xok[t]) ? lds_mean[m] : 0.f;
    rstd[t] = (MODE != kSlPlain && xok[t]) ? lds_rstd[m] : 0.f;
  }

  f32x4 acc[RT][MT];
  #pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    #pragma unroll
    for (int t = 0; t < MT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s0 = 0; s0 < s_count; s0 += U) {
    // all W loads of the batch first
    bf16x8 af[U][RT];
    #pragma unroll
    for (int u = 0; u < U; ++u)
      #pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        af[u][rt] = bf16x8{};
        if (s0 + u < s_count && wok[rt])
          af[u][rt] = *reinterpret_cast<const bf16x8*>(
              wrow[rt] + (long)(s_begin + s0 + u) * 32);
      }
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = s0 + u < s_count;  // wave-uniform
      const int k = (s_begin + s0 + u) * 32;
      float gm[8], bt[8];
      if (MODE != kSlPlain && live)
        sl_ln_params(a.gamma + k + g * 8, a.beta + k + g * 8, gm, bt);
      #pragma unroll
      for (int t = 0; t < MT; ++t) {
        bf16x8 xf = bf16x8{};
        if (live && xok[t])
          xf = sl_x_frag<MODE>(a, xoff[t], k, mean[t], rstd[t], gm, bt);
        // a dead step has zero A and zero B fragments
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt)
          acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[u][rt], xf, acc[rt][t], 0, 0, 0);
      }
    }
  }

  // ---- fold the waves in wave order, bias, GELU, round, store -----------
  #pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    #pragma unroll
    for (int t = 0; t < MT; ++t)
      *reinterpret_cast<f32x4*>(lds_red[wave][(rt * MT + t) * 64 + lane]) =
          acc[rt][t];
  __syncthreads();

  sl_fold_store<MT, WAVES, RT, false>(a, lds_red, n0);
}

// 8 e4m3 bytes (k ascending from the low byte of `lo`) as the bf16 A
// fragment. The scale operand is 1.0, so the conversion is exact.
__device__ __forceinline__ bf16x8 sl_fp8x8(unsigned lo, unsigned hi) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, true);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// The fp8-weight kernel (file header). WIDE: 16-byte W loads that feed the
// two MFMAs of a pair of k-steps; else 8-byte loads, one per k-step. UK:
// k-steps of W in flight per wave and row tile.
template <int MT, int RT, int MODE, bool WIDE, int UK>
__global__ __launch_bounds__(kSlWaves * 64) void skinny_linear_fp8_kernel(
    SlArgs a) {
  constexpr int WAVES = kSlWaves;
  constexpr int KS = WIDE ? 2 : 1;                     // k-steps per W load
  constexpr int U = (MT == 4 ? UK / 2 : UK) / KS;      // W loads in flight
  constexpr int kItems = RT * MT * 64;
  __shared__ float lds_mean[kSlMaxM];
  __shared__ float lds_rstd[kSlMaxM];
  __shared__ __attribute__((aligned(16))) float lds_red[WAVES][kItems][4];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4;
  const int c = lane & 15;
  const int n0 = blockIdx.x * (16 * RT);

  sl_row_stats<WAVES, MODE>(a, wave, lane, lds_mean, lds_rstd);

  // this wave's k-steps: the bf16 kernel's partition
  const int S = a.K >> 5;
  const int base = S / WAVES, rem = S - base * WAVES;
  const int s_begin = wave * base + min(wave, rem);
  const int s_count = base + (wave < rem ? 1 : 0);

  const unsigned char* wrow[RT];
  bool wok[RT];
  #pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int n = n0 + 16 * rt + c;
    wok[rt] = n < a.N;
    wrow[rt] = a.w8 + (long)(wok[rt] ? n : 0) * a.K;
  }
  long xoff[MT];
  bool xok[MT];
  float mean[MT], rstd[MT];
  #pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + c;
    xok[t] = m < a.M;
    xoff[t] = (long)(xok[t] ? m : 0) * a.K;
    mean[t] = (MODE != kSlPlain && xok[t]) ? lds_mean[m] : 0.f;
    rstd[t] = (MODE != kSlPlain && xok[t]) ? lds_rstd[m] : 0.f;
  }

  f32x4 acc[RT][MT];
  #pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    #pragma unroll
    for (int t = 0; t < MT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s0 = 0; s0 < s_count; s0 += U * KS) {
    // all W loads of the batch first; load u starts at k-step s0 + u * KS
    // and is a pair when the step after it is the wave's too (all of this
    // is wave-uniform)
    u32x4 af[U][RT];
    #pragma unroll
    for (int u = 0; u < U; ++u)
      #pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int s = s0 + u * KS;
        af[u][rt] = u32x4{0u, 0u, 0u, 0u};
        if (s < s_count && wok[rt]) {
          const unsigned char* p = wrow[rt] + (long)(s_begin + s) * 32;
          if (WIDE && s + 1 < s_count) {
            af[u][rt] = *reinterpret_cast<const u32x4*>(p + g * 16);
          } else {
            const u32x2 v = *reinterpret_cast<const u32x2*>(p + g * 8);
            af[u][rt][0] = v[0];
            af[u][rt][1] = v[1];
          }
        }
      }
    #pragma unroll
    for (int u = 0; u < U; ++u)
      #pragma unroll
      for (int h = 0; h < KS; ++h) {
        const int s = s0 + u * KS;
        if (s + h >= s_count) continue;
        const bool pair = WIDE && s + 1 < s_count;
        // first of this lane's 8 k in this MFMA
        const int k = (s_begin + s) * 32 + (pair ? g * 16 + h * 8 : g * 8);
        float gm[8], bt[8];
        if (MODE != kSlPlain) sl_ln_params(a.gamma + k, a.beta + k, gm, bt);
        bf16x8 wf[RT];
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt)
          wf[rt] = sl_fp8x8(af[u][rt][2 * h], af[u][rt][2 * h + 1]);
        #pragma unroll
        for (int t = 0; t < MT; ++t) {
          bf16x8 xf = bf16x8{};
          if (xok[t])
            xf = sl_x_frag<MODE>(a, xoff[t], k, mean[t], rstd[t], gm, bt);
          #pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[rt], xf, acc[rt][t], 0, 0, 0);
        }
      }
  }

  #pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    #pragma unroll
    for (int t = 0; t < MT; ++t)
      *reinterpret_cast<f32x4*>(lds_red[wave][(rt * MT + t) * 64 + lane]) =
          acc[rt][t];
  __syncthreads();

  sl_fold_store<MT, WAVES, RT, true>(a, lds_red, n0);
}

template <int WAVES, int RT, int MODE>
void sl_launch_mt(const SlArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * RT - 1) / (16 * RT)));
  const dim3 block(WAVES * 64);
  if (a.M <= 16)
    hipLaunchKernelGGL((skinny_linear_kernel<1, WAVES, RT, MODE>), grid,
                       block, 0, stream, a);
  else if (a.M <= 32)
    hipLaunchKernelGGL((skinny_linear_kernel<2, WAVES, RT, MODE>), grid,
                       block, 0, stream, a);
  else
    hipLaunchKernelGGL((skinny_linear_kernel<4, WAVES, RT, MODE>), grid,
                       block, 0, stream, a);
}

template <int WAVES, int RT>
void sl_launch_mode(const SlArgs& a, int mode, hipStream_t stream) {
  if (mode == kSlPlain) sl_launch_mt<WAVES, RT, kSlPlain>(a, stream);
  else if (mode == kSlLn) sl_launch_mt<WAVES, RT, kSlLn>(a, stream);
  else sl_launch_mt<WAVES, RT, kSlAddLn>(a, stream);
}

template <int RT, int MODE, bool WIDE, int UK>
void sl_fp8_launch_mt(const SlArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * RT - 1) / (16 * RT)));
  const dim3 block(kSlWaves * 64);
  if (a.M <= 16)
    hipLaunchKernelGGL((skinny_linear_fp8_kernel<1, RT, MODE, WIDE, UK>),
                       grid, block, 0, stream, a);
  else if (a.M <= 32)
    hipLaunchKernelGGL((skinny_linear_fp8_kernel<2, RT, MODE, WIDE, UK>),
                       grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((skinny_linear_fp8_kernel<4, RT, MODE, WIDE, UK>),
                       grid, block, 0, stream, a);
}

template <int RT, bool WIDE, int UK>
void sl_fp8_launch_mode(const SlArgs& a, int mode, hipStream_t stream) {
  if (mode == kSlPlain) sl_fp8_launch_mt<RT, kSlPlain, WIDE, UK>(a, stream);
  else if (mode == kSlLn) sl_fp8_launch_mt<RT, kSlLn, WIDE, UK>(a, stream);
  else sl_fp8_launch_mt<RT, kSlAddLn, WIDE, UK>(a, stream);
}

// the fp8 splits that are built: both layouts at 1 and 2 row tiles with 8
// and 16 k-steps in flight
bool sl_fp8_launch(const SlArgs& a, int mode, const SlSplit& sp,
                   hipStream_t stream, bool dry) {
  const int64_t rt = sp.row_tiles, uk = sp.uk;
  const bool w = sp.wide != 0;
#define SL_FP8_CASE(RT, WIDE, UK)                                   \
  if (rt == RT && w == WIDE && uk == UK) {                          \
    if (!dry) sl_fp8_launch_mode<RT, WIDE, UK>(a, mode, stream);    \
    return true;                                                    \
  }
  SL_FP8_CASE(1, false, 16) SL_FP8_CASE(2, false, 16)
  SL_FP8_CASE(1, true, 16) SL_FP8_CASE(2, true, 16)
  SL_FP8_CASE(1, false, 8) SL_FP8_CASE(2, false, 8)
  SL_FP8_CASE(1, true, 8) SL_FP8_CASE(2, true, 8)
#undef SL_FP8_CASE
  return false;
}

bool sl_config_known(const SlSplit& sp, bool fp8) {
  if (fp8)
    return sp.waves == kSlWaves && sl_fp8_launch(SlArgs{}, 0, sp, nullptr,
                                                 true);
  return (sp.waves == 4 && sp.row_tiles == 1) ||
         (sp.waves == 8 && sp.row_tiles == 1) ||
         (sp.waves == 8 && sp.row_tiles == 2);
}

using OptTensor = c10::optional<torch::Tensor>;

// Every check of one linear, before anything is allocated or launched.
// The activation is [M, K] bf16 on `dev`; `x` / `residual` are null when
// it is an intermediate this file allocates itself.
void sl_check(const char* who, const torch::Tensor* x,
              const torch::Tensor* residual, bool has_residual, int64_t M,
              int64_t K, c10::Device dev, const torch::Tensor& weight,
              const OptTensor& weight_scale, const OptTensor& bias,
              const OptTensor& ln_weight, const OptTensor& ln_bias,
              double eps) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  auto act_ok = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == dev &&
           t.scalar_type() == at::kBFloat16 && t.dim() == 2 &&
           t.is_contiguous() && t.size(0) == M && t.size(1) == K &&
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  if (x != nullptr)
    TORCH_CHECK(act_ok(*x), who, ": x must be a contiguous, 16-byte "
                "aligned bf16 GPU tensor [M, K]");
  // bf16 weights, or float8_e4m3fn ones together with their row scales
  const bool fp8 = weight_scale.has_value();
  TORCH_CHECK(weight.is_cuda() && weight.device() == dev &&
              weight.scalar_type() ==
                  (fp8 ? at::kFloat8_e4m3fn : at::kBFloat16) &&
              weight.dim() == 2 && weight.is_contiguous() &&
              reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
              who, ": weight must be a contiguous, 16-byte aligned [N, K] "
              "on x's device, bf16, or float8_e4m3fn with a weight_scale");
  const int64_t N = weight.size(0);
  if (fp8)
    TORCH_CHECK(weight_scale->is_cuda() && weight_scale->device() == dev &&
                weight_scale->scalar_type() == at::kFloat &&
                weight_scale->dim() == 1 && weight_scale->is_contiguous() &&
                weight_scale->size(0) == N,
                who, ": weight_scale must be a contiguous fp32 [N = ", N,
                "] on x's device");
  TORCH_CHECK(weight.size(1) == K, who, ": weight is [", N, ", ",
              weight.size(1), "], x has K = ", K);
  TORCH_CHECK(M >= 0 && M <= kSlMaxM, who, ": M = ", M,
              " rows, the kernel takes at most ", kSlMaxM);
  TORCH_CHECK(N >= 1, who, ": weight has no rows");
  TORCH_CHECK(K >= 32 && K % 32 == 0, who, ": K = ", K,
              " must be a positive multiple of 32");
  if (bias.has_value())
    TORCH_CHECK(bias->is_cuda() && bias->device() == dev &&
                bias->scalar_type() == at::kBFloat16 && bias->dim() == 1 &&
                bias->is_contiguous() && bias->size(0) == N,
                who, ": bias must be a contiguous bf16 [N = ", N,
                "] on x's device");
  TORCH_CHECK(ln_weight.has_value() == ln_bias.has_value(), who,
              ": ln_weight and ln_bias come together or not at all");
  if (ln_weight.has_value())
    for (const torch::Tensor* p : {&*ln_weight, &*ln_bias})
      TORCH_CHECK(p->is_cuda() && p->device() == dev &&
                  p->scalar_type() == at::kFloat && p->dim() == 1 &&
                  p->is_contiguous() && p->size(0) == K &&
                  reinterpret_cast<uintptr_t>(p->data_ptr()) % 16 == 0,
                  who, ": ln_weight and ln_bias must be contiguous fp32 "
                  "[K = ", K, "] on x's device");
  TORCH_CHECK(!has_residual || ln_weight.has_value(), who,
              ": a residual is only taken together with LayerNorm");
  if (residual != nullptr)
    TORCH_CHECK(act_ok(*residual), who, ": residual must be a contiguous, "
                "16-byte aligned bf16 [M, K] on x's device");
  TORCH_CHECK(std::isfinite(eps) && eps >= 0.0, who, ": eps = ", eps);
  TORCH_CHECK(N * K < kLimit && kSlMaxM * N < kLimit && kSlMaxM * K < kLimit,
              who, ": 2^31 elements or more in an operand");
  // the smallest workgroup owns 16 rows: the grid's x extent is N / 16
  TORCH_CHECK((N + 15) / 16 < kLimit, who, ": N exceeds the grid");
}

// one launch; operands were checked by sl_check
void sl_run(const torch::Tensor& x, const torch::Tensor* residual,
            torch::Tensor* x_new, const torch::Tensor& weight,
            const OptTensor& weight_scale, const OptTensor& bias,
            const OptTensor& ln_weight, const OptTensor& ln_bias, double eps,
            bool gelu, torch::Tensor& y, const SlSplit& sp) {
  const bool fp8 = weight_scale.has_value();
  SlArgs a;
  a.x = reinterpret_cast<const __bf16*>(x.data_ptr());
  a.res = residual ? reinterpret_cast<const __bf16*>(residual->data_ptr())
                   : nullptr;
  a.x_new = x_new ? reinterpret_cast<__bf16*>(x_new->data_ptr()) : nullptr;
  a.w = fp8 ? nullptr : reinterpret_cast<const __bf16*>(weight.data_ptr());
  a.w8 = fp8 ? reinterpret_cast<const unsigned char*>(weight.data_ptr())
             : nullptr;
  a.scale = fp8 ? weight_scale->data_ptr<float>() : nullptr;
  a.bias = bias.has_value()
               ? reinterpret_cast<const __bf16*>(bias->data_ptr())
               : nullptr;
  a.gamma = ln_weight.has_value() ? ln_weight->data_ptr<float>() : nullptr;
  a.beta = ln_bias.has_value() ? ln_bias->data_ptr<float>() : nullptr;
  a.y = reinterpret_cast<__bf16*>(y.data_ptr());
  a.M = (int)x.size(0);
  a.N = (int)weight.size(0);
  a.K = (int)x.size(1);
  a.eps = (float)eps;
  a.gelu = gelu ? 1 : 0;
  const int mode = residual ? kSlAddLn
                            : (ln_weight.has_value() ? kSlLn : kSlPlain);
  auto stream = at::hip::getCurrentHIPStream().stream();
  if (fp8) sl_fp8_launch(a, mode, sp, stream, false);
  else if (sp.waves == 4) sl_launch_mode<4, 1>(a, mode, stream);
  else if (sp.row_tiles == 1) sl_launch_mode<8, 1>(a, mode, stream);
  else sl_launch_mode<8, 2>(a, mode, stream);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "skinny_linear_fwd: ", hipGetErrorString(e));
}

std::tuple<torch::Tensor, OptTensor> sl_checked(
    torch::Tensor x, torch::Tensor weight, OptTensor weight_scale,
    OptTensor bias, OptTensor residual, OptTensor ln_weight,
    OptTensor ln_bias, double eps, bool gelu, const SlSplit& sp) {
  const char* who = "skinny_linear_fwd";
  TORCH_CHECK(x.dim() == 2, who, ": x must be [M, K]");
  TORCH_CHECK(sl_config_known(sp, weight_scale.has_value()), who,
              ": no kernel for waves = ", sp.waves, ", row_tiles = ",
              sp.row_tiles, ", wide = ", sp.wide, ", uk = ", sp.uk);
  sl_check(who, &x, residual.has_value() ? &*residual : nullptr,
           residual.has_value(), x.size(0), x.size(1), x.device(), weight,
           weight_scale, bias, ln_weight, ln_bias, eps);
  const int64_t M = x.size(0), N = weight.size(0), K = x.size(1);
  auto y = torch::empty({M, N}, x.options());
  OptTensor x_new;
  if (residual.has_value()) x_new = torch::empty({M, K}, x.options());
  if (M == 0) return {y, x_new};
  sl_run(x, residual.has_value() ? &*residual : nullptr,
         x_new.has_value() ? &*x_new : nullptr, weight, weight_scale, bias,
         ln_weight, ln_bias, eps, gelu, y, sp);
  return {y, x_new};
}

}  // namespace

#pragma clang attribute pop

// `weight` is bf16, or float8_e4m3fn with `weight_scale` fp32 [N]
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> skinny_linear_fwd(
    torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> bias,
    c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> ln_weight,
    c10::optional<torch::Tensor> ln_bias, double eps, bool gelu,
    c10::optional<torch::Tensor> weight_scale) {
  return sl_checked(x, weight, weight_scale, bias, residual, ln_weight,
                    ln_bias, eps, gelu,
                    sl_split(weight.dim() == 2 ? weight.size(0) : 0,
                             weight.dim() == 2 ? weight.size(1) : 0,
                             weight_scale.has_value()));
}

// the same op at another work split, for the measurement that picks
// kSlWaves / kSlWideN (scripts/bench_skinny_linear.py); nothing else
// calls it
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> skinny_linear_fwd_at(
    torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> bias,
    c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> ln_weight,
    c10::optional<torch::Tensor> ln_bias, double eps, bool gelu,
    int64_t waves, int64_t row_tiles) {
  return sl_checked(x, weight, c10::nullopt, bias, residual, ln_weight,
                    ln_bias, eps, gelu, SlSplit{waves, row_tiles, 0, 0});
}

// and the fp8-weight op at (row_tiles, wide, uk), for the measurement that
// picks sl_split's fp8 branch
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
skinny_linear_fp8_fwd_at(
    torch::Tensor x, torch::Tensor weight, torch::Tensor weight_scale,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> ln_weight,
    c10::optional<torch::Tensor> ln_bias, double eps, bool gelu,
    int64_t row_tiles, bool wide, int64_t uk) {
  return sl_checked(x, weight, weight_scale, bias, residual, ln_weight,
                    ln_bias, eps, gelu,
                    SlSplit{kSlWaves, row_tiles, wide ? 1 : 0, uk});
}

namespace {

// One GPT-2 block of a decode step. `x` is the previous block's MLP output
// and `residual` the residual stream it is added to; the first block has
// no pending output: `x` is the stream itself and `residual` is absent.
// Returns (x_mid, mlp_out): the stream after the attention sublayer and
// the MLP's output, the pair the next block (or the final LayerNorm)
// takes as (residual, x). The four weights are bf16 when `scales` is null
// and float8_e4m3fn with scales[0 .. 3] otherwise; the caches are bf16, or
// float8_e4m3fn when k_scale / v_scale [B, H, Tmax] are given.
std::tuple<torch::Tensor, torch::Tensor> sl_decode_layer(
    const char* who, torch::Tensor x, c10::optional<torch::Tensor> residual,
    torch::Tensor ln1_w, torch::Tensor ln1_b, torch::Tensor attn_w,
    torch::Tensor attn_b, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor pos, int64_t max_pos, double scale, torch::Tensor proj_w,
    torch::Tensor proj_b, torch::Tensor ln2_w, torch::Tensor ln2_b,
    torch::Tensor fc_w, torch::Tensor fc_b, torch::Tensor mlp_proj_w,
    torch::Tensor mlp_proj_b, double eps, const torch::Tensor* scales,
    c10::optional<torch::Tensor> k_scale,
    c10::optional<torch::Tensor> v_scale) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  const bool fp8 = scales != nullptr;
  const bool kv_fp8 = k_scale.has_value();
  OptTensor as, ps, fs, ms;
  if (fp8) as = scales[0], ps = scales[1], fs = scales[2], ms = scales[3];
  // ---- every check first ------------------------------------------------
  TORCH_CHECK(x.dim() == 2, who, ": x must be [B, C]");
  const int64_t B = x.size(0), C = x.size(1);
  const auto dev = x.device();
  TORCH_CHECK(B >= 1, who, ": no rows");
  const OptTensor none;
  sl_check("decode_layer_fwd (c_attn)", &x,
           residual.has_value() ? &*residual : nullptr, residual.has_value(),
           B, C, dev, attn_w, as, attn_b, ln1_w, ln1_b, eps);
  TORCH_CHECK(attn_w.size(0) == 3 * C, who, ": c_attn has ", attn_w.size(0),
              " rows, 3*C = ", 3 * C);
  sl_check("decode_layer_fwd (attn c_proj)", nullptr, nullptr, false, B, C,
           dev, proj_w, ps, proj_b, none, none, eps);
  TORCH_CHECK(proj_w.size(0) == C, who, ": the attention c_proj must be "
              "[C, C]");
  sl_check("decode_layer_fwd (c_fc)", nullptr, nullptr, true, B, C, dev,
           fc_w, fs, fc_b, ln2_w, ln2_b, eps);
  const int64_t F = fc_w.size(0);
  sl_check("decode_layer_fwd (mlp c_proj)", nullptr, nullptr, false, B, F,
           dev, mlp_proj_w, ms, mlp_proj_b, none, none, eps);
  TORCH_CHECK(mlp_proj_w.size(0) == C, who, ": the MLP c_proj must be "
              "[C, F]");
  // what decode_attn_fwd will ask of its operands
  TORCH_CHECK(kv_fp8 == v_scale.has_value(), who,
              ": k_scale and v_scale come together or not at all");
  for (const torch::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(c->is_cuda() && c->device() == dev &&
                c->scalar_type() ==
                    (kv_fp8 ? at::kFloat8_e4m3fn : at::kBFloat16) &&
                c->dim() == 4 && c->is_contiguous() && c->size(3) == 64 &&
                reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0,
                who, ": k_cache and v_cache must be contiguous, 16-byte "
                "aligned [B, H, Tmax, 64] on x's device, bf16 or, with "
                "scales, float8_e4m3fn");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), who,
              ": k_cache and v_cache differ in shape");
  if (kv_fp8)
    for (const torch::Tensor* sc : {&*k_scale, &*v_scale})
      TORCH_CHECK(sc->is_cuda() && sc->device() == dev &&
                  sc->scalar_type() == at::kFloat && sc->dim() == 3 &&
                  sc->is_contiguous() && sc->size(0) == k_cache.size(0) &&
                  sc->size(1) == k_cache.size(1) &&
                  sc->size(2) == k_cache.size(2),
                  who, ": k_scale and v_scale must be contiguous fp32 "
                  "[B, H, Tmax] on x's device");
  const int64_t H = k_cache.size(1), Tmax = k_cache.size(2);
  TORCH_CHECK(k_cache.size(0) == B && H > 0 && H * 64 == C, who,
              ": the caches must be [B = ", B, ", H = C / 64 = ", C / 64,
              ", Tmax, 64]");
  TORCH_CHECK(pos.is_cuda() && pos.device() == dev &&
              pos.scalar_type() == at::kInt && pos.dim() == 1 &&
              pos.size(0) == B && pos.is_contiguous(),
              who, ": pos must be a contiguous int32 [B] on x's device");
  TORCH_CHECK(max_pos >= 0 && max_pos < Tmax, who, ": max_pos = ", max_pos,
              " is outside [0, Tmax) = [0, ", Tmax, ")");
  TORCH_CHECK(std::isfinite(scale), who, ": scale not finite");
  TORCH_CHECK(k_cache.numel() < kLimit && B * H <= 65535 &&
              B * H * (Tmax / 64 + 1) * 66 < kLimit,
              who, ": the caches exceed the attention kernel's limits");

  // ---- then the launches, on the current stream --------------------------
  const auto opt = x.options();
  const OptTensor ab(attn_b), pb(proj_b), fb(fc_b), mb(mlp_proj_b);
  const OptTensor l1w(ln1_w), l1b(ln1_b), l2w(ln2_w), l2b(ln2_b);
  auto qkv = torch::empty({B, 3 * C}, opt);
  torch::Tensor x1 = x;
  if (residual.has_value()) x1 = torch::empty({B, C}, opt);
  sl_run(x, residual.has_value() ? &*residual : nullptr,
         residual.has_value() ? &x1 : nullptr, attn_w, as, ab, l1w, l1b, eps,
         false, qkv, sl_split(3 * C, C, fp8));
  auto att = decode_attn_fwd(qkv, k_cache, v_cache, pos, max_pos, scale,
                             k_scale, v_scale);
  auto att_out = torch::empty({B, C}, opt);
  sl_run(att, nullptr, nullptr, proj_w, ps, pb, none, none, eps, false,
         att_out, sl_split(C, C, fp8));
  auto hid = torch::empty({B, F}, opt);
  auto x_mid = torch::empty({B, C}, opt);
  sl_run(att_out, &x1, &x_mid, fc_w, fs, fb, l2w, l2b, eps, true, hid,
         sl_split(F, C, fp8));
  auto mlp_out = torch::empty({B, C}, opt);
  sl_run(hid, nullptr, nullptr, mlp_proj_w, ms, mb, none, none, eps, false,
         mlp_out, sl_split(C, F, fp8));
  return {x_mid, mlp_out};
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor> decode_layer_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> residual,
    torch::Tensor ln1_w, torch::Tensor ln1_b, torch::Tensor attn_w,
    torch::Tensor attn_b, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor pos, int64_t max_pos, double scale, torch::Tensor proj_w,
    torch::Tensor proj_b, torch::Tensor ln2_w, torch::Tensor ln2_b,
    torch::Tensor fc_w, torch::Tensor fc_b, torch::Tensor mlp_proj_w,
    torch::Tensor mlp_proj_b, double eps,
    c10::optional<torch::Tensor> k_scale,
    c10::optional<torch::Tensor> v_scale) {
  return sl_decode_layer("decode_layer_fwd", x, residual, ln1_w, ln1_b,
                         attn_w, attn_b, k_cache, v_cache, pos, max_pos,
                         scale, proj_w, proj_b, ln2_w, ln2_b, fc_w, fc_b,
                         mlp_proj_w, mlp_proj_b, eps, nullptr, k_scale,
                         v_scale);
}

// the same block with float8_e4m3fn weights and their fp32 row scales
std::tuple<torch::Tensor, torch::Tensor> decode_layer_fp8_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> residual,
    torch::Tensor ln1_w, torch::Tensor ln1_b, torch::Tensor attn_w,
    torch::Tensor attn_s, torch::Tensor attn_b, torch::Tensor k_cache,
    torch::Tensor v_cache, torch::Tensor pos, int64_t max_pos, double scale,
    torch::Tensor proj_w, torch::Tensor proj_s, torch::Tensor proj_b,
    torch::Tensor ln2_w, torch::Tensor ln2_b, torch::Tensor fc_w,
    torch::Tensor fc_s, torch::Tensor fc_b, torch::Tensor mlp_proj_w,
    torch::Tensor mlp_proj_s, torch::Tensor mlp_proj_b, double eps,
    c10::optional<torch::Tensor> k_scale,
    c10::optional<torch::Tensor> v_scale) {
  const torch::Tensor scales[4] = {attn_s, proj_s, fc_s, mlp_proj_s};
  return sl_decode_layer("decode_layer_fp8_fwd", x, residual, ln1_w, ln1_b,
                         attn_w, attn_b, k_cache, v_cache, pos, max_pos,
                         scale, proj_w, proj_b, ln2_w, ln2_b, fc_w, fc_b,
                         mlp_proj_w, mlp_proj_b, eps, scales, k_scale,
                         v_scale);
}
