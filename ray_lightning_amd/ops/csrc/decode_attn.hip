// Single-token (decode) attention over a KV cache, split along the KV
// range, with the new token's k/v appended to the cache in the same
// launch. bf16, head size 64, gfx950.
//
//   o[b, h] = softmax(q . K^T * scale) . V   over positions 0 .. pos[b]
//
// Positions 0 .. pos[b]-1 come from the caches [B, H, Tmax, 64];
// position pos[b] is the new token and comes from qkv [B, 3*H*64] (the
// c_attn output row: q, then k, then v), never from the cache.
//
// One query row per head leaves nothing for an MFMA tile to do: the work
// is one read of the cached K and V rows, 2 * pos * 128 bytes per (b, h).
// So the kernel is shaped as a streaming read:
//  - grid (KV chunks, B*H). Chunk c owns positions [c*CHUNK, (c+1)*CHUNK)
//    clipped to pos[b]; the partition is a function of the position alone,
//    so a row computes the same bits whatever batch it sits in.
//  - a 64-wide bf16 row is 8 lanes x 16 bytes, so one load instruction of
//    a wave covers 8 consecutive positions (1 KiB contiguous) and one of
//    the workgroup (4 waves) 32. Every K and V load of a thread is issued
//    before the first use; nothing goes through LDS on the way in.
//  - q lives in registers as fp32 (pre-multiplied by scale * log2 e);
//    dot products, the softmax and P.V accumulate in fp32.
//  - each workgroup writes one fp32 partial (64 accumulators, running max,
//    sum) to a workspace; a chunk that is empty for its row writes the
//    neutral partial (0, -inf, 0). A second kernel folds a row's partials
//    in chunk order and rounds to bf16 once. No atomics, no flags, no
//    spins: every loop bound is a host number (max_pos) or a constant.
//  - the thread group that meets position pos[b] takes that k/v row from
//    qkv and stores the same 16-byte vectors to the caches at slot pos[b].
//    It is the only reader and the only writer of that slot in the launch.
//
// fp8 cache (decode_attn_fp8_partial_kernel, docs/DESIGN.md §20): K and V
// are OCP float8_e4m3fn codes with one fp32 power-of-two scale per (b, h,
// position), [B, H, Tmax]. The same grid, chunks, partials and combine,
// with a data path of its own:
//  - a 64-byte row is 4 lanes x 16 bytes: one wave load covers 16
//    positions (1 KiB contiguous) and one of the workgroup (2 waves) 32, q
//    is 16 fp32 per lane, a dot product folds over 4 lanes;
//  - a chunk's 128 K scales and 128 V scales are loaded once per workgroup
//    into LDS; codes become fp32 in registers (v_cvt_scalef32_pk_f32_fp8,
//    scale operand 1.0); the scales multiply the score and the probability,
//    once per position: s = (q . kq) * ks[t], acc += (p * vs[t]) * vq;
//  - the group that owns slot pos[b] quantizes the new k / v row (absmax
//    over its 4 lanes, kv_fp8_core.h), stores codes and scales, and attends
//    the codes it stored, so the output is attention over the updated cache;
//  - the 16 groups of a wave are folded by a halving exchange, 15 shuffles
//    for the 16 accumulators of a lane.
// kv_cache_fill_kernel quantizes the prefill's k and v into the caches.
//
// pos is read on the device only. A row whose pos[b] lies outside
// [0, max_pos] is inactive: all its positions are invalid, so it forms no
// address from pos[b], stores nothing and its output is zero.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>

#include "kv_fp8_core.h"

namespace {

using OptTensor = c10::optional<torch::Tensor>;

constexpr int kDaThreads = 256;
constexpr int kDaWaves = kDaThreads / 64;
constexpr int kDaHs = 64;              // head size
constexpr int kDaStep = kDaWaves * 8;  // positions per workgroup load
constexpr int kDaPartial = kDaHs + 2;  // floats: 64 acc, max, sum
// KV positions per workgroup; profiles/gpt2_generate.md has the
// alternatives measured
constexpr int kDaChunk = 128;
// waves per workgroup of the fp8-cache kernel: 2 (four K and four V loads
// in flight per thread) beat 4 at five of the six points measured in
// profiles/kv_fp8.md
constexpr int kDaFp8Waves = 2;

__device__ __forceinline__ void bf16x8_to_float(const uint4& raw,
                                                float* f) {
  const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

template <int CHUNK>
__global__ __launch_bounds__(kDaThreads) void decode_attn_partial_kernel(
    const unsigned short* __restrict__ qkv,  // [B, 3*H*64]
    unsigned short* __restrict__ k_cache,    // [B, H, Tmax, 64]
    unsigned short* __restrict__ v_cache,    // [B, H, Tmax, 64]
    const int* __restrict__ pos,             // [B]
    float* __restrict__ ws,                  // [B*H, gridDim.x, 66]
    int H, int Tmax, int max_pos, float scale_log2e) {
  constexpr int U = CHUNK / kDaStep;  // positions per thread group
  static_assert(CHUNK % kDaStep == 0, "CHUNK must be a multiple of 32");
  __shared__ float lds_acc[kDaWaves][kDaHs];
  __shared__ float lds_ml[kDaWaves][2];

  const int chunk = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh - b * H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane & 7;   // which 16 bytes of the 128-byte row
  const int grp = lane >> 3;  // which of the wave's 8 positions

  // the last position this row attends; -1 makes every position invalid
  const int pb = pos[b];
  const int last = (pb >= 0 && pb <= max_pos) ? pb : -1;
  float* __restrict__ part =
      ws + ((long)bh * gridDim.x + chunk) * kDaPartial;

  if (chunk * CHUNK > last) {  // uniform: nothing of this row in here
    if (threadIdx.x < kDaHs) part[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) {
      part[kDaHs] = -INFINITY;
      part[kDaHs + 1] = 0.f;
    }
    return;
  }

  const long C = (long)H * kDaHs;
  const unsigned short* __restrict__ qrow =
      qkv + (long)b * 3 * C + h * kDaHs + sub * 8;
  const long cache_row = (long)bh * Tmax * kDaHs + sub * 8;

  // all loads first: q, then this thread's U rows of K and of V
  const uint4 qraw = *reinterpret_cast<const uint4*>(qrow);
  uint4 kraw[U], vraw[U];
  const int p0 = chunk * CHUNK + wave * 8 + grp;
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * kDaStep;
    kraw[u] = uint4{0, 0, 0, 0};
    vraw[u] = uint4{0, 0, 0, 0};
    if (p <= last) {  // 0 <= p <= last <= max_pos < Tmax
      const long off = cache_row + (long)p * kDaHs;
      const unsigned short* ka = p == last ? qrow + C : k_cache + off;
      const unsigned short* va = p == last ? qrow + 2 * C : v_cache + off;
      kraw[u] = *reinterpret_cast<const uint4*>(ka);
      vraw[u] = *reinterpret_cast<const uint4*>(va);
    }
  }

  float q[8];
  bf16x8_to_float(qraw, q);
  #pragma unroll
  for (int j = 0; j < 8; ++j) q[j] *= scale_log2e;

  // scores (in units of log 2), and the append of the new row
  float s[U];
  float m = -INFINITY;
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * kDaStep;
    if (p == last) {
      const long off = cache_row + (long)p * kDaHs;
      *reinterpret_cast<uint4*>(k_cache + off) = kraw[u];
      *reinterpret_cast<uint4*>(v_cache + off) = vraw[u];
    }
    float kf[8];
    bf16x8_to_float(kraw[u], kf);
    float d = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; ++j) d = fmaf(q[j], kf[j], d);
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    s[u] = p <= last ? d : -INFINITY;
    m = fmaxf(m, s[u]);
  }

  float l = 0.f;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    // an invalid position has s = -inf and, if all are, m = -inf too
    const float pr = s[u] == -INFINITY ? 0.f : exp2f(s[u] - m);
    float vf[8];
    bf16x8_to_float(vraw[u], vf);
    l += pr;
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(pr, vf[j], acc[j]);
  }

  // fold the wave's 8 thread groups: common max, rescale, butterfly sum
  float mw = m;
  mw = fmaxf(mw, __shfl_xor(mw, 8, 64));
  mw = fmaxf(mw, __shfl_xor(mw, 16, 64));
  mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
  const float f = m == -INFINITY ? 0.f : exp2f(m - mw);
  l *= f;
  #pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= f;
  #pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    l += __shfl_xor(l, off, 64);
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (grp == 0) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) lds_acc[wave][sub * 8 + j] = acc[j];
    if (sub == 0) {
      lds_ml[wave][0] = mw;
      lds_ml[wave][1] = l;
    }
  }
  __syncthreads();

  // fold the 4 waves in wave order; thread t owns accumulator t
  if (threadIdx.x < kDaHs) {
    float M = lds_ml[0][0];
    #pragma unroll
    for (int w = 1; w < kDaWaves; ++w) M = fmaxf(M, lds_ml[w][0]);
    float L = 0.f, A = 0.f;
    #pragma unroll
    for (int w = 0; w < kDaWaves; ++w) {
      const float mwv = lds_ml[w][0];
      const float fw = mwv == -INFINITY ? 0.f : exp2f(mwv - M);
      L = fmaf(lds_ml[w][1], fw, L);
      A = fmaf(lds_acc[w][threadIdx.x], fw, A);
    }
    part[threadIdx.x] = A;
    if (threadIdx.x == 0) {
      part[kDaHs] = M;
      part[kDaHs + 1] = L;
    }
  }
}

// o[bh, t] = sum_c acc_c[t] * 2^(m_c - M) / sum_c l_c * 2^(m_c - M), the
// chunks taken in order. A neutral partial adds +0 to both sums, so the
// chunks past a row's pos (there because another row of the batch is
// longer) do not change its bits. All partials neutral: zero.
__global__ __launch_bounds__(kDaHs) void decode_attn_combine_kernel(
    const float* __restrict__ ws,         // [B*H, n_chunks, 66]
    unsigned short* __restrict__ o,       // [B*H, 64]
    int n_chunks) {
  const int bh = blockIdx.x;
  const int t = threadIdx.x;
  const float* __restrict__ part = ws + (long)bh * n_chunks * kDaPartial;
  float M = -INFINITY;
  for (int c = 0; c < n_chunks; ++c)
    M = fmaxf(M, part[(long)c * kDaPartial + kDaHs]);
  float L = 0.f, A = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const float* pc = part + (long)c * kDaPartial;
    const float mc = pc[kDaHs];
    const float fc = mc == -INFINITY ? 0.f : exp2f(mc - M);
    L = fmaf(pc[kDaHs + 1], fc, L);
    A = fmaf(pc[t], fc, A);
  }
  const float r = L > 0.f ? A / L : 0.f;
  const __hip_bfloat16 ob = __float2bfloat16(r);
  o[(long)bh * kDaHs + t] = *reinterpret_cast<const unsigned short*>(&ob);
}

// ---- fp8 KV cache (file header, "fp8 cache") ----------------------------

// 4 e4m3 bytes of `w` as fp32, low byte first. The scale operand is 1.0, so
// the conversion is exact.
__device__ __forceinline__ void fp8x4_to_float(unsigned w, float* f) {
  const auto lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, 1.f, false);
  const auto hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, 1.f, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

__device__ __forceinline__ void fp8x16_to_float(const uint4& raw, float* f) {
  fp8x4_to_float(raw.x, f);
  fp8x4_to_float(raw.y, f + 4);
  fp8x4_to_float(raw.z, f + 8);
  fp8x4_to_float(raw.w, f + 12);
}

// kv_amax16, kv_row_amax and kv_quant_row (a row of 64 bf16 on 4 adjacent
// lanes) are in kv_fp8_core.h.

// The partial kernel over an fp8 cache: the grid, the chunk partition, the
// partial's layout and the folds are decode_attn_partial_kernel's, so the
// combine kernel serves both. Its own: a 64-byte row is 4 lanes x 16
// bytes, one wave load covers 16 positions; the chunk's scales go through
// LDS once; the 16 groups of a wave are folded by a halving exchange that
// leaves every lane one accumulator.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void decode_attn_fp8_partial_kernel(
    const unsigned short* __restrict__ qkv,  // [B, 3*H*64] bf16
    unsigned char* __restrict__ k_cache,     // [B, H, Tmax, 64] e4m3
    unsigned char* __restrict__ v_cache,     // [B, H, Tmax, 64] e4m3
    float* __restrict__ k_scale,             // [B, H, Tmax]
    float* __restrict__ v_scale,             // [B, H, Tmax]
    const int* __restrict__ pos,             // [B]
    float* __restrict__ ws,                  // [B*H, gridDim.x, 66]
    int H, int Tmax, int max_pos, float scale_log2e) {
  constexpr int THREADS = WAVES * 64;
  constexpr int STEP = WAVES * 16;     // positions per workgroup load
  constexpr int U = kDaChunk / STEP;   // positions per thread group
  static_assert(kDaChunk % STEP == 0, "the chunk must be whole loads");
  __shared__ float lds_scale[2][kDaChunk];  // K, then V
  __shared__ float lds_acc[WAVES][kDaHs];
  __shared__ float lds_ml[WAVES][2];

  const int chunk = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh - b * H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane & 3;   // which 16 bytes of the 64-byte row
  const int grp = lane >> 2;  // which of the wave's 16 positions

  const int pb = pos[b];
  const int last = (pb >= 0 && pb <= max_pos) ? pb : -1;
  float* __restrict__ part =
      ws + ((long)bh * gridDim.x + chunk) * kDaPartial;
  const int c0 = chunk * kDaChunk;

  if (c0 > last) {  // uniform: nothing of this row in here
    if (threadIdx.x < kDaHs) part[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) {
      part[kDaHs] = -INFINITY;
      part[kDaHs + 1] = 0.f;
    }
    return;
  }

  // the scales of the chunk's cached positions, one load per workgroup;
  // slot `last` and above are not read (0 <= p < last <= max_pos < Tmax)
  const long scale_row = (long)bh * Tmax;
  for (int i = threadIdx.x; i < 2 * kDaChunk; i += THREADS) {
    const int which = i / kDaChunk, p = c0 + (i & (kDaChunk - 1));
    float s = 0.f;
    if (p < last) s = (which ? v_scale : k_scale)[scale_row + p];
    lds_scale[which][i & (kDaChunk - 1)] = s;
  }

  const long C = (long)H * kDaHs;
  const unsigned short* __restrict__ qrow =
      qkv + (long)b * 3 * C + h * kDaHs + sub * 16;
  const long cache_row = (long)bh * Tmax * kDaHs + sub * 16;  // bytes

  // all loads first: q, this thread's U rows of K and of V, and the new
  // row's k and v (bf16, from qkv) in the group that meets slot `last`
  const uint4 q0 = *reinterpret_cast<const uint4*>(qrow);
  const uint4 q1 = *reinterpret_cast<const uint4*>(qrow + 8);
  uint4 kraw[U], vraw[U];
  const int p0 = c0 + wave * 16 + grp;
  bool own = false;
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * STEP;
    kraw[u] = uint4{0, 0, 0, 0};
    vraw[u] = uint4{0, 0, 0, 0};
    own = own || p == last;
    if (p < last) {
      const long off = cache_row + (long)p * kDaHs;
      kraw[u] = *reinterpret_cast<const uint4*>(k_cache + off);
      vraw[u] = *reinterpret_cast<const uint4*>(v_cache + off);
    }
  }
  uint4 nk0 = uint4{0, 0, 0, 0}, nk1 = nk0, nv0 = nk0, nv1 = nk0;
  if (own) {
    nk0 = *reinterpret_cast<const uint4*>(qrow + C);
    nk1 = *reinterpret_cast<const uint4*>(qrow + C + 8);
    nv0 = *reinterpret_cast<const uint4*>(qrow + 2 * C);
    nv1 = *reinterpret_cast<const uint4*>(qrow + 2 * C + 8);
  }

  // quantize the new row (every lane runs the absmax shuffles, the owning
  // group alone the conversion) and store it: one writer, and no reader,
  // of slot `last`
  const unsigned nk_amax = kv_row_amax(nk0, nk1);
  const unsigned nv_amax = kv_row_amax(nv0, nv1);
  const unsigned nks_bits = kv_scale_bits(nk_amax);
  const unsigned nvs_bits = kv_scale_bits(nv_amax);
  uint4 nkq = uint4{0, 0, 0, 0}, nvq = nkq;
  if (own) {
    nkq = kv_quant_row(nk0, nk1, nk_amax);
    nvq = kv_quant_row(nv0, nv1, nv_amax);
    const long off = cache_row + (long)last * kDaHs;
    *reinterpret_cast<uint4*>(k_cache + off) = nkq;
    *reinterpret_cast<uint4*>(v_cache + off) = nvq;
    if (sub == 0) {
      k_scale[scale_row + last] = __uint_as_float(nks_bits);
      v_scale[scale_row + last] = __uint_as_float(nvs_bits);
    }
  }
  __syncthreads();  // lds_scale

  float q[16];
  bf16x8_to_float(q0, q);
  bf16x8_to_float(q1, q + 8);
  #pragma unroll
  for (int j = 0; j < 16; ++j) q[j] *= scale_log2e;

  // scores (in units of log 2): (q . codes) * scale[p], exact in the scale
  float s[U], vs[U];
  float m = -INFINITY;
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * STEP;
    const int i = p - c0;
    float ks = lds_scale[0][i];
    vs[u] = lds_scale[1][i];
    if (p == last) {  // attends what it stored: the dequantized new row
      kraw[u] = nkq;
      vraw[u] = nvq;
      ks = __uint_as_float(nks_bits);
      vs[u] = __uint_as_float(nvs_bits);
    }
    float kf[16];
    fp8x16_to_float(kraw[u], kf);
    float d = 0.f;
    #pragma unroll
    for (int j = 0; j < 16; ++j) d = fmaf(q[j], kf[j], d);
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    s[u] = p <= last ? d * ks : -INFINITY;
    m = fmaxf(m, s[u]);
  }

  float l = 0.f;
  float acc[16];
  #pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  #pragma unroll
  for (int u = 0; u < U; ++u) {
    const float pr = s[u] == -INFINITY ? 0.f : exp2f(s[u] - m);
    float vf[16];
    fp8x16_to_float(vraw[u], vf);
    l += pr;
    const float pv = pr * vs[u];
    #pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = fmaf(pv, vf[j], acc[j]);
  }

  // fold the wave's 16 thread groups: common max, rescale, then a halving
  // exchange over lane bits 2 .. 5. At each step a lane keeps one half of
  // its accumulators and adds the partner's copy of that half, so after 4
  // steps (8 + 4 + 2 + 1 shuffles) lane (grp, sub) holds the wave's sum of
  // accumulator sub*16 + bitrev4(grp). The tree is fixed: same bits always.
  float mw = m;
  #pragma unroll
  for (int off = 4; off < 64; off <<= 1)
    mw = fmaxf(mw, __shfl_xor(mw, off, 64));
  const float f = m == -INFINITY ? 0.f : exp2f(m - mw);
  l *= f;
  #pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] *= f;
  #pragma unroll
  for (int off = 4; off < 64; off <<= 1) l += __shfl_xor(l, off, 64);
  int idx = sub * 16;
  #pragma unroll
  for (int n = 8, off = 4; n >= 1; n >>= 1, off <<= 1) {
    const bool up = lane & off;
    #pragma unroll
    for (int j = 0; j < n; ++j) {
      const float keep = up ? acc[j + n] : acc[j];
      const float send = up ? acc[j] : acc[j + n];
      acc[j] = keep + __shfl_xor(send, off, 64);
    }
    idx += up ? n : 0;
  }
  lds_acc[wave][idx] = acc[0];
  if (lane == 0) {
    lds_ml[wave][0] = mw;
    lds_ml[wave][1] = l;
  }
  __syncthreads();

  // fold the waves in wave order; thread t owns accumulator t
  if (threadIdx.x < kDaHs) {
    float M = lds_ml[0][0];
    #pragma unroll
    for (int w = 1; w < WAVES; ++w) M = fmaxf(M, lds_ml[w][0]);
    float L = 0.f, A = 0.f;
    #pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float mwv = lds_ml[w][0];
      const float fw = mwv == -INFINITY ? 0.f : exp2f(mwv - M);
      L = fmaf(lds_ml[w][1], fw, L);
      A = fmaf(lds_acc[w][threadIdx.x], fw, A);
    }
    part[threadIdx.x] = A;
    if (threadIdx.x == 0) {
      part[kDaHs] = M;
      part[kDaHs + 1] = L;
    }
  }
}

// The prefill's cache fill: k and v of qkv [B, T, 3*H*64] quantized into
// slots 0 .. T-1. One 4-lane group per (k | v, b, h, t) row, t fastest: a
// wave reads 16 full 128-byte lines and writes 1 KiB of codes and 64 bytes
// of scales, both contiguous. Slots >= T are not touched.
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(
    const unsigned short* __restrict__ qkv,
    unsigned char* __restrict__ k_cache, unsigned char* __restrict__ v_cache,
    float* __restrict__ k_scale, float* __restrict__ v_scale, int B, int T,
    int H, int Tmax) {
  const long rows = (long)B * H * T;  // per cache
  const long r = ((long)blockIdx.x * 256 + threadIdx.x) >> 2;
  const int sub = threadIdx.x & 3;
  const bool live = r < 2 * rows;  // uniform over the 4 lanes of a row
  const int which = live && r >= rows;
  const long rr = live ? r - which * rows : 0;
  const int t = (int)(rr % T);
  const long bhi = rr / T;  // b * H + h
  const int b = (int)(bhi / H);
  const int h = (int)(bhi - (long)b * H);
  const long C = (long)H * kDaHs;
  uint4 a = uint4{0, 0, 0, 0}, c = a;
  if (live) {
    const unsigned short* src = qkv + ((long)b * T + t) * 3 * C +
                                (1 + which) * C + h * kDaHs + sub * 16;
    a = *reinterpret_cast<const uint4*>(src);
    c = *reinterpret_cast<const uint4*>(src + 8);
  }
  const unsigned amax = kv_row_amax(a, c);
  if (live) {
    const uint4 codes = kv_quant_row(a, c, amax);
    const unsigned scale_bits = kv_scale_bits(amax);
    const long slot = bhi * Tmax + t;
    *reinterpret_cast<uint4*>((which ? v_cache : k_cache) + slot * kDaHs +
                              sub * 16) = codes;
    if (sub == 0)
      (which ? v_scale : k_scale)[slot] = __uint_as_float(scale_bits);
  }
}

template <int WAVES>
void da_fp8_launch(const torch::Tensor& qkv, torch::Tensor& k_cache,
                   torch::Tensor& v_cache, torch::Tensor& k_scale,
                   torch::Tensor& v_scale, const torch::Tensor& pos,
                   torch::Tensor& ws, torch::Tensor& o, int B, int H,
                   int Tmax, int max_pos, int n_chunks, float scale_log2e) {
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(
      (decode_attn_fp8_partial_kernel<WAVES>), dim3(n_chunks, B * H),
      dim3(WAVES * 64), 0, stream,
      reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
      reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
      reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
      k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
      pos.data_ptr<int>(), ws.data_ptr<float>(), H, Tmax, max_pos,
      scale_log2e);
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(B * H), dim3(kDaHs),
                     0, stream, ws.data_ptr<float>(),
                     reinterpret_cast<unsigned short*>(o.data_ptr()),
                     n_chunks);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "decode_attn_fwd: ", hipGetErrorString(e));
}

}  // namespace

// what a pair of fp8 caches and their scales must be, for `who`; also the
// check of append_attn.hip
void kv_fp8_check(const char* who, const torch::Tensor& k_cache,
                  const torch::Tensor& v_cache, const torch::Tensor& k_scale,
                  const torch::Tensor& v_scale, const at::Device& dev) {
  for (const torch::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(c->is_cuda() && c->device() == dev &&
                c->scalar_type() == at::kFloat8_e4m3fn && c->dim() == 4 &&
                c->is_contiguous() && c->size(3) == kDaHs,
                who, ": with scales, k_cache and v_cache must be contiguous "
                "float8_e4m3fn [B, H, Tmax, 64] on qkv's device");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), who,
              ": k_cache and v_cache differ in shape");
  for (const torch::Tensor* s : {&k_scale, &v_scale})
    TORCH_CHECK(s->is_cuda() && s->device() == dev &&
                s->scalar_type() == at::kFloat && s->dim() == 3 &&
                s->is_contiguous() && s->size(0) == k_cache.size(0) &&
                s->size(1) == k_cache.size(1) &&
                s->size(2) == k_cache.size(2),
                who, ": k_scale and v_scale must be contiguous fp32 "
                "[B, H, Tmax] on qkv's device");
}

namespace {

template <int CHUNK>
void da_launch(const torch::Tensor& qkv, torch::Tensor& k_cache,
               torch::Tensor& v_cache, const torch::Tensor& pos,
               torch::Tensor& ws, torch::Tensor& o, int B, int H, int Tmax,
               int max_pos, int n_chunks, float scale_log2e) {
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(
      (decode_attn_partial_kernel<CHUNK>), dim3(n_chunks, B * H),
      dim3(kDaThreads), 0, stream,
      reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
      reinterpret_cast<unsigned short*>(k_cache.data_ptr()),
      reinterpret_cast<unsigned short*>(v_cache.data_ptr()),
      pos.data_ptr<int>(), ws.data_ptr<float>(), H, Tmax, max_pos,
      scale_log2e);
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(B * H), dim3(kDaHs),
                     0, stream, ws.data_ptr<float>(),
                     reinterpret_cast<unsigned short*>(o.data_ptr()),
                     n_chunks);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "decode_attn_fwd: ", hipGetErrorString(e));
}

// every check happens here, before anything is allocated or launched
// With scales the caches are fp8 and `waves` picks the fp8 kernel's
// workgroup size.
torch::Tensor da_checked(torch::Tensor qkv, torch::Tensor k_cache,
                         torch::Tensor v_cache, torch::Tensor pos,
                         int64_t max_pos, double scale, int64_t chunk,
                         OptTensor k_scale = OptTensor(),
                         OptTensor v_scale = OptTensor(),
                         int64_t waves = kDaFp8Waves) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  const bool fp8 = k_scale.has_value();
  TORCH_CHECK(fp8 == v_scale.has_value(),
              "decode_attn_fwd: k_scale and v_scale come together or not "
              "at all");
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
              qkv.dim() == 2 && qkv.is_contiguous(),
              "decode_attn_fwd: qkv must be a contiguous bf16 GPU tensor "
              "[B, 3*H*64]");
  if (fp8) {
    kv_fp8_check("decode_attn_fwd", k_cache, v_cache, *k_scale, *v_scale,
                 qkv.device());
    TORCH_CHECK(chunk == kDaChunk && (waves == 2 || waves == 4),
                "decode_attn_fwd: the fp8 kernel has chunk = ", kDaChunk,
                " and 2 or 4 waves");
  }
  for (const torch::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(fp8 || (c->is_cuda() && c->device() == qkv.device() &&
                        c->scalar_type() == at::kBFloat16 && c->dim() == 4 &&
                        c->is_contiguous() && c->size(3) == kDaHs),
                "decode_attn_fwd: k_cache and v_cache must be contiguous "
                "bf16 [B, H, Tmax, 64] on qkv's device");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(),
              "decode_attn_fwd: k_cache and v_cache differ in shape");
  const int64_t B = qkv.size(0), H = k_cache.size(1),
                Tmax = k_cache.size(2);
  TORCH_CHECK(k_cache.size(0) == B,
              "decode_attn_fwd: caches hold ", k_cache.size(0),
              " rows, qkv ", B);
  TORCH_CHECK(H > 0 && qkv.size(1) == 3 * H * kDaHs,
              "decode_attn_fwd: qkv row is ", qkv.size(1),
              " wide, the caches' H = ", H, " needs ", 3 * H * kDaHs);
  TORCH_CHECK(pos.is_cuda() && pos.device() == qkv.device() &&
              pos.scalar_type() == at::kInt && pos.dim() == 1 &&
              pos.size(0) == B && pos.is_contiguous(),
              "decode_attn_fwd: pos must be a contiguous int32 [B] on "
              "qkv's device");
  TORCH_CHECK(max_pos >= 0 && max_pos < Tmax,
              "decode_attn_fwd: max_pos = ", max_pos,
              " is outside [0, Tmax) = [0, ", Tmax, ")");
  TORCH_CHECK(std::isfinite(scale), "decode_attn_fwd: scale not finite");
  TORCH_CHECK(chunk == 64 || chunk == 128 || chunk == 256,
              "decode_attn_fwd: no kernel for chunk = ", chunk);
  const int64_t n_chunks = max_pos / chunk + 1;
  TORCH_CHECK(qkv.numel() < kLimit && k_cache.numel() < kLimit &&
              B * H * n_chunks * kDaPartial < kLimit,
              "decode_attn_fwd: 2^31 elements or more in an operand");
  TORCH_CHECK(B * H <= 65535, "decode_attn_fwd: B*H = ", B * H,
              " exceeds the grid's y extent");
  for (const torch::Tensor* t : {&qkv, &k_cache, &v_cache})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "decode_attn_fwd: operands must be 16-byte aligned");

  auto o = torch::empty({B, H * kDaHs}, qkv.options());
  if (B == 0) return o;
  auto ws = torch::empty({B * H, n_chunks, kDaPartial},
                         qkv.options().dtype(at::kFloat));
  const float scale_log2e = (float)(scale * 1.4426950408889634);
  if (fp8) {
    if (waves == 2)
      da_fp8_launch<2>(qkv, k_cache, v_cache, *k_scale, *v_scale, pos, ws, o,
                       (int)B, (int)H, (int)Tmax, (int)max_pos,
                       (int)n_chunks, scale_log2e);
    else
      da_fp8_launch<4>(qkv, k_cache, v_cache, *k_scale, *v_scale, pos, ws, o,
                       (int)B, (int)H, (int)Tmax, (int)max_pos,
                       (int)n_chunks, scale_log2e);
    return o;
  }
#define DA_CASE(CH)                                                     \
  if (chunk == CH)                                                      \
    da_launch<CH>(qkv, k_cache, v_cache, pos, ws, o, (int)B, (int)H,    \
                  (int)Tmax, (int)max_pos, (int)n_chunks, scale_log2e);
  DA_CASE(64)
  DA_CASE(128)
  DA_CASE(256)
#undef DA_CASE
  return o;
}

}  // namespace

long decode_attn_chunk() { return kDaChunk; }

torch::Tensor decode_attn_fwd(torch::Tensor qkv, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor pos,
                              int64_t max_pos, double scale,
                              c10::optional<torch::Tensor> k_scale,
                              c10::optional<torch::Tensor> v_scale) {
  return da_checked(qkv, k_cache, v_cache, pos, max_pos, scale, kDaChunk,
                    k_scale, v_scale);
}

// the fp8-cache op at 2 or 4 waves per workgroup, for the measurement that
// picks kDaFp8Waves (scripts/bench_kv_fp8.py); nothing else calls it
torch::Tensor decode_attn_fp8_fwd_at(torch::Tensor qkv,
                                     torch::Tensor k_cache,
                                     torch::Tensor v_cache,
                                     torch::Tensor k_scale,
                                     torch::Tensor v_scale,
                                     torch::Tensor pos, int64_t max_pos,
                                     double scale, int64_t waves) {
  return da_checked(qkv, k_cache, v_cache, pos, max_pos, scale, kDaChunk,
                    k_scale, v_scale, waves);
}

// k and v of the prefill's qkv [B, T, 3*H*64], quantized into slots
// 0 .. T-1 of fp8 caches and their scales; every check before the launch
void kv_cache_fill(torch::Tensor qkv, torch::Tensor k_cache,
                   torch::Tensor v_cache, torch::Tensor k_scale,
                   torch::Tensor v_scale) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
              qkv.dim() == 3 && qkv.is_contiguous(),
              "kv_cache_fill: qkv must be a contiguous bf16 GPU tensor "
              "[B, T, 3*H*64]");
  kv_fp8_check("kv_cache_fill", k_cache, v_cache, k_scale, v_scale,
               qkv.device());
  const int64_t B = qkv.size(0), T = qkv.size(1), H = k_cache.size(1),
                Tmax = k_cache.size(2);
  TORCH_CHECK(k_cache.size(0) == B && H > 0 &&
              qkv.size(2) == 3 * H * kDaHs,
              "kv_cache_fill: qkv is ", qkv.sizes(), ", the caches ",
              k_cache.sizes());
  TORCH_CHECK(T <= Tmax, "kv_cache_fill: T = ", T, " exceeds Tmax = ", Tmax);
  TORCH_CHECK(qkv.numel() < kLimit && k_cache.numel() < kLimit,
              "kv_cache_fill: 2^31 elements or more in an operand");
  for (const torch::Tensor* t : {&qkv, &k_cache, &v_cache})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "kv_cache_fill: operands must be 16-byte aligned");
  if (B == 0 || T == 0) return;
  const int64_t groups = 2 * B * H * T;  // 4 lanes each, 64 per workgroup
  hipLaunchKernelGGL(
      kv_cache_fill_kernel, dim3((unsigned)((groups + 63) / 64)), dim3(256),
      0, at::hip::getCurrentHIPStream().stream(),
      reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
      reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
      reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
      k_scale.data_ptr<float>(), v_scale.data_ptr<float>(), (int)B, (int)T,
      (int)H, (int)Tmax);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "kv_cache_fill: ", hipGetErrorString(e));
}

// the same op at another chunk size, for the measurement that picks
// kDaChunk (scripts/bench_decode_attn.py); nothing else calls it
torch::Tensor decode_attn_fwd_at_chunk(torch::Tensor qkv,
                                       torch::Tensor k_cache,
                                       torch::Tensor v_cache,
                                       torch::Tensor pos, int64_t max_pos,
                                       double scale, int64_t chunk) {
  return da_checked(qkv, k_cache, v_cache, pos, max_pos, scale, chunk);
}
