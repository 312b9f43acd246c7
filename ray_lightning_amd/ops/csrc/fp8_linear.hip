// Linear layers over fp8 weights at any row count:
//   y[M, N] = act(x[M, K] . dequant(W)[N, K]^T + bias)
// x, bias and y bf16; W OCP float8_e4m3fn with one fp32 power-of-two scale
// per row (ops/skinny_linear.py: quantize_weight); act the identity or
// tanh-GELU; fp32 inside, one rounding to bf16 at the end. gfx950.
//
// Where skinny_linear.hip streams W past at most 64 rows of x, this is a
// tiled LDS GEMM: prefill, extend and every other call with many rows reuse
// each weight tile BM times, so the tile is staged once and shared.
//  - a workgroup of 256 threads, four waves in 2 x 2, owns a BM x BN tile
//    of y and all of K; the tile is 128 x 128, or 64 x 64 where the larger
//    grid would leave most of the machine idle (fl_tile, a function of M
//    and N). A wave owns a quarter: TM x TN tiles of
//    v_mfma_f32_16x16x32_bf16 with fp32 accumulators in registers (4 x 4,
//    64 VGPRs, in the large tile). As in skinny_linear.hip the operands are
//    swapped: 16 rows of W are the A fragment, 16 rows of x the B fragment
//    (lane: row lane & 15, k = 8 * (lane >> 4) .. + 7 of the 32), so both
//    are one 16-byte read of 8 consecutive k, and lane (g = lane >> 4,
//    c = lane & 15) holds y[m = c][A rows 4g .. 4g + 3].
//  - K is walked in steps of 64 (two MFMA k-steps); K % 64 == 32 ends in a
//    half step whose second k-step is skipped and never loaded.
//  - x tile: global -> registers -> LDS in 16-byte pieces of 8 bf16.
//    W tile: 16 codes per lane and piece, converted to bf16 in registers,
//    v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact), and stored to LDS as
//    bf16: once per workgroup, where reading fp8 from LDS would repeat the
//    converts in both waves that share the column block and in every one
//    of a wave's TM reuses of the fragment.
//  - the LDS image of either tile is rows of 64 bf16 = eight 16-byte
//    chunks, chunk j of row r kept at chunk j ^ swz(r). swz is chosen so
//    that the 16 rows of a fragment read (same j) fall into 16 different
//    16-byte columns of the 256 bytes that the 64 banks span, parity of
//    the row picking the half: swz = (r >> 1) & 7 for x, whose fragment
//    reads rows c. For W the A rows of a pair of 16-row tiles are
//    permuted, A row i of half h being W row 8 * (i >> 2) + 4 * h + (i & 3)
//    of the 32, so that a lane holds y[m][8g .. 8g + 7] across the pair
//    and stores 16 bytes; those rows differ in bits 0, 1, 3, 4 and swz =
//    ((r >> 1) & 1) | (((r >> 3) & 3) << 1).
//  - register-prefetch double buffering: the global loads of step s + 1
//    are issued before the MFMAs of step s and written, converted, to the
//    other LDS buffer after them; one barrier per step. Two buffers of
//    (BM + BN) x 64 bf16 are 64 KB at 128 x 128: two workgroups per CU.
//  - epilogue: acc * scale[n] (exact, a power of two), + bias, GELU, one
//    rounding; 16-byte stores when N % 8 == 0, else element by element.
//    Rows m >= M and n >= N are never read (their pieces are zeros) and
//    never written.
//  - a row's bits depend on neither M, the other rows, nor the tile: every
//    y[m][n] is one accumulator lane that walks K in the same order, MFMA
//    columns are independent, K is never split, there are no atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int kFlThreads = 256;
constexpr int kFlBK = 64;  // k per step: two MFMA k-steps, 8 chunks a row
// the 128 x 128 tile from this many of its workgroups on: measured on
// GPT-2-XL's shapes, the 64 x 64 tile still wins by 2 % at 304 of them
// and loses by 2 % at 400 (profiles/fp8_linear.md)
constexpr int64_t kFlBigTiles = 352;

struct FlArgs {
  const __bf16* x;           // [M, K]
  const unsigned char* w8;   // [N, K] e4m3 bytes
  const float* scale;        // [N]
  const __bf16* bias;        // [N] or null
  __bf16* y;                 // [M, N]
  int M, N, K;
  int gelu;
};

// 8 e4m3 bytes (k ascending from the low byte of `lo`) as 8 bf16. The
// scale operand is 1.0, so the conversion is exact.
__device__ __forceinline__ bf16x8 fl_fp8x8(unsigned lo, unsigned hi) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, true);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

__device__ __forceinline__ int fl_swz_x(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int fl_swz_w(int r) {
  return ((r >> 1) & 1) | (((r >> 3) & 3) << 1);
}

template <int BM, int BN>
__global__ __launch_bounds__(kFlThreads) void fp8_linear_kernel(FlArgs a) {
  constexpr int TM = BM / 32;        // 16-row x tiles per wave
  constexpr int TP = BN / 64;        // pairs of 16-row W tiles per wave
  constexpr int XP = BM / 32;        // x pieces per thread and step
  constexpr int WP = BN / 64;        // W pieces (16 codes) per thread and step
  // [buffer][row][chunk]: BM rows of x, then BN rows of W
  __shared__ __attribute__((aligned(16))) bf16x8 lds[2][BM + BN][8];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g = lane >> 4;
  const int c = lane & 15;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int wm = (wave >> 1) * (BM / 2);   // this wave's quarter
  const int wn = (wave & 1) * (BN / 2);

  // ---- what this thread moves per step ----------------------------------
  // x piece i: row xr[i] of the tile, chunk xc = tid & 7 (8 bf16)
  // W piece i: row wr[i] of the tile, codes 16 * wj .. + 15, wj = tid & 3
  const int xc = tid & 7, wj = tid & 3;
  const __bf16* xsrc[XP];
  const unsigned char* wsrc[WP];
  int xr[XP], wr[WP];
  #pragma unroll
  for (int i = 0; i < XP; ++i) {
    xr[i] = (tid >> 3) + 32 * i;
    const int m = m0 + xr[i];
    xsrc[i] = m < a.M ? a.x + (long)m * a.K + 8 * xc : nullptr;
  }
  #pragma unroll
  for (int i = 0; i < WP; ++i) {
    wr[i] = (tid >> 2) + 64 * i;
    const int n = n0 + wr[i];
    wsrc[i] = n < a.N ? a.w8 + (long)n * a.K + 16 * wj : nullptr;
  }

  bf16x8 xreg[XP];
  u32x4 wreg[WP];
  // pieces of the step at k0; a piece at or past K, or of a row past M or
  // N, is zeros and is not read (K % 32 == 0: a piece is whole or absent)
  auto load = [&](int k0) {
    #pragma unroll
    for (int i = 0; i < XP; ++i) {
      xreg[i] = bf16x8{};
      if (xsrc[i] != nullptr && k0 + 8 * xc < a.K)
        xreg[i] = *reinterpret_cast<const bf16x8*>(xsrc[i] + k0);
    }
    #pragma unroll
    for (int i = 0; i < WP; ++i) {
      wreg[i] = u32x4{0u, 0u, 0u, 0u};
      if (wsrc[i] != nullptr && k0 + 16 * wj < a.K)
        wreg[i] = *reinterpret_cast<const u32x4*>(wsrc[i] + k0);
    }
  };
  auto stage = [&](int buf) {
    #pragma unroll
    for (int i = 0; i < XP; ++i)
      lds[buf][xr[i]][xc ^ fl_swz_x(xr[i])] = xreg[i];
    #pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int s = fl_swz_w(wr[i]);
      lds[buf][BM + wr[i]][(2 * wj) ^ s] = fl_fp8x8(wreg[i][0], wreg[i][1]);
      lds[buf][BM + wr[i]][(2 * wj + 1) ^ s] =
          fl_fp8x8(wreg[i][2], wreg[i][3]);
    }
  };

  // ---- fragment rows of this lane ----------------------------------------
  int xrow[TM], wrow[TP][2];
  #pragma unroll
  for (int t = 0; t < TM; ++t) xrow[t] = wm + 16 * t + c;
  #pragma unroll
  for (int p = 0; p < TP; ++p)
    #pragma unroll
    for (int h = 0; h < 2; ++h)
      wrow[p][h] = wn + 32 * p + 8 * (c >> 2) + 4 * h + (c & 3);

  f32x4 acc[TP][2][TM];
  #pragma unroll
  for (int p = 0; p < TP; ++p)
    #pragma unroll
    for (int h = 0; h < 2; ++h)
      #pragma unroll
      for (int t = 0; t < TM; ++t) acc[p][h][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = (a.K + kFlBK - 1) / kFlBK;
  load(0);
  stage(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < steps;  // uniform
    if (more) load((s + 1) * kFlBK);
    const int nks = (s * kFlBK + 32 < a.K) ? 2 : 1;  // a half step at the end
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks < nks) {
        const int j = 4 * ks + g;  // this lane's chunk of the row
        bf16x8 xf[TM];
        #pragma unroll
        for (int t = 0; t < TM; ++t)
          xf[t] = lds[buf][xrow[t]][j ^ fl_swz_x(xrow[t])];
        #pragma unroll
        for (int p = 0; p < TP; ++p)
          #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bf16x8 wf =
                lds[buf][BM + wrow[p][h]][j ^ fl_swz_w(wrow[p][h])];
            #pragma unroll
            for (int t = 0; t < TM; ++t)
              acc[p][h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  wf, xf[t], acc[p][h][t], 0, 0, 0);
          }
      }
    }
    // buffer buf ^ 1 was last read in step s - 1, before that step's barrier
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // ---- scale, bias, GELU, one rounding, store ----------------------------
  // lane (g, c) holds y[m = .. + c][n .. n + 7], n = n0 + wn + 32p + 8g:
  // element 4h + r is accumulator r of half h
  const bool vec_store = (a.N & 7) == 0;
  #pragma unroll
  for (int p = 0; p < TP; ++p) {
    const int n = n0 + wn + 32 * p + 8 * g;
    if (n >= a.N) continue;
    float sc[8], bi[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = n + e < a.N;
      sc[e] = ok ? a.scale[n + e] : 0.f;
      bi[e] = (ok && a.bias != nullptr) ? (float)a.bias[n + e] : 0.f;
    }
    #pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int m = m0 + wm + 16 * t + c;
      if (m >= a.M) continue;
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = acc[p][e >> 2][t][e & 3] * sc[e];
        if (a.bias != nullptr) v += bi[e];
        if (a.gelu) {
          const float u3 = 0.7978845608028654f * (v + 0.044715f * v * v * v);
          v = 0.5f * v * (1.f + tanhf(u3));
        }
        o[e] = (__bf16)v;
      }
      __bf16* dst = a.y + (long)m * a.N + n;
      if (vec_store) {  // N % 8 == 0: n + 7 < N and dst is 16-byte aligned
        *reinterpret_cast<bf16x8*>(dst) = o;
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          if (n + e < a.N) dst[e] = o[e];
      }
    }
  }
}

int64_t fl_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The tile of a call, from M and N alone: 128 x 128 where that grid has
// more workgroups than the 256 CUs, 64 x 64 below.
int64_t fl_tile(int64_t M, int64_t N) {
  return fl_cdiv(M, 128) * fl_cdiv(N, 128) >= kFlBigTiles ? 128 : 64;
}

using OptTensor = c10::optional<torch::Tensor>;

// `tile` is 128, 64, or 0 for fl_tile's pick
torch::Tensor fl_checked(const char* who, const torch::Tensor& x,
                         const torch::Tensor& weight,
                         const torch::Tensor& scale, const OptTensor& bias,
                         bool gelu, int64_t tile) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  // ---- every check first -------------------------------------------------
  TORCH_CHECK(tile == 0 || tile == 64 || tile == 128, who,
              ": no kernel for tile = ", tile);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.dim() == 2 && x.is_contiguous() &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              who, ": x must be a contiguous, 16-byte aligned bf16 GPU "
              "tensor [M, K]");
  const auto dev = x.device();
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(weight.is_cuda() && weight.device() == dev &&
              weight.scalar_type() == at::kFloat8_e4m3fn &&
              weight.dim() == 2 && weight.is_contiguous() &&
              reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
              who, ": weight_fp8 must be a contiguous, 16-byte aligned "
              "float8_e4m3fn [N, K] on x's device");
  const int64_t N = weight.size(0);
  TORCH_CHECK(scale.is_cuda() && scale.device() == dev &&
              scale.scalar_type() == at::kFloat && scale.dim() == 1 &&
              scale.is_contiguous() && scale.size(0) == N,
              who, ": weight_scale must be a contiguous fp32 [N = ", N,
              "] on x's device");
  TORCH_CHECK(weight.size(1) == K, who, ": weight_fp8 is [", N, ", ",
              weight.size(1), "], x has K = ", K);
  TORCH_CHECK(N >= 1, who, ": weight_fp8 has no rows");
  TORCH_CHECK(K >= 32 && K % 32 == 0, who, ": K = ", K,
              " must be a positive multiple of 32");
  if (bias.has_value())
    TORCH_CHECK(bias->is_cuda() && bias->device() == dev &&
                bias->scalar_type() == at::kBFloat16 && bias->dim() == 1 &&
                bias->is_contiguous() && bias->size(0) == N,
                who, ": bias must be a contiguous bf16 [N = ", N,
                "] on x's device");
  TORCH_CHECK(M < kLimit && N < kLimit && K < kLimit, who,
              ": 2^31 rows or columns or more");
  // the smallest tile has 64 columns: the grid's y extent is N / 64
  TORCH_CHECK(fl_cdiv(N, 64) <= 65535, who, ": N exceeds the grid");

  // ---- then the allocation and the launch ---------------------------------
  auto y = torch::empty({M, N}, x.options());
  if (M == 0) return y;
  FlArgs a;
  a.x = reinterpret_cast<const __bf16*>(x.data_ptr());
  a.w8 = reinterpret_cast<const unsigned char*>(weight.data_ptr());
  a.scale = scale.data_ptr<float>();
  a.bias = bias.has_value()
               ? reinterpret_cast<const __bf16*>(bias->data_ptr())
               : nullptr;
  a.y = reinterpret_cast<__bf16*>(y.data_ptr());
  a.M = (int)M;
  a.N = (int)N;
  a.K = (int)K;
  a.gelu = gelu ? 1 : 0;
  if (tile == 0) tile = fl_tile(M, N);
  auto stream = at::hip::getCurrentHIPStream().stream();
  const dim3 grid((unsigned)fl_cdiv(M, tile), (unsigned)fl_cdiv(N, tile));
  if (tile == 128)
    hipLaunchKernelGGL((fp8_linear_kernel<128, 128>), grid,
                       dim3(kFlThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((fp8_linear_kernel<64, 64>), grid, dim3(kFlThreads),
                       0, stream, a);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, who, ": ", hipGetErrorString(e));
  return y;
}

}  // namespace

#pragma clang attribute pop

torch::Tensor fp8_linear_fwd(torch::Tensor x, torch::Tensor weight_fp8,
                             torch::Tensor weight_scale,
                             c10::optional<torch::Tensor> bias, bool gelu) {
  return fl_checked("fp8_linear_fwd", x, weight_fp8, weight_scale, bias,
                    gelu, 0);
}

// the same op at a given tile (64 or 128), for the measurement that picks
// kFlBigTiles and for the tests of either instantiation at small shapes
torch::Tensor fp8_linear_fwd_at(torch::Tensor x, torch::Tensor weight_fp8,
                                torch::Tensor weight_scale,
                                c10::optional<torch::Tensor> bias, bool gelu,
                                int64_t tile) {
  return fl_checked("fp8_linear_fwd_at", x, weight_fp8, weight_scale, bias,
                    gelu, tile);
}
