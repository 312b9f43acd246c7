// Fused (dropout +) residual-add + LayerNorm for [R, C] rows
// (transformer pre-norm blocks) on CDNA4. One kernel set; dropout, the
// residual and the extra gradient are template switches.
//
//   forward:  x_new = res + keep * sub / (1-p)   (no residual: res = 0;
//                                                 p == 0: keep = 1)
//             y     = (x_new - mean_row) * invstd_row * g + beta
//   one kernel: reads sub,res once, writes x_new,y once — replaces the
//   eager dropout + add (2R+1W each) + ATen LN (1R+1W) chain and its
//   backward's grad_input + two-stage PartGradGammaBeta kernels. y is
//   computed from the stored, rounded x_new. Plain LN of sub (no
//   residual, p == 0) stores no x_new: x_new is sub.
//
//   backward: block-per-row dx kernel (row reductions in LDS) +
//             column-reduction kernel for dgamma/dbeta with the same
//             two-stage [nblocks, C] -> fold pattern as fused_bn.hip.
//
// g = invstd * (dyg - mean_row(dyg) - xhat * mean_row(dyg * xhat))
//     + d_extern(x_new),   dyg = dy * gamma;
// d(res) = g, d(sub) = keep * g / (1-p), both from the fp32 g. With
// p == 0 they are the same values and one buffer is written.
//
// Row layout: C contiguous, bf16/f32; C % 8 == 0 (bf16) / % 4 (f32),
// C <= 16384. gamma, beta, mean, invstd are fp32. The two entry points
// at the end of the file check all of it before anything is launched.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <ATen/hip/HIPGraphsUtils.cuh>

#include <type_traits>

#include "philox_dropout.h"

#define CHECK_HIP_LN(cmd)                                                  \
  do {                                                                     \
    hipError_t e = (cmd);                                                  \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e));     \
  } while (0)

namespace {

constexpr int kT = 256;

template <typename T> struct LnVec;
template <> struct LnVec<float> { static constexpr int V = 4; };
template <> struct LnVec<__hip_bfloat16> { static constexpr int V = 8; };

template <typename T>
__device__ __forceinline__ float ln_tof(T v);
template <>
__device__ __forceinline__ float ln_tof<float>(float v) { return v; }
template <>
__device__ __forceinline__ float ln_tof<__hip_bfloat16>(
    __hip_bfloat16 v) { return __bfloat162float(v); }

template <typename T>
__device__ __forceinline__ T ln_fromf(float v);
template <>
__device__ __forceinline__ float ln_fromf<float>(float v) { return v; }
template <>
__device__ __forceinline__ __hip_bfloat16 ln_fromf<__hip_bfloat16>(
    float v) { return __float2bfloat16(v); }

__device__ __forceinline__ float block_sum(float v, float* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const float out = lds[0];
  __syncthreads();
  return out;
}

// ====================================================================
// The dropout mask is never stored. keep(i) for flat element
// i = r*C + c is
//   word[i & 3] of Philox4x32-10(key = seed, counter = (offset/4, i>>2))
//   >= floor(p * 2^32)
// i.e. one Philox call per aligned group of four elements, one 32-bit
// word per element: a pure function of (seed, offset, i). A bf16 slot
// (8 elements) makes two calls, an fp32 slot (4 elements) one, so both
// dtypes, any grid and any row->block assignment draw the same mask,
// and backward regenerates exactly what forward used. The counter
// layout is the one torch's own Philox consumers use (offset/4 in the
// low 64 bits, the "subsequence" i>>2 in the high 64), so advancing the
// generator's offset by 4 per call keeps every (key, counter) pair
// unique among all users of that generator.
// ====================================================================

// DropArgs, philox4x32_10 and make_drop_args: philox_dropout.h, shared
// with the flash attention dropout kernels.

// keep bits for the V elements starting at flat element e0 (e0 % 4 == 0)
template <int V>
__device__ __forceinline__ uint32_t drop_keep_bits(uint64_t e0,
                                                   const DropArgs& d) {
  uint32_t bits = 0;
  #pragma unroll
  for (int j = 0; j < V / 4; ++j) {
    const uint64_t g = (e0 >> 2) + j;
    const uint4 w = philox4x32_10(
        d.k0, d.k1,
        make_uint4(d.o0, d.o1, (uint32_t)g, (uint32_t)(g >> 32)));
    bits |= (uint32_t)(w.x >= d.thr) << (4 * j);
    bits |= (uint32_t)(w.y >= d.thr) << (4 * j + 1);
    bits |= (uint32_t)(w.z >= d.thr) << (4 * j + 2);
    bits |= (uint32_t)(w.w >= d.thr) << (4 * j + 3);
  }
  return bits;
}

// --------------------------------------------------------------------
// forward: one block per row. RES: a residual is added; DROP: sub is
// dropped on the way in. x_new is stored iff RES || DROP.
// The three ways of forming x_new stay separate expressions: the
// compiler contracts a * b + c to an FMA, so one merged form
// (res + keep * sub * scale) would round differently from these.
// --------------------------------------------------------------------
template <typename T, bool RES, bool DROP>
__global__ __launch_bounds__(kT) void ln_fwd_kernel(
    const T* __restrict__ sub, const T* __restrict__ res,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    T* __restrict__ x_new, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ invstd_out,
    long R, int C, float eps, DropArgs drop) {
  constexpr int V = LnVec<T>::V;
  constexpr bool STORE = RES || DROP;
  const int nvec = C / V;   // vector slots per row
  __shared__ float lds[kT];

  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const T* srow = sub + r * C;
    const T* rrow = RES ? res + r * C : nullptr;
    T* xrow = STORE ? x_new + r * C : nullptr;
    // pass 1: form x; accumulate sum/sumsq; stage x in registers
    // when the row fits (C <= kT*V covers GPT-2 sizes), else re-read.
    float s = 0.f, s2 = 0.f;
    const bool fits = nvec <= kT;
    // local storage for one vector slot per thread (fits case)
    T xloc[LnVec<T>::V];
    for (int vi = threadIdx.x; vi < nvec; vi += kT) {
      T xv[V];
      if constexpr (DROP) {
        T sv[V];
        *reinterpret_cast<int4*>(sv) =
            *reinterpret_cast<const int4*>(srow + vi * V);
        if constexpr (RES)
          *reinterpret_cast<int4*>(xv) =
              *reinterpret_cast<const int4*>(rrow + vi * V);
        const uint32_t keep =
            drop_keep_bits<V>((uint64_t)r * C + (uint64_t)vi * V, drop);
        #pragma unroll
        for (int i = 0; i < V; ++i) {
          const float sc = ln_tof<T>(sv[i]) * drop.scale;
          const bool k = (keep >> i) & 1u;
          if constexpr (RES) {
            // dropped: the residual passes through unchanged (T -> f32
            // -> T is exact), not as res + 0
            const float rf = ln_tof<T>(xv[i]);
            xv[i] = ln_fromf<T>(k ? rf + sc : rf);
          } else {
            xv[i] = ln_fromf<T>(k ? sc : 0.f);
          }
        }
      } else if constexpr (RES) {
        T sv[V];
        *reinterpret_cast<int4*>(xv) =
            *reinterpret_cast<const int4*>(rrow + vi * V);
        *reinterpret_cast<int4*>(sv) =
            *reinterpret_cast<const int4*>(srow + vi * V);
        #pragma unroll
        for (int i = 0; i < V; ++i)
          xv[i] = ln_fromf<T>(ln_tof<T>(xv[i]) + ln_tof<T>(sv[i]));
      } else {
        *reinterpret_cast<int4*>(xv) =
            *reinterpret_cast<const int4*>(srow + vi * V);
      }
      if constexpr (STORE)
        *reinterpret_cast<int4*>(xrow + vi * V) =
            *reinterpret_cast<const int4*>(xv);
      #pragma unroll
      for (int i = 0; i < V; ++i) {
        const float f = ln_tof<T>(xv[i]);
        s += f;
        s2 += f * f;
      }
      if (fits) {
        #pragma unroll
        for (int i = 0; i < V; ++i) xloc[i] = xv[i];
      }
    }
    s = block_sum(s, lds);
    s2 = block_sum(s2, lds);
    const float mean = s / (float)C;
    const float var = fmaxf(s2 / (float)C - mean * mean, 0.f);
    const float invstd = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
      mean_out[r] = mean;
      invstd_out[r] = invstd;
    }
    // pass 2: normalize + affine
    for (int vi = threadIdx.x; vi < nvec; vi += kT) {
      T av[V];
      if (fits && (unsigned)vi == threadIdx.x) {
        #pragma unroll
        for (int i = 0; i < V; ++i) av[i] = xloc[i];
      } else {
        // STORE: this thread's own pass-1 store, visible to it in
        // program order
        const T* src = STORE ? xrow : srow;
        *reinterpret_cast<int4*>(av) =
            *reinterpret_cast<const int4*>(src + vi * V);
      }
      float gv[V], bv2[V];
      #pragma unroll
      for (int i = 0; i < V; i += 4) {
        *reinterpret_cast<float4*>(gv + i) =
            *reinterpret_cast<const float4*>(gamma + vi * V + i);
        *reinterpret_cast<float4*>(bv2 + i) =
            *reinterpret_cast<const float4*>(beta + vi * V + i);
      }
      T ov[V];
      #pragma unroll
      for (int i = 0; i < V; ++i)
        ov[i] = ln_fromf<T>(
            (ln_tof<T>(av[i]) - mean) * invstd * gv[i] + bv2[i]);
      *reinterpret_cast<int4*>(y + r * C + vi * V) =
          *reinterpret_cast<const int4*>(ov);
    }
  }
}

// --------------------------------------------------------------------
// backward dx: block per row. dyg = dy * gamma;
// g = invstd * (dyg - mean(dyg) - xhat * mean(dyg * xhat))
// EXT: dext (grad flowing into x_new from its other consumer) is added.
// DROP: g goes to d_res (RES only) and keep * g / (1-p), with the mask
// drawn again, to d_sub. !DROP: g is both; it is written once, to
// d_sub (instantiated with RES = false only).
// --------------------------------------------------------------------
template <typename T, bool EXT, bool RES, bool DROP>
__global__ __launch_bounds__(kT) void ln_bwd_dx_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const T* __restrict__ dext, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    T* __restrict__ d_res, T* __restrict__ d_sub, long R, int C,
    DropArgs drop) {
  constexpr int V = LnVec<T>::V;
  const int nvec = C / V;
  __shared__ float lds[kT];

  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const float mu = mean[r];
    const float is = invstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int vi = threadIdx.x; vi < nvec; vi += kT) {
      T dv[V], xv[V];
      *reinterpret_cast<int4*>(dv) =
          *reinterpret_cast<const int4*>(dy + r * C + vi * V);
      *reinterpret_cast<int4*>(xv) =
          *reinterpret_cast<const int4*>(x + r * C + vi * V);
      float gv[V];
      #pragma unroll
      for (int i = 0; i < V; i += 4)
        *reinterpret_cast<float4*>(gv + i) =
            *reinterpret_cast<const float4*>(gamma + vi * V + i);
      #pragma unroll
      for (int i = 0; i < V; ++i) {
        const float dyg = ln_tof<T>(dv[i]) * gv[i];
        const float xh = (ln_tof<T>(xv[i]) - mu) * is;
        s1 += dyg;
        s2 += dyg * xh;
      }
    }
    s1 = block_sum(s1, lds) / (float)C;
    s2 = block_sum(s2, lds) / (float)C;
    for (int vi = threadIdx.x; vi < nvec; vi += kT) {
      T dv[V], xv[V];
      *reinterpret_cast<int4*>(dv) =
          *reinterpret_cast<const int4*>(dy + r * C + vi * V);
      *reinterpret_cast<int4*>(xv) =
          *reinterpret_cast<const int4*>(x + r * C + vi * V);
      T ev[V];
      if constexpr (EXT)
        *reinterpret_cast<int4*>(ev) =
            *reinterpret_cast<const int4*>(dext + r * C + vi * V);
      float gv[V];
      #pragma unroll
      for (int i = 0; i < V; i += 4)
        *reinterpret_cast<float4*>(gv + i) =
            *reinterpret_cast<const float4*>(gamma + vi * V + i);
      uint32_t keep = 0;
      if constexpr (DROP)
        keep = drop_keep_bits<V>((uint64_t)r * C + (uint64_t)vi * V,
                                 drop);
      T ov[V], sv[V];
      #pragma unroll
      for (int i = 0; i < V; ++i) {
        const float dyg = ln_tof<T>(dv[i]) * gv[i];
        const float xh = (ln_tof<T>(xv[i]) - mu) * is;
        float g = is * (dyg - s1 - xh * s2);
        if constexpr (EXT) g += ln_tof<T>(ev[i]);
        ov[i] = ln_fromf<T>(g);
        if constexpr (DROP)
          sv[i] = ln_fromf<T>(((keep >> i) & 1u) ? g * drop.scale : 0.f);
      }
      if constexpr (DROP) {
        if constexpr (RES)
          *reinterpret_cast<int4*>(d_res + r * C + vi * V) =
              *reinterpret_cast<const int4*>(ov);
        *reinterpret_cast<int4*>(d_sub + r * C + vi * V) =
            *reinterpret_cast<const int4*>(sv);
      } else {
        *reinterpret_cast<int4*>(d_sub + r * C + vi * V) =
            *reinterpret_cast<const int4*>(ov);
      }
    }
  }
}

// --------------------------------------------------------------------
// backward dgamma/dbeta: stage 1 like fused_bn (rows x channels
// partials), then the bn_fold pattern. Reuses the column-reduction
// structure: thread layout (C/V slots x rows-per-block).
// --------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void ln_bwd_gb_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    float* __restrict__ partial, long R, int C) {
  constexpr int V = LnVec<T>::V;
  const int nvec = C / V;
  // Each block owns a channel-slot range and strides over rows.
  // Layout: threads split as (slots_per_block x rows_per_block).
  const int spb = min(nvec, kT);       // slots handled per block row
  const int rpb = kT / spb;            // rows in flight
  const int slot0 = (int)(blockIdx.x % ((nvec + spb - 1) / spb)) * spb;
  const int nblk_c = (nvec + spb - 1) / spb;
  const int brow = (int)(blockIdx.x / nblk_c);
  const int nblk_r = (int)(gridDim.x / nblk_c);
  const int slot = slot0 + (int)(threadIdx.x % spb);
  const int rlane = (int)(threadIdx.x / spb);

  float dg[V], db[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { dg[i] = 0.f; db[i] = 0.f; }

  if (slot < nvec) {
    for (long r = (long)brow * rpb + rlane; r < R;
         r += (long)nblk_r * rpb) {
      const float mu = mean[r];
      const float is = invstd[r];
      T dv[V], xv[V];
      *reinterpret_cast<int4*>(dv) =
          *reinterpret_cast<const int4*>(dy + r * C + slot * V);
      *reinterpret_cast<int4*>(xv) =
          *reinterpret_cast<const int4*>(x + r * C + slot * V);
      #pragma unroll
      for (int i = 0; i < V; ++i) {
        const float d = ln_tof<T>(dv[i]);
        const float xh = (ln_tof<T>(xv[i]) - mu) * is;
        db[i] += d;
        dg[i] += d * xh;
      }
    }
  }

  __shared__ float lds[kT * LnVec<T>::V];
  const long pC = (long)gridDim.x * C;  // plane stride (grid, C)
  for (int pass = 0; pass < 2; ++pass) {
    #pragma unroll
    for (int i = 0; i < V; ++i)
      lds[threadIdx.x * V + i] = pass ? db[i] : dg[i];
    __syncthreads();
    for (int s = rpb / 2; s > 0; s >>= 1) {
      if (rlane < s) {
        #pragma unroll
        for (int i = 0; i < V; ++i)
          lds[threadIdx.x * V + i] +=
              lds[(threadIdx.x + s * spb) * V + i];
      }
      __syncthreads();
    }
    if (rlane == 0 && slot < nvec) {
      #pragma unroll
      for (int i = 0; i < V; ++i)
        partial[pass * pC + (long)blockIdx.x * C + slot * V + i] =
            lds[threadIdx.x * V + i];
    }
    __syncthreads();
  }
}

// 2-D fold (channel-groups x b-slices) -> [kLnB2, C] second-level
// partials, then a tiny per-channel kernel — the same structure as
// fused_bn's fold (a 1-thread-per-channel fold measured 74us
// latency-bound on GPT-2-XL's 776 calls/step).
constexpr int kLnFoldC = 64;
constexpr int kLnB2 = 16;

__global__ __launch_bounds__(256) void ln_fold2_kernel(
    const float* __restrict__ partial, int nblocks,
    float* __restrict__ partial2, int C) {
  const int lanes = 256 / kLnFoldC;
  const int c = blockIdx.x * kLnFoldC + (int)(threadIdx.x % kLnFoldC);
  const int lane = (int)(threadIdx.x / kLnFoldC);
  const bool active = c < C;
  const int b_begin = (int)(((long)blockIdx.y * nblocks) / kLnB2);
  const int b_end = (int)(((long)(blockIdx.y + 1) * nblocks) / kLnB2);
  const long pC = (long)nblocks * C;
  float dg = 0.f, db = 0.f;
  if (active)
    for (int b = b_begin + lane; b < b_end; b += lanes) {
      dg += partial[(long)b * C + c];
      db += partial[pC + (long)b * C + c];
    }
  __shared__ float l1[256], l2[256];
  l1[threadIdx.x] = dg;
  l2[threadIdx.x] = db;
  __syncthreads();
  for (int st = lanes / 2; st > 0; st >>= 1) {
    if (lane < st) {
      l1[threadIdx.x] += l1[threadIdx.x + st * kLnFoldC];
      l2[threadIdx.x] += l2[threadIdx.x + st * kLnFoldC];
    }
    __syncthreads();
  }
  if (lane != 0 || !active) return;
  const long p2C = (long)kLnB2 * C;
  partial2[(long)blockIdx.y * C + c] = l1[threadIdx.x];
  partial2[p2C + (long)blockIdx.y * C + c] = l2[threadIdx.x];
}

__global__ void ln_gb_fold_kernel(
    const float* __restrict__ partial2, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long p2C = (long)kLnB2 * C;
  float dg = 0.f, db = 0.f;
  #pragma unroll
  for (int b = 0; b < kLnB2; ++b) {
    dg += partial2[(long)b * C + c];
    db += partial2[p2C + (long)b * C + c];
  }
  dgamma[c] = dg;
  dbeta[c] = db;
}

long ln_rows_grid(long R) {
  return std::min<long>(std::max<long>(R, 1), 8192);
}

// ---------------------------------------------------------------- host

struct LnShape { long R; int C; };

// The operand checks of both directions. x fixes dtype, shape and
// device: sub in forward, x_new in backward. `same` (null entries:
// operand absent) must match it; `per_col` are fp32 [C], `per_row`
// fp32 [R].
LnShape ln_check_operands(
    const torch::Tensor& x,
    std::initializer_list<const torch::Tensor*> same,
    std::initializer_list<const torch::Tensor*> per_col,
    std::initializer_list<const torch::Tensor*> per_row, double p) {
  TORCH_CHECK(x.is_cuda() && x.dim() >= 1 && x.size(-1) > 0,
              "fused_ln: rows must be a GPU tensor [..., C], C > 0");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
                  x.scalar_type() == at::kFloat,
              "fused_ln: dtype must be bf16 or f32");
  TORCH_CHECK(x.is_contiguous(), "fused_ln: contiguous input required");
  for (const torch::Tensor* t : same)
    TORCH_CHECK(t == nullptr ||
                    (t->sizes() == x.sizes() &&
                     t->scalar_type() == x.scalar_type() &&
                     t->device() == x.device() && t->is_contiguous()),
                "fused_ln: residual and grads must be contiguous and "
                "match the rows' shape, dtype and device");
  const long C = x.size(-1);
  const long R = x.numel() / C;
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(C % V == 0, "fused_ln: C % ", V, " != 0");
  TORCH_CHECK(C <= 16384, "fused_ln: C > 16384");
  auto fp32_vec = [&](const torch::Tensor* t, long n) {
    return t->scalar_type() == at::kFloat && t->numel() == n &&
           t->device() == x.device() && t->is_contiguous();
  };
  for (const torch::Tensor* t : per_col)
    TORCH_CHECK(fp32_vec(t, C),
                "fused_ln: weight/bias must be fp32 with C elements");
  for (const torch::Tensor* t : per_row)
    TORCH_CHECK(fp32_vec(t, R),
                "fused_ln: mean/invstd must be fp32 with R elements");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "fused_ln: p must be in [0, 1)");
  return {R, (int)C};
}

const torch::Tensor* ln_opt(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? &*t : nullptr;
}

// dgamma/dbeta (they do not depend on the mask): stage-1 partials, the
// 2-D fold, the per-channel fold.
void ln_gamma_beta_grads(const torch::Tensor& dy, const torch::Tensor& x,
                         const torch::Tensor& mean,
                         const torch::Tensor& invstd,
                         torch::Tensor& dgamma, torch::Tensor& dbeta,
                         long R, int C, hipStream_t stream) {
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  auto fopts = dgamma.options();
  const int V = bf16 ? 8 : 4;
  const int nvec = C / V;
  const int spb = std::min(nvec, kT);
  const int rpb = kT / spb;
  const int nblk_c = (nvec + spb - 1) / spb;
  const int nblk_r = (int)std::min<long>((R + rpb - 1) / rpb, 256);
  const int nb = nblk_c * nblk_r;
  // zeros: a block writes only its own slot range of its [C] row
  auto partial = torch::zeros({2, nb, C}, fopts);
  auto partial2 = torch::empty({2, kLnB2, C}, fopts);
  #define LAUNCH_GB(T)                                                    \
    hipLaunchKernelGGL((ln_bwd_gb_kernel<T>), dim3(nb), dim3(kT), 0,     \
        stream, reinterpret_cast<const T*>(dy.data_ptr()),               \
        reinterpret_cast<const T*>(x.data_ptr()),                        \
        mean.data_ptr<float>(), invstd.data_ptr<float>(),                \
        partial.data_ptr<float>(), R, C)
  if (bf16) LAUNCH_GB(__hip_bfloat16); else LAUNCH_GB(float);
  #undef LAUNCH_GB
  CHECK_HIP_LN(hipGetLastError());
  hipLaunchKernelGGL(ln_fold2_kernel,
                     dim3((C + kLnFoldC - 1) / kLnFoldC, kLnB2),
                     dim3(256), 0, stream, partial.data_ptr<float>(),
                     nb, partial2.data_ptr<float>(), C);
  CHECK_HIP_LN(hipGetLastError());
  hipLaunchKernelGGL(ln_gb_fold_kernel, dim3((C + 255) / 256), dim3(256),
                     0, stream, partial2.data_ptr<float>(),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
                     C);
  CHECK_HIP_LN(hipGetLastError());
}

}  // namespace

// sub: [R, C], the operand that is dropped when p > 0; res: optional
// residual. Returns (y, x_new, mean, invstd, seed, offset).
// p > 0 draws (seed, offset) from the default generator of sub's
// device; backward takes the two integers back and regenerates the
// mask. p == 0 leaves the generator alone (seed = offset = 0) and can
// be captured in a graph. Without a residual and with p == 0, x_new is
// sub itself — no copy made.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           uint64_t, uint64_t>
fused_ln_fwd(torch::Tensor sub, c10::optional<torch::Tensor> res,
             torch::Tensor gamma, torch::Tensor beta, double eps,
             double p) {
  const auto [R, C] =
      ln_check_operands(sub, {ln_opt(res)}, {&gamma, &beta}, {}, p);
  const bool has_res = res.has_value(), drop = p > 0.0;
  std::pair<uint64_t, uint64_t> rng{0, 0};
  if (drop) {
    // graph-capture-safe RNG (device-side offset) is not implemented
    at::cuda::assertNotCapturing("fused_ln: drawing the dropout seed");
    auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
        c10::nullopt,
        at::cuda::detail::getDefaultCUDAGenerator(sub.get_device()));
    std::lock_guard<std::mutex> lock(gen->mutex_);
    // one Philox call per (offset/4, element group): 4 outputs "per
    // thread" in the generator's bookkeeping
    rng = gen->philox_engine_inputs(4);
  }
  const DropArgs dargs = make_drop_args(p, rng.first, rng.second);

  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(sub);
  auto x_new = has_res || drop ? torch::empty_like(sub) : sub;
  auto fopts = gamma.options().dtype(at::kFloat);
  auto mean = torch::empty({R}, fopts);
  auto invstd = torch::empty({R}, fopts);

  auto launch = [&, R = R, C = C](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto* kern =
        drop ? (has_res ? ln_fwd_kernel<T, true, true>
                        : ln_fwd_kernel<T, false, true>)
             : (has_res ? ln_fwd_kernel<T, true, false>
                        : ln_fwd_kernel<T, false, false>);
    hipLaunchKernelGGL(
        kern, dim3(ln_rows_grid(R)), dim3(kT), 0, stream,
        reinterpret_cast<const T*>(sub.data_ptr()),
        has_res ? reinterpret_cast<const T*>(res->data_ptr()) : nullptr,
        gamma.data_ptr<float>(), beta.data_ptr<float>(),
        has_res || drop ? reinterpret_cast<T*>(x_new.data_ptr())
                        : nullptr,
        reinterpret_cast<T*>(y.data_ptr()), mean.data_ptr<float>(),
        invstd.data_ptr<float>(), R, C, (float)eps, dargs);
  };
  if (sub.scalar_type() == at::kBFloat16) launch((__hip_bfloat16*)nullptr);
  else launch((float*)nullptr);
  CHECK_HIP_LN(hipGetLastError());
  return {y, x_new, mean, invstd, rng.first, rng.second};
}

// x: the x_new of the forward; dext: optional extra grad into x_new;
// (p, seed, offset): as passed to / returned by the forward. Returns
// (d_res, d_sub, dgamma, dbeta); d_res is undefined (None) when has_res
// is false, and the same buffer as d_sub when p == 0.
std::vector<c10::optional<torch::Tensor>> fused_ln_bwd(
    torch::Tensor dy, torch::Tensor x,
    c10::optional<torch::Tensor> dext, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor invstd, double p, uint64_t seed,
    uint64_t offset, bool has_res) {
  dy = dy.contiguous();
  const auto [R, C] = ln_check_operands(x, {&dy, ln_opt(dext)}, {&gamma},
                                        {&mean, &invstd}, p);
  const bool ext = dext.has_value(), drop = p > 0.0;
  const DropArgs dargs = make_drop_args(p, seed, offset);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto d_sub = torch::empty_like(x);
  c10::optional<torch::Tensor> d_res;
  if (has_res) d_res = drop ? torch::empty_like(x) : d_sub;
  auto fopts = gamma.options().dtype(at::kFloat);
  auto dgamma = torch::empty({C}, fopts);
  auto dbeta = torch::empty({C}, fopts);

  auto launch = [&, R = R, C = C](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto* kern =
        !drop ? (ext ? ln_bwd_dx_kernel<T, true, false, false>
                     : ln_bwd_dx_kernel<T, false, false, false>)
        : ext ? (has_res ? ln_bwd_dx_kernel<T, true, true, true>
                         : ln_bwd_dx_kernel<T, true, false, true>)
              : (has_res ? ln_bwd_dx_kernel<T, false, true, true>
                         : ln_bwd_dx_kernel<T, false, false, true>);
    hipLaunchKernelGGL(
        kern, dim3(ln_rows_grid(R)), dim3(kT), 0, stream,
        reinterpret_cast<const T*>(dy.data_ptr()),
        reinterpret_cast<const T*>(x.data_ptr()),
        ext ? reinterpret_cast<const T*>(dext->data_ptr()) : nullptr,
        gamma.data_ptr<float>(), mean.data_ptr<float>(),
        invstd.data_ptr<float>(),
        has_res && drop ? reinterpret_cast<T*>(d_res->data_ptr())
                        : nullptr,
        reinterpret_cast<T*>(d_sub.data_ptr()), R, C, dargs);
  };
  if (x.scalar_type() == at::kBFloat16) launch((__hip_bfloat16*)nullptr);
  else launch((float*)nullptr);
  CHECK_HIP_LN(hipGetLastError());

  ln_gamma_beta_grads(dy, x, mean, invstd, dgamma, dbeta, R, C, stream);
  return {d_res, d_sub, dgamma, dbeta};
}
