// Fused BatchNorm(+ReLU)(+residual add) for NHWC (channels_last) on
// CDNA4. Replaces the MIOpen BN kernel quintet + ATen add/clamp chain
// that dominates the ResNet-50 step (see
// profiles/r01_resnet50_1gpu_fixedfind.md: BN + elementwise = >50% of
// step time; the convs themselves are only ~1/3).
//
// Memory-bound design: the train forward is 2 passes over x (stats +
// apply) instead of eager's 4 reads + 3 writes (BN stats, BN norm,
// add, relu); the backward is 2 passes (reduce + dx) instead of 5.
//
// Per-channel reductions are TWO-STAGE: stage 1 writes per-workgroup
// partials [nblocks, C] (coalesced stores, no atomics — a v1 of this
// file used one fp32 atomicAdd per (block, channel) and the ~8k
// serialized RMWs per address made stats 50x slower than MIOpen's);
// stage 2 folds partials and emits the per-channel coefficients the
// elementwise pass needs, so the hot elementwise kernels do float4
// coefficient loads instead of 16 scalar loads per 8 elements.
// Fixed stage-1 grid => deterministic accumulation order.
//
// Layout convention: x is [R, C] row-major with C contiguous
// (R = N*H*W): exactly torch channels_last.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define CHECK_HIP_BN(cmd)                                                  \
  do {                                                                     \
    hipError_t e = (cmd);                                                  \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e));     \
  } while (0)

namespace {

constexpr int kT = 256;        // 4 wave64 per workgroup
constexpr int kMaxStage1 = 1024;  // stage-1 workgroups (reduction grid)

template <typename T> struct BnVec;
template <> struct BnVec<float> { static constexpr int V = 4; };
template <> struct BnVec<__hip_bfloat16> { static constexpr int V = 8; };

template <typename T>
__device__ __forceinline__ float bn_tof(T v);
template <>
__device__ __forceinline__ float bn_tof<float>(float v) { return v; }
template <>
__device__ __forceinline__ float bn_tof<__hip_bfloat16>(
    __hip_bfloat16 v) { return __bfloat162float(v); }

template <typename T>
__device__ __forceinline__ T bn_fromf(float v);
template <>
__device__ __forceinline__ float bn_fromf<float>(float v) { return v; }
template <>
__device__ __forceinline__ __hip_bfloat16 bn_fromf<__hip_bfloat16>(
    float v) { return __float2bfloat16(v); }

template <typename T, int V>
__device__ __forceinline__ void load_vec(T (&dst)[V], const T* src) {
  *reinterpret_cast<int4*>(dst) = *reinterpret_cast<const int4*>(src);
}
template <typename T, int V>
__device__ __forceinline__ void store_vec(T* dst, const T (&src)[V]) {
  *reinterpret_cast<int4*>(dst) = *reinterpret_cast<const int4*>(src);
}
template <int V>
__device__ __forceinline__ void load_coef(float (&dst)[V],
                                          const float* src) {
  #pragma unroll
  for (int i = 0; i < V; i += 4)
    *reinterpret_cast<float4*>(dst + i) =
        *reinterpret_cast<const float4*>(src + i);
}

// --------------------------------------------------------------------
// stage 1 stats: per-(block, channel) partial sum / sumsq
// partial layout: [2, nblocks, C] (sum plane then sumsq plane)
// --------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void bn_stats_kernel(
    const T* __restrict__ x, float* __restrict__ partial, long R,
    int C) {
  constexpr int V = BnVec<T>::V;
  const int tpr = C / V;             // threads per row (<= kT)
  const int rpb = kT / tpr;          // rows per block (power of 2)
  const int slot = threadIdx.x % tpr;
  const int row_in_block = threadIdx.x / tpr;
  const int c0 = slot * V;

  float acc[V], acc2[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { acc[i] = 0.f; acc2[i] = 0.f; }

  const long row_stride = (long)gridDim.x * rpb;
  for (long r = (long)blockIdx.x * rpb + row_in_block; r < R;
       r += row_stride) {
    T v[V];
    load_vec<T, V>(v, x + r * C + c0);
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      const float f = bn_tof<T>(v[i]);
      acc[i] += f;
      acc2[i] += f * f;
    }
  }

  __shared__ float lds[kT * BnVec<T>::V];
  const long nbC = (long)gridDim.x * C;
  // reduce sum then sumsq across the rpb rows sharing a channel slot
  for (int pass = 0; pass < 2; ++pass) {
    #pragma unroll
    for (int i = 0; i < V; ++i)
      lds[threadIdx.x * V + i] = pass ? acc2[i] : acc[i];
    __syncthreads();
    for (int s = rpb / 2; s > 0; s >>= 1) {
      if (row_in_block < s) {
        #pragma unroll
        for (int i = 0; i < V; ++i)
          lds[threadIdx.x * V + i] +=
              lds[(threadIdx.x + s * tpr) * V + i];
      }
      __syncthreads();
    }
    if (row_in_block == 0) {
      #pragma unroll
      for (int i = 0; i < V; ++i)
        partial[pass * nbC + (long)blockIdx.x * C + c0 + i] =
            lds[threadIdx.x * V + i];
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------
// stage 2a: fold the [nblocks, C] partials down to [kB2, C] with a 2-D
// grid (channel-groups x b-slices) so even C=64 layers get enough
// workgroups to hide memory latency (a v3 used one block per 64
// channels: 1 block on the whole chip for layer1, 74us latency-bound).
// Deterministic: fixed slice boundaries, no atomics.
// stage 2b: tiny per-channel kernel folds the kB2 rows and computes
// the coefficients.
// --------------------------------------------------------------------
constexpr int kFoldC = 64;   // channels per fold block
constexpr int kB2 = 16;      // second-level partial rows

__global__ __launch_bounds__(kT) void bn_fold2_kernel(
    const float* __restrict__ partial, int nblocks,
    float* __restrict__ partial2, int C) {
  // grid: (ceil(C/kFoldC), kB2); threads (kFoldC x lanes)
  const int lanes = kT / kFoldC;
  const int c = blockIdx.x * kFoldC + threadIdx.x % kFoldC;
  const int lane = threadIdx.x / kFoldC;
  const bool active = c < C;
  const int b_begin = (int)(((long)blockIdx.y * nblocks) / kB2);
  const int b_end = (int)(((long)(blockIdx.y + 1) * nblocks) / kB2);
  const long nbC = (long)nblocks * C;
  float s = 0.f, s2 = 0.f;
  if (active)
    for (int b = b_begin + lane; b < b_end; b += lanes) {
      s += partial[(long)b * C + c];
      s2 += partial[nbC + (long)b * C + c];
    }
  __shared__ float lsum[kT], lsq[kT];
  lsum[threadIdx.x] = s;
  lsq[threadIdx.x] = s2;
  __syncthreads();
  for (int st = lanes / 2; st > 0; st >>= 1) {
    if (lane < st) {
      lsum[threadIdx.x] += lsum[threadIdx.x + st * kFoldC];
      lsq[threadIdx.x] += lsq[threadIdx.x + st * kFoldC];
    }
    __syncthreads();
  }
  if (lane != 0 || !active) return;
  const long b2C = (long)kB2 * C;
  partial2[(long)blockIdx.y * C + c] = lsum[threadIdx.x];
  partial2[b2C + (long)blockIdx.y * C + c] = lsq[threadIdx.x];
}

__global__ void bn_stats_coef_kernel(
    const float* __restrict__ partial2,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float* __restrict__ mean_out, float* __restrict__ invstd_out,
    float* __restrict__ scale_out, float* __restrict__ bias_out,
    long R, int C, float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long b2C = (long)kB2 * C;
  float s = 0.f, s2 = 0.f;
  #pragma unroll
  for (int b = 0; b < kB2; ++b) {
    s += partial2[(long)b * C + c];
    s2 += partial2[b2C + (long)b * C + c];
  }
  const float m = s / (float)R;
  const float var = fmaxf(s2 / (float)R - m * m, 0.f);
  const float inv = rsqrtf(var + eps);
  mean_out[c] = m;
  invstd_out[c] = inv;
  const float sc = gamma[c] * inv;
  scale_out[c] = sc;
  bias_out[c] = beta[c] - m * sc;
  if (running_mean != nullptr) {
    // unbiased variance for running stats (torch semantics)
    const float var_unb = R > 1 ? var * (float)R / (float)(R - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] +
                     momentum * var_unb;
  }
}

// --------------------------------------------------------------------
// synchronized BN: the forward and backward above, cut where the
// per-channel sums exist so that they can be all-reduced across ranks.
// sums = [2C+1]: sum(x), sum(x^2), then the row count as one fp32 word
// (summed over ranks it is off by at most 2^-24 relative, below the
// rounding of the sums themselves). bsums = [2C]: sum(dy_eff),
// sum(dy_eff * xhat). The kB2 rows are folded in the order of
// bn_stats_coef_kernel / bn_bwd_coef_kernel: one rank gives their bits.
// --------------------------------------------------------------------
__global__ void bn_sync_fold_kernel(
    const float* __restrict__ partial2, float* __restrict__ sums, int C,
    float count, bool with_count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long b2C = (long)kB2 * C;
  float s = 0.f, s2 = 0.f;
  #pragma unroll
  for (int b = 0; b < kB2; ++b) {
    s += partial2[(long)b * C + c];
    s2 += partial2[b2C + (long)b * C + c];
  }
  sums[c] = s;
  sums[C + c] = s2;
  if (with_count && c == 0) sums[2 * C] = count;
}

// bn_stats_coef_kernel on reduced sums, the global row count read from
// the device
__global__ void bn_sync_stats_coef_kernel(
    const float* __restrict__ sums, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ scale_out,
    float* __restrict__ bias_out, int C, float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float R = sums[2 * C];
  const float m = sums[c] / R;
  const float var = fmaxf(sums[C + c] / R - m * m, 0.f);
  const float inv = rsqrtf(var + eps);
  mean_out[c] = m;
  invstd_out[c] = inv;
  const float sc = gamma[c] * inv;
  scale_out[c] = sc;
  bias_out[c] = beta[c] - m * sc;
  if (running_mean != nullptr) {
    const float var_unb = R > 1.f ? var * R / (R - 1.f) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] +
                     momentum * var_unb;
  }
}

// bn_bwd_coef_kernel on reduced sums; dgamma/dbeta stay the caller's
// local sums
__global__ void bn_sync_bwd_coef_kernel(
    const float* __restrict__ bsums, const float* __restrict__ count,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ coefP,
    float* __restrict__ coefQ, float* __restrict__ coefS, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float dsum = bsums[c];
  const float dxhat = bsums[C + c];
  const float invR = 1.f / count[0];
  const float P = gamma[c] * invstd[c];
  const float Q = -P * invstd[c] * dxhat * invR;
  coefP[c] = P;
  coefQ[c] = Q;
  coefS[c] = -P * dsum * invR - Q * mean[c];
}

// eval mode: scale/bias straight from running stats
__global__ void bn_eval_coef_kernel(
    const float* __restrict__ running_mean,
    const float* __restrict__ running_var,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ scale_out, float* __restrict__ bias_out, int C,
    float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float inv = rsqrtf(running_var[c] + eps);
  const float sc = gamma[c] * inv;
  scale_out[c] = sc;
  bias_out[c] = beta[c] - running_mean[c] * sc;
}

// --------------------------------------------------------------------
// apply: y = [relu](scale*x + bias [+ res])
// --------------------------------------------------------------------
template <typename T, bool RELU, bool RES, bool WMASK>
__global__ __launch_bounds__(kT) void bn_apply_kernel(
    const T* __restrict__ x, T* __restrict__ y,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const T* __restrict__ res, unsigned char* __restrict__ mask,
    long total, int C) {
  constexpr int V = BnVec<T>::V;
  const long stride = (long)gridDim.x * kT;
  const long nvec = total / V;
  for (long vi = (long)blockIdx.x * kT + threadIdx.x; vi < nvec;
       vi += stride) {
    const long idx = vi * V;
    const int c0 = (int)(idx % C);
    T xv[V];
    load_vec<T, V>(xv, x + idx);
    float sc[V], bi[V];
    load_coef<V>(sc, scale + c0);
    load_coef<V>(bi, bias + c0);
    T rv[V];
    if constexpr (RES) load_vec<T, V>(rv, res + idx);
    T ov[V];
    unsigned int m = 0;
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      float o = sc[i] * bn_tof<T>(xv[i]) + bi[i];
      if constexpr (RES) o += bn_tof<T>(rv[i]);
      if constexpr (RELU) {
        if constexpr (WMASK) m |= (o > 0.f ? 1u : 0u) << i;
        o = fmaxf(o, 0.f);
      }
      ov[i] = bn_fromf<T>(o);
    }
    store_vec<T, V>(y + idx, ov);
    if constexpr (WMASK) mask[vi] = (unsigned char)m;
  }
}

// --------------------------------------------------------------------
// backward stage 1: per-(block, channel) partial sum(dy_eff) and
// sum(dy_eff * xhat); dy_eff = relu ? dy * (y > 0) : dy
// partial layout: [2, nblocks, C]
// --------------------------------------------------------------------
template <typename T, bool RELU>
__global__ __launch_bounds__(kT) void bn_bwd_reduce_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ mask,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ partial,
    long R, int C) {
  constexpr int V = BnVec<T>::V;
  const int tpr = C / V;
  const int rpb = kT / tpr;
  const int slot = threadIdx.x % tpr;
  const int row_in_block = threadIdx.x / tpr;
  const int c0 = slot * V;

  float mu[V], is[V];
  load_coef<V>(mu, mean + c0);
  load_coef<V>(is, invstd + c0);

  float a0[V], a1[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a1[i] = 0.f; }

  const long row_stride = (long)gridDim.x * rpb;
  for (long r = (long)blockIdx.x * rpb + row_in_block; r < R;
       r += row_stride) {
    T dv[V], xv[V];
    load_vec<T, V>(dv, dy + r * C + c0);
    load_vec<T, V>(xv, x + r * C + c0);
    unsigned int m = 0xffu;
    if constexpr (RELU) m = mask[(r * C + c0) / V];
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      float d = bn_tof<T>(dv[i]);
      if constexpr (RELU) d = (m >> i) & 1u ? d : 0.f;
      const float xh = (bn_tof<T>(xv[i]) - mu[i]) * is[i];
      a0[i] += d;
      a1[i] += d * xh;
    }
  }

  __shared__ float lds[kT * BnVec<T>::V];
  const long nbC = (long)gridDim.x * C;
  for (int pass = 0; pass < 2; ++pass) {
    #pragma unroll
    for (int i = 0; i < V; ++i)
      lds[threadIdx.x * V + i] = pass ? a1[i] : a0[i];
    __syncthreads();
    for (int s = rpb / 2; s > 0; s >>= 1) {
      if (row_in_block < s) {
        #pragma unroll
        for (int i = 0; i < V; ++i)
          lds[threadIdx.x * V + i] +=
              lds[(threadIdx.x + s * tpr) * V + i];
      }
      __syncthreads();
    }
    if (row_in_block == 0) {
      #pragma unroll
      for (int i = 0; i < V; ++i)
        partial[pass * nbC + (long)blockIdx.x * C + c0 + i] =
            lds[threadIdx.x * V + i];
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------
// backward stage 2: fold partials -> dgamma/dbeta and the three
// per-channel dx coefficients:
//   dx = P*dy_eff + Q*x + S
//   P = gamma*invstd
//   Q = -P * invstd * (dxhat_sum/R)
//   S = -P * (dsum/R) - Q * mean
// --------------------------------------------------------------------
__global__ void bn_bwd_coef_kernel(
    const float* __restrict__ partial2,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ coefP,
    float* __restrict__ coefQ, float* __restrict__ coefS, long R,
    int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long b2C = (long)kB2 * C;
  float dsum = 0.f, dxhat = 0.f;
  #pragma unroll
  for (int b = 0; b < kB2; ++b) {
    dsum += partial2[(long)b * C + c];
    dxhat += partial2[b2C + (long)b * C + c];
  }
  dbeta[c] = dsum;
  dgamma[c] = dxhat;
  const float invR = 1.f / (float)R;
  const float P = gamma[c] * invstd[c];
  const float Q = -P * invstd[c] * dxhat * invR;
  coefP[c] = P;
  coefQ[c] = Q;
  coefS[c] = -P * dsum * invR - Q * mean[c];
}

// --------------------------------------------------------------------
// backward dx elementwise: dx = P*dy_eff + Q*x + S [, dres = dy_eff]
// --------------------------------------------------------------------
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(kT) void bn_bwd_dx_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ mask,
    const T* __restrict__ x, const float* __restrict__ coefP,
    const float* __restrict__ coefQ, const float* __restrict__ coefS,
    T* __restrict__ dx, T* __restrict__ dres, long total, int C) {
  constexpr int V = BnVec<T>::V;
  const long stride = (long)gridDim.x * kT;
  const long nvec = total / V;
  for (long vi = (long)blockIdx.x * kT + threadIdx.x; vi < nvec;
       vi += stride) {
    const long idx = vi * V;
    const int c0 = (int)(idx % C);
    T dv[V], xv[V];
    load_vec<T, V>(dv, dy + idx);
    load_vec<T, V>(xv, x + idx);
    unsigned int m = 0xffu;
    if constexpr (RELU) m = mask[vi];
    float P[V], Q[V], S[V];
    load_coef<V>(P, coefP + c0);
    load_coef<V>(Q, coefQ + c0);
    load_coef<V>(S, coefS + c0);
    T dxv[V], drv[V];
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      float d = bn_tof<T>(dv[i]);
      if constexpr (RELU) d = (m >> i) & 1u ? d : 0.f;
      if constexpr (RES) drv[i] = bn_fromf<T>(d);
      dxv[i] = bn_fromf<T>(P[i] * d + Q[i] * bn_tof<T>(xv[i]) + S[i]);
    }
    store_vec<T, V>(dx + idx, dxv);
    if constexpr (RES) store_vec<T, V>(dres + idx, drv);
  }
}

// fold one per-thread accumulator across the rpb rows of a block that
// share a channel slot and store the block's row of a partial plane
// (the LDS tree of bn_stats_kernel / bn_bwd_reduce_kernel)
template <int V>
__device__ __forceinline__ void bn_block_fold(
    float* __restrict__ lds, const float (&a)[V],
    float* __restrict__ plane_row, int tpr, int rpb, int row_in_block) {
  #pragma unroll
  for (int i = 0; i < V; ++i) lds[threadIdx.x * V + i] = a[i];
  __syncthreads();
  for (int s = rpb / 2; s > 0; s >>= 1) {
    if (row_in_block < s) {
      #pragma unroll
      for (int i = 0; i < V; ++i)
        lds[threadIdx.x * V + i] += lds[(threadIdx.x + s * tpr) * V + i];
    }
    __syncthreads();
  }
  if (row_in_block == 0) {
    #pragma unroll
    for (int i = 0; i < V; ++i) plane_row[i] = lds[threadIdx.x * V + i];
  }
  __syncthreads();
}

// ====================================================================
// BN + ReLU + MaxPool(3, stride 2, pad 1): the ResNet stem. The
// full-resolution BN output is never written; backward gathers the
// pooled gradient through a 4-bit argmax code per pooled element.
// ====================================================================
constexpr unsigned kPoolDead = 15u;  // code: window max <= 0

// apply+pool: one thread per (n, oh, ow, V channels). Every in-bounds
// tap is y = round_to_T(max(sc*x+bi, 0)) exactly as bn_apply_kernel
// computes it; the first maximum in (kh, kw) scan order wins (ATen's
// tie rule). Padding taps are skipped. code word: 4 bits per channel.
template <typename T>
__global__ __launch_bounds__(kT) void bn_relu_pool_apply_kernel(
    const T* __restrict__ x, T* __restrict__ pooled,
    unsigned int* __restrict__ code, const float* __restrict__ scale,
    const float* __restrict__ bias, unsigned int nvec, int H, int W,
    int OH, int OW, int C) {
  constexpr int V = BnVec<T>::V;
  const unsigned int tpr = C / V;
  const unsigned int stride = gridDim.x * kT;
  for (unsigned int vi = blockIdx.x * kT + threadIdx.x; vi < nvec;
       vi += stride) {
    const unsigned int opix = vi / tpr;
    const int c0 = (int)(vi - opix * tpr) * V;
    const unsigned int orow = opix / OW;   // n * OH + oh
    const int ow = (int)(opix - orow * OW);
    const unsigned int n = orow / OH;
    const int oh = (int)(orow - n * OH);
    float sc[V], bi[V];
    load_coef<V>(sc, scale + c0);
    load_coef<V>(bi, bias + c0);
    float best[V];
    unsigned int tap_of[V];
    #pragma unroll
    for (int i = 0; i < V; ++i) { best[i] = -1.f; tap_of[i] = 0; }
    #pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = 2 * oh - 1 + kh;
      #pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = 2 * ow - 1 + kw;
        if (h < 0 || h >= H || w < 0 || w >= W) continue;
        T xv[V];
        load_vec<T, V>(xv, x + (((long)n * H + h) * W + w) * C + c0);
        #pragma unroll
        for (int i = 0; i < V; ++i) {
          const float o = sc[i] * bn_tof<T>(xv[i]) + bi[i];
          const float yv = bn_tof<T>(bn_fromf<T>(fmaxf(o, 0.f)));
          // y >= 0 > -1: the first in-bounds tap always takes the slot
          if (yv > best[i]) { best[i] = yv; tap_of[i] = kh * 3 + kw; }
        }
      }
    }
    T ov[V];
    unsigned int word = 0;
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      ov[i] = bn_fromf<T>(best[i]);
      word |= (best[i] > 0.f ? tap_of[i] : kPoolDead) << (4 * i);
    }
    store_vec<T, V>(pooled + (long)opix * C + c0, ov);
    code[vi] = word;
  }
}

// dy_eff of the BN output at input position (h, w): the pooled
// gradients of the (at most 2x2) windows whose argmax this position
// is, summed in fp32 in (oh, ow) order and rounded to T as ATen's
// maxpool backward hands them on. A dead window adds nothing (ReLU).
template <typename T>
__device__ __forceinline__ void bn_pool_gather_dy(
    float (&d)[BnVec<T>::V], const T* __restrict__ dpool,
    const unsigned int* __restrict__ code, long obase, int h, int w,
    int OH, int OW, int C, int tpr, int slot) {
  constexpr int V = BnVec<T>::V;
  #pragma unroll
  for (int i = 0; i < V; ++i) d[i] = 0.f;
  // even h lies in window h/2 only (kh = 1); odd h in (h-1)/2 (kh = 2)
  // and (h+1)/2 (kh = 0)
  // All four windows are loaded unconditionally, at clamped in-bounds
  // addresses, so the loads overlap and lanes of mixed w parity do not
  // diverge; a window that does not cover (h, w) gets a tap no 4-bit
  // code equals.
  #pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int oh_raw = (h >> 1) + a;
    const bool va = a <= (h & 1) && oh_raw < OH;
    const int oh = va ? oh_raw : (h >> 1);
    const int kh = h - 2 * oh + 1;
    #pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ow_raw = (w >> 1) + b;
      const bool vb = b <= (w & 1) && ow_raw < OW;
      const int ow = vb ? ow_raw : (w >> 1);
      const unsigned int tap = (va && vb)
          ? (unsigned int)(kh * 3 + (w - 2 * ow + 1)) : 0xffu;
      const long o = obase + (long)oh * OW + ow;
      const unsigned int word = code[o * tpr + slot];
      T gv[V];
      load_vec<T, V>(gv, dpool + o * C + slot * V);
      #pragma unroll
      for (int i = 0; i < V; ++i)
        d[i] += ((word >> (4 * i)) & 15u) == tap ? bn_tof<T>(gv[i]) : 0.f;
    }
  }
  #pragma unroll
  for (int i = 0; i < V; ++i) d[i] = bn_tof<T>(bn_fromf<T>(d[i]));
}

// backward stage 1 over the stem input. Rows go to blocks and threads
// exactly as in bn_bwd_reduce_kernel, so the partials, and with them
// dgamma, dbeta and dx, are bit for bit what that kernel gives on the
// materialised maxpool gradient. (n, h, w) of a row is stepped along
// with r: no per-row division. partial layout: [2, nblocks, C]
template <typename T>
__global__ __launch_bounds__(kT) void bn_pool_bwd_reduce_kernel(
    const T* __restrict__ dpool, const unsigned int* __restrict__ code,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ partial,
    long R, int H, int W, int OH, int OW, int C) {
  constexpr int V = BnVec<T>::V;
  const int tpr = C / V;
  const int rpb = kT / tpr;
  const int slot = threadIdx.x % tpr;
  const int row_in_block = threadIdx.x / tpr;
  const int c0 = slot * V;

  float mu[V], is[V];
  load_coef<V>(mu, mean + c0);
  load_coef<V>(is, invstd + c0);
  float a0[V], a1[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a1[i] = 0.f; }

  const long row_stride = (long)gridDim.x * rpb;
  long r = (long)blockIdx.x * rpb + row_in_block;
  int w = (int)(r % W);
  int h = (int)((r / W) % H);
  long n = r / W / H;
  const int dw = (int)(row_stride % W);
  const int dh = (int)((row_stride / W) % H);
  const long dn = row_stride / W / H;
  for (; r < R; r += row_stride) {
    T xv[V];
    load_vec<T, V>(xv, x + r * C + c0);
    float d[V];
    bn_pool_gather_dy<T>(d, dpool, code, n * OH * OW, h, w, OH, OW, C,
                         tpr, slot);
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      const float xh = (bn_tof<T>(xv[i]) - mu[i]) * is[i];
      a0[i] += d[i];
      a1[i] += d[i] * xh;
    }
    // (n, h, w) += row_stride, with carries
    w += dw;
    if (w >= W) { w -= W; ++h; }
    h += dh;
    if (h >= H) { h -= H; ++n; }
    n += dn;
  }

  __shared__ float lds[kT * BnVec<T>::V];
  const long nbC = (long)gridDim.x * C;
  float* row = partial + (long)blockIdx.x * C + c0;
  bn_block_fold<V>(lds, a0, row, tpr, rpb, row_in_block);
  bn_block_fold<V>(lds, a1, row + nbC, tpr, rpb, row_in_block);
}

// backward dx over the stem input: dx = P*dy_eff + Q*x + S
template <typename T>
__global__ __launch_bounds__(kT) void bn_pool_bwd_dx_kernel(
    const T* __restrict__ dpool, const unsigned int* __restrict__ code,
    const T* __restrict__ x, const float* __restrict__ coefP,
    const float* __restrict__ coefQ, const float* __restrict__ coefS,
    T* __restrict__ dx, int lines, int H, int W, int OH, int OW,
    int C) {
  constexpr int V = BnVec<T>::V;
  const int tpr = C / V;
  const int rpb = kT / tpr;
  const int slot = threadIdx.x % tpr;
  const int row_in_block = threadIdx.x / tpr;
  const int c0 = slot * V;
  if (row_in_block >= rpb) return;  // C/V not a divisor of kT
  float P[V], Q[V], S[V];
  load_coef<V>(P, coefP + c0);
  load_coef<V>(Q, coefQ + c0);
  load_coef<V>(S, coefS + c0);
  for (int line = blockIdx.x; line < lines; line += gridDim.x) {
    const int n = line / H;
    const int h = line - n * H;
    const long obase = (long)n * OH * OW;
    for (int w = row_in_block; w < W; w += rpb) {
      const long idx = ((long)line * W + w) * C + c0;
      T xv[V];
      load_vec<T, V>(xv, x + idx);
      float d[V];
      bn_pool_gather_dy<T>(d, dpool, code, obase, h, w, OH, OW, C, tpr,
                           slot);
      T dxv[V];
      #pragma unroll
      for (int i = 0; i < V; ++i)
        dxv[i] = bn_fromf<T>(P[i] * d[i] + Q[i] * bn_tof<T>(xv[i]) +
                             S[i]);
      store_vec<T, V>(dx + idx, dxv);
    }
  }
}

// ====================================================================
// dual BN + ReLU for the downsample junction:
//   y = relu(bn3(x3) + bn_ds(xd))
// The identity branch's BN output and its gradient never reach memory.
// ====================================================================
// The identity term is rounded to T before the add, as the composed
// pair of kernels rounds it when it stores `identity`.
template <typename T>
__global__ __launch_bounds__(kT) void bn_dual_apply_kernel(
    const T* __restrict__ x3, const T* __restrict__ xd,
    T* __restrict__ y, const float* __restrict__ scale3,
    const float* __restrict__ bias3, const float* __restrict__ scaled,
    const float* __restrict__ biasd, unsigned char* __restrict__ mask,
    long total, int C) {
  constexpr int V = BnVec<T>::V;
  const long stride = (long)gridDim.x * kT;
  const long nvec = total / V;
  for (long vi = (long)blockIdx.x * kT + threadIdx.x; vi < nvec;
       vi += stride) {
    const long idx = vi * V;
    const int c0 = (int)(idx % C);
    T av[V], bv[V];
    load_vec<T, V>(av, x3 + idx);
    load_vec<T, V>(bv, xd + idx);
    float s3[V], b3[V], sd[V], bd[V];
    load_coef<V>(s3, scale3 + c0);
    load_coef<V>(b3, bias3 + c0);
    load_coef<V>(sd, scaled + c0);
    load_coef<V>(bd, biasd + c0);
    T ov[V];
    unsigned int m = 0;
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      const float idn = sd[i] * bn_tof<T>(bv[i]) + bd[i];
      float o = s3[i] * bn_tof<T>(av[i]) + b3[i];
      o += bn_tof<T>(bn_fromf<T>(idn));
      m |= (o > 0.f ? 1u : 0u) << i;
      ov[i] = bn_fromf<T>(fmaxf(o, 0.f));
    }
    store_vec<T, V>(y + idx, ov);
    mask[vi] = (unsigned char)m;
  }
}

// backward stage 1 for both BNs in one pass over dy, mask, x3, xd.
// dy_eff = dy * mask is a T value already, so the downsample BN sees
// what it saw as `dres`. partial layout: [4, nblocks, C] =
// (sum d, sum d*xhat3, sum d, sum d*xhatd): two [2, nblocks, C] halves
// for bn_fold2_kernel.
template <typename T>
__global__ __launch_bounds__(kT) void bn_dual_bwd_reduce_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ mask,
    const T* __restrict__ x3, const T* __restrict__ xd,
    const float* __restrict__ mean3, const float* __restrict__ invstd3,
    const float* __restrict__ meand, const float* __restrict__ invstdd,
    float* __restrict__ partial, long R, int C) {
  constexpr int V = BnVec<T>::V;
  const int tpr = C / V;
  const int rpb = kT / tpr;
  const int slot = threadIdx.x % tpr;
  const int row_in_block = threadIdx.x / tpr;
  const int c0 = slot * V;

  float mu3[V], is3[V], mud[V], isd[V];
  load_coef<V>(mu3, mean3 + c0);
  load_coef<V>(is3, invstd3 + c0);
  load_coef<V>(mud, meand + c0);
  load_coef<V>(isd, invstdd + c0);
  float a0[V], a3[V], ad[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a3[i] = 0.f; ad[i] = 0.f; }

  const long row_stride = (long)gridDim.x * rpb;
  for (long r = (long)blockIdx.x * rpb + row_in_block; r < R;
       r += row_stride) {
    T dv[V], av[V], bv[V];
    load_vec<T, V>(dv, dy + r * C + c0);
    load_vec<T, V>(av, x3 + r * C + c0);
    load_vec<T, V>(bv, xd + r * C + c0);
    const unsigned int m = mask[(r * C + c0) / V];
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      const float d = (m >> i) & 1u ? bn_tof<T>(dv[i]) : 0.f;
      a0[i] += d;
      a3[i] += d * ((bn_tof<T>(av[i]) - mu3[i]) * is3[i]);
      ad[i] += d * ((bn_tof<T>(bv[i]) - mud[i]) * isd[i]);
    }
  }

  __shared__ float lds[kT * BnVec<T>::V];
  const long nbC = (long)gridDim.x * C;
  float* row = partial + (long)blockIdx.x * C + c0;
  bn_block_fold<V>(lds, a0, row, tpr, rpb, row_in_block);
  bn_block_fold<V>(lds, a3, row + nbC, tpr, rpb, row_in_block);
  bn_block_fold<V>(lds, a0, row + 2 * nbC, tpr, rpb, row_in_block);
  bn_block_fold<V>(lds, ad, row + 3 * nbC, tpr, rpb, row_in_block);
}

// backward dx for both BNs: dx3 = P3*d + Q3*x3 + S3, dxd likewise
template <typename T>
__global__ __launch_bounds__(kT) void bn_dual_bwd_dx_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ mask,
    const T* __restrict__ x3, const T* __restrict__ xd,
    const float* __restrict__ coef3, const float* __restrict__ coefd,
    T* __restrict__ dx3, T* __restrict__ dxd, long total, int C) {
  // coef3 / coefd: [3, C] = P, Q, S
  constexpr int V = BnVec<T>::V;
  const long stride = (long)gridDim.x * kT;
  const long nvec = total / V;
  for (long vi = (long)blockIdx.x * kT + threadIdx.x; vi < nvec;
       vi += stride) {
    const long idx = vi * V;
    const int c0 = (int)(idx % C);
    T dv[V], av[V], bv[V];
    load_vec<T, V>(dv, dy + idx);
    load_vec<T, V>(av, x3 + idx);
    load_vec<T, V>(bv, xd + idx);
    const unsigned int m = mask[vi];
    float P[V], Q[V], S[V];
    load_coef<V>(P, coef3 + c0);
    load_coef<V>(Q, coef3 + C + c0);
    load_coef<V>(S, coef3 + 2 * C + c0);
    float d[V];
    T o3[V], od[V];
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      d[i] = (m >> i) & 1u ? bn_tof<T>(dv[i]) : 0.f;
      o3[i] = bn_fromf<T>(P[i] * d[i] + Q[i] * bn_tof<T>(av[i]) + S[i]);
    }
    store_vec<T, V>(dx3 + idx, o3);
    load_coef<V>(P, coefd + c0);
    load_coef<V>(Q, coefd + C + c0);
    load_coef<V>(S, coefd + 2 * C + c0);
    #pragma unroll
    for (int i = 0; i < V; ++i)
      od[i] = bn_fromf<T>(P[i] * d[i] + Q[i] * bn_tof<T>(bv[i]) + S[i]);
    store_vec<T, V>(dxd + idx, od);
  }
}

int bn_grid_rows(long R, int rpb) {
  long blocks = (R + rpb - 1) / rpb;
  return (int)std::min<long>(std::max<long>(blocks, 1), kMaxStage1);
}

long bn_grid_elems(long nvec) {
  long blocks = (nvec + kT - 1) / kT;
  return std::min<long>(std::max<long>(blocks, 1), 16384);
}

// stats -> fold: the [2, kB2, C] second-level partials of sum / sumsq
template <typename T>
torch::Tensor bn_stats_partial2(const torch::Tensor& x,
                                const at::TensorOptions& opts, long R,
                                int C, hipStream_t stream) {
  const int tpr = C / BnVec<T>::V;
  const int rpb = kT / tpr;
  const int nb = bn_grid_rows(R, rpb);
  auto partial = torch::empty({2, nb, C}, opts);
  auto partial2 = torch::empty({2, kB2, C}, opts);
  hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(nb), dim3(kT), 0,
                     stream,
                     reinterpret_cast<const T*>(x.data_ptr()),
                     partial.data_ptr<float>(), R, C);
  CHECK_HIP_BN(hipGetLastError());
  hipLaunchKernelGGL(bn_fold2_kernel,
                     dim3((C + kFoldC - 1) / kFoldC, kB2), dim3(kT), 0,
                     stream, partial.data_ptr<float>(), nb,
                     partial2.data_ptr<float>(), C);
  CHECK_HIP_BN(hipGetLastError());
  return partial2;
}

// training-mode stats -> fold -> coef: batch mean/invstd, the apply
// pass's scale/bias, and the running-stat update
template <typename T>
void bn_train_coefs(const torch::Tensor& x, const torch::Tensor& gamma,
                    const torch::Tensor& beta,
                    torch::Tensor& running_mean,
                    torch::Tensor& running_var, torch::Tensor& mean,
                    torch::Tensor& invstd, torch::Tensor& scale,
                    torch::Tensor& bias, double momentum, double eps,
                    long R, int C, hipStream_t stream) {
  torch::Tensor partial2 = bn_stats_partial2<T>(
      x, gamma.options().dtype(at::kFloat), R, C, stream);
  hipLaunchKernelGGL(bn_stats_coef_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, partial2.data_ptr<float>(),
                     gamma.data_ptr<float>(),
                     beta.data_ptr<float>(),
                     running_mean.defined()
                         ? running_mean.data_ptr<float>() : nullptr,
                     running_var.defined()
                         ? running_var.data_ptr<float>() : nullptr,
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     scale.data_ptr<float>(), bias.data_ptr<float>(),
                     R, C, (float)momentum, (float)eps);
  CHECK_HIP_BN(hipGetLastError());
}

// the elementwise forward pass: y = [relu](scale*x + bias [+ res])
template <typename T>
void bn_launch_apply(const torch::Tensor& x, torch::Tensor& y,
                     const torch::Tensor& scale,
                     const torch::Tensor& bias,
                     const c10::optional<torch::Tensor>& res,
                     torch::Tensor& mask, bool relu, long R, int C,
                     hipStream_t stream) {
  const long total = R * (long)C;
  const long grid = bn_grid_elems(total / BnVec<T>::V);
  const T* resp = res.has_value()
      ? reinterpret_cast<const T*>(res->data_ptr()) : nullptr;
  unsigned char* mp = mask.defined()
      ? mask.data_ptr<unsigned char>() : nullptr;
  #define APPLY(RELU_, RES_, WM_)                                       \
    hipLaunchKernelGGL((bn_apply_kernel<T, RELU_, RES_, WM_>),          \
                       dim3(grid), dim3(kT), 0, stream,                 \
                       reinterpret_cast<const T*>(x.data_ptr()),        \
                       reinterpret_cast<T*>(y.data_ptr()),              \
                       scale.data_ptr<float>(), bias.data_ptr<float>(), \
                       resp, mp, total, C)
  const bool wm = relu && mp != nullptr;
  if (relu && resp) { if (wm) APPLY(true, true, true);
                      else APPLY(true, true, false); }
  else if (relu) { if (wm) APPLY(true, false, true);
                   else APPLY(true, false, false); }
  else if (resp) APPLY(false, true, false);
  else APPLY(false, false, false);
  #undef APPLY
  CHECK_HIP_BN(hipGetLastError());
}

template <typename T>
void bn_fwd_impl(const torch::Tensor& x, torch::Tensor& y,
                 const torch::Tensor& gamma, const torch::Tensor& beta,
                 torch::Tensor& running_mean, torch::Tensor& running_var,
                 torch::Tensor& mean, torch::Tensor& invstd,
                 const c10::optional<torch::Tensor>& res,
                 torch::Tensor& mask, bool relu,
                 bool training, double momentum, double eps, long R,
                 int C, hipStream_t stream) {
  auto opts = gamma.options().dtype(at::kFloat);
  auto scale = torch::empty({C}, opts);
  auto bias = torch::empty({C}, opts);
  if (training) {
    bn_train_coefs<T>(x, gamma, beta, running_mean, running_var, mean,
                      invstd, scale, bias, momentum, eps, R, C, stream);
  } else {
    hipLaunchKernelGGL(bn_eval_coef_kernel, dim3((C + 255) / 256),
                       dim3(256), 0, stream,
                       running_mean.data_ptr<float>(),
                       running_var.data_ptr<float>(),
                       gamma.data_ptr<float>(), beta.data_ptr<float>(),
                       scale.data_ptr<float>(), bias.data_ptr<float>(),
                       C, (float)eps);
    CHECK_HIP_BN(hipGetLastError());
  }
  bn_launch_apply<T>(x, y, scale, bias, res, mask, relu, R, C, stream);
}

// backward reduce -> fold: the [2, kB2, C] second-level partials of
// sum(dy_eff) / sum(dy_eff * xhat)
template <typename T>
torch::Tensor bn_bwd_partial2(const torch::Tensor& dy,
                              const torch::Tensor& mask,
                              const torch::Tensor& x,
                              const torch::Tensor& mean,
                              const torch::Tensor& invstd, bool relu,
                              long R, int C, hipStream_t stream) {
  const int tpr = C / BnVec<T>::V;
  const int rpb = kT / tpr;
  const int nb = bn_grid_rows(R, rpb);
  auto fopts = mean.options().dtype(at::kFloat);
  auto partial = torch::empty({2, nb, C}, fopts);
  auto partial2 = torch::empty({2, kB2, C}, fopts);
  const unsigned char* mp = mask.defined()
      ? mask.data_ptr<unsigned char>() : nullptr;
  #define RED(RELU_)                                                     \
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, RELU_>), dim3(nb),       \
                       dim3(kT), 0, stream,                              \
                       reinterpret_cast<const T*>(dy.data_ptr()),        \
                       mp,                                               \
                       reinterpret_cast<const T*>(x.data_ptr()),         \
                       mean.data_ptr<float>(), invstd.data_ptr<float>(), \
                       partial.data_ptr<float>(), R, C)
  if (relu) RED(true); else RED(false);
  #undef RED
  CHECK_HIP_BN(hipGetLastError());
  hipLaunchKernelGGL(bn_fold2_kernel,
                     dim3((C + kFoldC - 1) / kFoldC, kB2), dim3(kT), 0,
                     stream, partial.data_ptr<float>(), nb,
                     partial2.data_ptr<float>(), C);
  CHECK_HIP_BN(hipGetLastError());
  return partial2;
}

// the elementwise backward pass: dx = P*dy_eff + Q*x + S [, dres]
template <typename T>
void bn_launch_bwd_dx(const torch::Tensor& dy, const torch::Tensor& mask,
                      const torch::Tensor& x, const torch::Tensor& coefP,
                      const torch::Tensor& coefQ,
                      const torch::Tensor& coefS, torch::Tensor& dx,
                      const c10::optional<torch::Tensor>& dres, bool relu,
                      long R, int C, hipStream_t stream) {
  const unsigned char* mp = mask.defined()
      ? mask.data_ptr<unsigned char>() : nullptr;
  const long total = R * (long)C;
  const long grid = bn_grid_elems(total / BnVec<T>::V);
  T* dresp = dres.has_value()
      ? reinterpret_cast<T*>(dres->data_ptr()) : nullptr;
  #define DX(RELU_, RES_)                                                \
    hipLaunchKernelGGL((bn_bwd_dx_kernel<T, RELU_, RES_>), dim3(grid),   \
                       dim3(kT), 0, stream,                              \
                       reinterpret_cast<const T*>(dy.data_ptr()),        \
                       mp,                                               \
                       reinterpret_cast<const T*>(x.data_ptr()),         \
                       coefP.data_ptr<float>(), coefQ.data_ptr<float>(), \
                       coefS.data_ptr<float>(),                          \
                       reinterpret_cast<T*>(dx.data_ptr()), dresp,       \
                       total, C)
  if (relu && dresp) DX(true, true);
  else if (relu) DX(true, false);
  else if (dresp) DX(false, true);
  else DX(false, false);
  #undef DX
  CHECK_HIP_BN(hipGetLastError());
}

template <typename T>
void bn_bwd_impl(const torch::Tensor& dy, const torch::Tensor& mask,
                 const torch::Tensor& x, const torch::Tensor& mean,
                 const torch::Tensor& invstd, const torch::Tensor& gamma,
                 torch::Tensor& dx, torch::Tensor& dgamma,
                 torch::Tensor& dbeta,
                 const c10::optional<torch::Tensor>& dres, bool relu,
                 long R, int C, hipStream_t stream) {
  auto fopts = gamma.options().dtype(at::kFloat);
  torch::Tensor partial2 = bn_bwd_partial2<T>(dy, mask, x, mean, invstd,
                                              relu, R, C, stream);
  auto coefP = torch::empty({C}, fopts);
  auto coefQ = torch::empty({C}, fopts);
  auto coefS = torch::empty({C}, fopts);
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, partial2.data_ptr<float>(),
                     gamma.data_ptr<float>(), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), dgamma.data_ptr<float>(),
                     dbeta.data_ptr<float>(), coefP.data_ptr<float>(),
                     coefQ.data_ptr<float>(), coefS.data_ptr<float>(), R,
                     C);
  CHECK_HIP_BN(hipGetLastError());
  bn_launch_bwd_dx<T>(dy, mask, x, coefP, coefQ, coefS, dx, dres, relu, R,
                      C, stream);
}

// backward fold -> coef for one BN from its [2, nb, C] partial:
// dgamma/dbeta and coef = [3, C] (P, Q, S)
void bn_bwd_fold_coefs(const float* partial, int nb,
                       const torch::Tensor& gamma,
                       const torch::Tensor& mean,
                       const torch::Tensor& invstd, torch::Tensor& dgamma,
                       torch::Tensor& dbeta, torch::Tensor& coef, long R,
                       int C, hipStream_t stream) {
  auto partial2 = torch::empty({2, kB2, C}, coef.options());
  hipLaunchKernelGGL(bn_fold2_kernel,
                     dim3((C + kFoldC - 1) / kFoldC, kB2), dim3(kT), 0,
                     stream, partial, nb, partial2.data_ptr<float>(), C);
  CHECK_HIP_BN(hipGetLastError());
  float* cp = coef.data_ptr<float>();
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, partial2.data_ptr<float>(),
                     gamma.data_ptr<float>(), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), dgamma.data_ptr<float>(),
                     dbeta.data_ptr<float>(), cp, cp + C, cp + 2 * C, R,
                     C);
  CHECK_HIP_BN(hipGetLastError());
}

struct PoolGeom { int N, H, W, OH, OW; };

PoolGeom pool_geom(const torch::Tensor& x) {
  PoolGeom g;
  g.N = (int)x.size(0); g.H = (int)x.size(2); g.W = (int)x.size(3);
  g.OH = (g.H - 1) / 2 + 1;   // kernel 3, stride 2, pad 1, floor mode
  g.OW = (g.W - 1) / 2 + 1;
  return g;
}

template <typename T>
void bn_relu_pool_fwd_impl(const torch::Tensor& x, torch::Tensor& pooled,
                           torch::Tensor& code,
                           const torch::Tensor& gamma,
                           const torch::Tensor& beta,
                           torch::Tensor& running_mean,
                           torch::Tensor& running_var,
                           torch::Tensor& mean, torch::Tensor& invstd,
                           double momentum, double eps, long R, int C,
                           hipStream_t stream) {
  auto opts = gamma.options().dtype(at::kFloat);
  auto scale = torch::empty({C}, opts);
  auto bias = torch::empty({C}, opts);
  bn_train_coefs<T>(x, gamma, beta, running_mean, running_var, mean,
                    invstd, scale, bias, momentum, eps, R, C, stream);
  const PoolGeom g = pool_geom(x);
  const long nvec = code.numel();
  hipLaunchKernelGGL((bn_relu_pool_apply_kernel<T>),
                     dim3(bn_grid_elems(nvec)), dim3(kT), 0, stream,
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<T*>(pooled.data_ptr()),
                     reinterpret_cast<unsigned int*>(code.data_ptr()),
                     scale.data_ptr<float>(), bias.data_ptr<float>(),
                     (unsigned int)nvec, g.H, g.W, g.OH, g.OW, C);
  CHECK_HIP_BN(hipGetLastError());
}

template <typename T>
void bn_relu_pool_bwd_impl(const torch::Tensor& dpool,
                           const torch::Tensor& code,
                           const torch::Tensor& x,
                           const torch::Tensor& mean,
                           const torch::Tensor& invstd,
                           const torch::Tensor& gamma, torch::Tensor& dx,
                           torch::Tensor& dgamma, torch::Tensor& dbeta,
                           long R, int C, hipStream_t stream) {
  const PoolGeom g = pool_geom(x);
  const int lines = g.N * g.H;
  const int nb = bn_grid_rows(R, kT / (C / BnVec<T>::V));
  auto fopts = gamma.options().dtype(at::kFloat);
  auto partial = torch::empty({2, nb, C}, fopts);
  auto coef = torch::empty({3, C}, fopts);
  const T* dp = reinterpret_cast<const T*>(dpool.data_ptr());
  const unsigned int* cp =
      reinterpret_cast<const unsigned int*>(code.data_ptr());
  const T* xp = reinterpret_cast<const T*>(x.data_ptr());
  hipLaunchKernelGGL((bn_pool_bwd_reduce_kernel<T>), dim3(nb), dim3(kT),
                     0, stream, dp, cp, xp, mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), partial.data_ptr<float>(),
                     R, g.H, g.W, g.OH, g.OW, C);
  CHECK_HIP_BN(hipGetLastError());
  bn_bwd_fold_coefs(partial.data_ptr<float>(), nb, gamma, mean, invstd,
                    dgamma, dbeta, coef, R, C, stream);
  const float* cf = coef.data_ptr<float>();
  hipLaunchKernelGGL((bn_pool_bwd_dx_kernel<T>),
                     dim3(std::min(lines, 16384)), dim3(kT), 0, stream,
                     dp, cp, xp, cf, cf + C, cf + 2 * C,
                     reinterpret_cast<T*>(dx.data_ptr()), lines, g.H,
                     g.W, g.OH, g.OW, C);
  CHECK_HIP_BN(hipGetLastError());
}

template <typename T>
void bn_dual_fwd_impl(const torch::Tensor& x3, const torch::Tensor& xd,
                      torch::Tensor& y, torch::Tensor& mask,
                      const torch::Tensor& gamma3,
                      const torch::Tensor& beta3, torch::Tensor& rm3,
                      torch::Tensor& rv3, const torch::Tensor& gammad,
                      const torch::Tensor& betad, torch::Tensor& rmd,
                      torch::Tensor& rvd, torch::Tensor& mean3,
                      torch::Tensor& invstd3, torch::Tensor& meand,
                      torch::Tensor& invstdd, double momentum3,
                      double momentumd, double eps3, double epsd, long R,
                      int C, hipStream_t stream) {
  auto opts = gamma3.options().dtype(at::kFloat);
  auto scale3 = torch::empty({C}, opts);
  auto bias3 = torch::empty({C}, opts);
  auto scaled = torch::empty({C}, opts);
  auto biasd = torch::empty({C}, opts);
  bn_train_coefs<T>(xd, gammad, betad, rmd, rvd, meand, invstdd, scaled,
                    biasd, momentumd, epsd, R, C, stream);
  bn_train_coefs<T>(x3, gamma3, beta3, rm3, rv3, mean3, invstd3, scale3,
                    bias3, momentum3, eps3, R, C, stream);
  const long total = R * (long)C;
  hipLaunchKernelGGL((bn_dual_apply_kernel<T>),
                     dim3(bn_grid_elems(total / BnVec<T>::V)), dim3(kT),
                     0, stream,
                     reinterpret_cast<const T*>(x3.data_ptr()),
                     reinterpret_cast<const T*>(xd.data_ptr()),
                     reinterpret_cast<T*>(y.data_ptr()),
                     scale3.data_ptr<float>(), bias3.data_ptr<float>(),
                     scaled.data_ptr<float>(), biasd.data_ptr<float>(),
                     mask.data_ptr<unsigned char>(), total, C);
  CHECK_HIP_BN(hipGetLastError());
}

template <typename T>
void bn_dual_bwd_impl(const torch::Tensor& dy, const torch::Tensor& mask,
                      const torch::Tensor& x3, const torch::Tensor& xd,
                      const torch::Tensor& mean3,
                      const torch::Tensor& invstd3,
                      const torch::Tensor& gamma3,
                      const torch::Tensor& meand,
                      const torch::Tensor& invstdd,
                      const torch::Tensor& gammad,
                      std::vector<torch::Tensor>& out, long R, int C,
                      hipStream_t stream) {
  // out: dx3, dxd, dgamma3, dbeta3, dgammad, dbetad
  const int tpr = C / BnVec<T>::V;
  const int rpb = kT / tpr;
  const int nb = bn_grid_rows(R, rpb);
  auto fopts = gamma3.options().dtype(at::kFloat);
  auto partial = torch::empty({4, nb, C}, fopts);
  auto coef3 = torch::empty({3, C}, fopts);
  auto coefd = torch::empty({3, C}, fopts);
  const T* dyp = reinterpret_cast<const T*>(dy.data_ptr());
  const unsigned char* mp = mask.data_ptr<unsigned char>();
  const T* x3p = reinterpret_cast<const T*>(x3.data_ptr());
  const T* xdp = reinterpret_cast<const T*>(xd.data_ptr());
  hipLaunchKernelGGL((bn_dual_bwd_reduce_kernel<T>), dim3(nb), dim3(kT),
                     0, stream, dyp, mp, x3p, xdp,
                     mean3.data_ptr<float>(), invstd3.data_ptr<float>(),
                     meand.data_ptr<float>(), invstdd.data_ptr<float>(),
                     partial.data_ptr<float>(), R, C);
  CHECK_HIP_BN(hipGetLastError());
  const float* pp = partial.data_ptr<float>();
  bn_bwd_fold_coefs(pp, nb, gamma3, mean3, invstd3, out[2], out[3],
                    coef3, R, C, stream);
  bn_bwd_fold_coefs(pp + 2 * (long)nb * C, nb, gammad, meand, invstdd,
                    out[4], out[5], coefd, R, C, stream);
  const long total = R * (long)C;
  hipLaunchKernelGGL((bn_dual_bwd_dx_kernel<T>),
                     dim3(bn_grid_elems(total / BnVec<T>::V)), dim3(kT),
                     0, stream, dyp, mp, x3p, xdp,
                     coef3.data_ptr<float>(), coefd.data_ptr<float>(),
                     reinterpret_cast<T*>(out[0].data_ptr()),
                     reinterpret_cast<T*>(out[1].data_ptr()), total, C);
  CHECK_HIP_BN(hipGetLastError());
}

void bn_check_input(const torch::Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, what,
              ": 4-D GPU input expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), what,
              ": channels_last input required");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kFloat, what,
              ": dtype must be bf16 or f32");
  const int C = (int)x.size(1);
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(C % V == 0 && C / V <= kT, what, ": C=", C,
              " unsupported for vec", V);
}

// The sync entry points additionally want C/V to be a power of two:
// only then do the LDS trees of the stage-1 reductions cover every row
// of a block.
void bn_check_sync_input(const torch::Tensor& x, const char* what) {
  bn_check_input(x, what);
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  const int tpr = (int)x.size(1) / V;
  TORCH_CHECK((tpr & (tpr - 1)) == 0, what, ": C/", V,
              " must be a power of two");
  TORCH_CHECK(x.numel() > 0, what, ": empty input");
}

// an fp32 vector of n elements on x's device
void bn_check_vec(const torch::Tensor& t, const torch::Tensor& x, long n,
                  const char* what, const char* name) {
  TORCH_CHECK(t.defined() && t.scalar_type() == at::kFloat &&
              t.device() == x.device() && t.is_contiguous() &&
              t.numel() == n, what, ": ", name, " must be fp32 [", n,
              "] on the input's device");
}

void bn_check_bwd_args(const torch::Tensor& dy, const torch::Tensor& mask,
                       const torch::Tensor& x, const torch::Tensor& mean,
                       const torch::Tensor& invstd, bool relu,
                       const char* what) {
  bn_check_sync_input(x, what);
  const int C = (int)x.size(1);
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(dy.sizes() == x.sizes() &&
              dy.scalar_type() == x.scalar_type() &&
              dy.device() == x.device(), what, ": bad gradient");
  bn_check_vec(mean, x, C, what, "mean");
  bn_check_vec(invstd, x, C, what, "invstd");
  TORCH_CHECK(!relu || (mask.defined() &&
                        mask.scalar_type() == at::kByte &&
                        mask.device() == x.device() &&
                        mask.numel() == x.numel() / V),
              what, ": relu path needs the fwd mask");
}

}  // namespace

// ---- synchronized BN: forward and backward cut where the sums exist.
// No call below waits for the device or reads a value back.

// Returns sums = fp32 [2C+1]: sum(x), sum(x^2) per channel, then the
// row count N*H*W.
torch::Tensor fused_bn_sync_stats(torch::Tensor x) {
  bn_check_sync_input(x, "fused_bn_sync_stats");
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto fopts = x.options().dtype(at::kFloat);
  auto sums = torch::empty({2 * (long)C + 1}, fopts);
  torch::Tensor partial2 = x.scalar_type() == at::kBFloat16
      ? bn_stats_partial2<__hip_bfloat16>(x, fopts, R, C, stream)
      : bn_stats_partial2<float>(x, fopts, R, C, stream);
  hipLaunchKernelGGL(bn_sync_fold_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, partial2.data_ptr<float>(),
                     sums.data_ptr<float>(), C, (float)R, true);
  CHECK_HIP_BN(hipGetLastError());
  return sums;
}

// sums: the all-reduced [2C+1]. Returns (y, mean, invstd, mask); mean
// and invstd are the global batch statistics.
std::vector<torch::Tensor> fused_bn_sync_apply(
    torch::Tensor x, torch::Tensor sums, torch::Tensor gamma,
    torch::Tensor beta, torch::Tensor running_mean,
    torch::Tensor running_var, c10::optional<torch::Tensor> res,
    bool relu, double momentum, double eps) {
  const char* what = "fused_bn_sync_apply";
  bn_check_sync_input(x, what);
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  bn_check_vec(sums, x, 2 * (long)C + 1, what, "sums");
  bn_check_vec(gamma, x, C, what, "gamma");
  bn_check_vec(beta, x, C, what, "beta");
  // an empty tensor stands for "no running stats", as in fused_bn_fwd
  const bool has_running =
      running_mean.defined() && running_mean.numel() > 0;
  TORCH_CHECK(has_running ==
              (running_var.defined() && running_var.numel() > 0), what,
              ": running_mean and running_var go together");
  if (has_running) {
    bn_check_vec(running_mean, x, C, what, "running_mean");
    bn_check_vec(running_var, x, C, what, "running_var");
  }
  if (res.has_value()) {
    TORCH_CHECK(res->is_contiguous(at::MemoryFormat::ChannelsLast) &&
                res->scalar_type() == x.scalar_type() &&
                res->device() == x.device() &&
                res->sizes() == x.sizes(), what, ": bad residual");
  }
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x);
  auto fopts = x.options().dtype(at::kFloat);
  auto mean = torch::empty({C}, fopts);
  auto invstd = torch::empty({C}, fopts);
  auto scale = torch::empty({C}, fopts);
  auto bias = torch::empty({C}, fopts);
  torch::Tensor mask;
  if (relu)
    mask = torch::empty({x.numel() / V}, x.options().dtype(at::kByte));
  hipLaunchKernelGGL(bn_sync_stats_coef_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, sums.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     has_running ? running_mean.data_ptr<float>()
                                 : nullptr,
                     has_running ? running_var.data_ptr<float>()
                                 : nullptr,
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     scale.data_ptr<float>(), bias.data_ptr<float>(), C,
                     (float)momentum, (float)eps);
  CHECK_HIP_BN(hipGetLastError());
  if (x.scalar_type() == at::kBFloat16)
    bn_launch_apply<__hip_bfloat16>(x, y, scale, bias, res, mask, relu, R,
                                    C, stream);
  else
    bn_launch_apply<float>(x, y, scale, bias, res, mask, relu, R, C,
                           stream);
  if (!mask.defined())
    mask = torch::empty({0}, x.options().dtype(at::kByte));
  return {y, mean, invstd, mask};
}

// Returns bsums = fp32 [2C]: sum(dy_eff) (this rank's dbeta), then
// sum(dy_eff * xhat) (its dgamma).
torch::Tensor fused_bn_sync_bwd_reduce(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, bool relu) {
  bn_check_bwd_args(dy, mask, x, mean, invstd, relu,
                    "fused_bn_sync_bwd_reduce");
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto bsums = torch::empty({2 * (long)C}, mean.options());
  torch::Tensor partial2 = x.scalar_type() == at::kBFloat16
      ? bn_bwd_partial2<__hip_bfloat16>(dy, mask, x, mean, invstd, relu,
                                        R, C, stream)
      : bn_bwd_partial2<float>(dy, mask, x, mean, invstd, relu, R, C,
                               stream);
  hipLaunchKernelGGL(bn_sync_fold_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, partial2.data_ptr<float>(),
                     bsums.data_ptr<float>(), C, 0.f, false);
  CHECK_HIP_BN(hipGetLastError());
  return bsums;
}

// bsums: the all-reduced [2C]; count: the 1-element global row count
// (the last word of the forward's reduced sums). Returns (dx[, dres]).
std::vector<torch::Tensor> fused_bn_sync_bwd_dx(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, torch::Tensor gamma,
    torch::Tensor bsums, torch::Tensor count, bool relu, bool has_res) {
  const char* what = "fused_bn_sync_bwd_dx";
  bn_check_bwd_args(dy, mask, x, mean, invstd, relu, what);
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  bn_check_vec(gamma, x, C, what, "gamma");
  bn_check_vec(bsums, x, 2 * (long)C, what, "bsums");
  bn_check_vec(count, x, 1, what, "count");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  auto coefP = torch::empty({C}, mean.options());
  auto coefQ = torch::empty({C}, mean.options());
  auto coefS = torch::empty({C}, mean.options());
  c10::optional<torch::Tensor> dres;
  if (has_res) dres = torch::empty_like(x);
  hipLaunchKernelGGL(bn_sync_bwd_coef_kernel, dim3((C + 255) / 256),
                     dim3(256), 0, stream, bsums.data_ptr<float>(),
                     count.data_ptr<float>(), gamma.data_ptr<float>(),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     coefP.data_ptr<float>(), coefQ.data_ptr<float>(),
                     coefS.data_ptr<float>(), C);
  CHECK_HIP_BN(hipGetLastError());
  if (x.scalar_type() == at::kBFloat16)
    bn_launch_bwd_dx<__hip_bfloat16>(dy, mask, x, coefP, coefQ, coefS, dx,
                                     dres, relu, R, C, stream);
  else
    bn_launch_bwd_dx<float>(dy, mask, x, coefP, coefQ, coefS, dx, dres,
                            relu, R, C, stream);
  std::vector<torch::Tensor> out = {dx};
  if (has_res) out.push_back(*dres);
  return out;
}

// BN(train) + ReLU + MaxPool2d(3, stride 2, pad 1).
// Returns (pooled, save_mean, save_invstd, code); code holds one 32-bit
// word per V channels of a pooled pixel, 4 bits per channel: the
// argmax tap kh*3+kw, or 15 where the window max is <= 0.
std::vector<torch::Tensor> fused_bn_relu_pool_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor running_mean, torch::Tensor running_var,
    double momentum, double eps) {
  bn_check_input(x, "fused_bn_relu_pool");
  // the kernels index pixels and code words in 32 bits
  TORCH_CHECK(x.numel() < (1L << 31), "fused_bn_relu_pool: input too large");
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  const PoolGeom g = pool_geom(x);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto pooled = torch::empty({g.N, C, g.OH, g.OW}, x.options(),
                             at::MemoryFormat::ChannelsLast);
  auto code = torch::empty({(long)g.N * g.OH * g.OW * (C / V)},
                           x.options().dtype(at::kInt));
  auto fopts = gamma.options().dtype(at::kFloat);
  auto mean = torch::empty({C}, fopts);
  auto invstd = torch::empty({C}, fopts);
  if (x.scalar_type() == at::kBFloat16)
    bn_relu_pool_fwd_impl<__hip_bfloat16>(
        x, pooled, code, gamma, beta, running_mean, running_var, mean,
        invstd, momentum, eps, R, C, stream);
  else
    bn_relu_pool_fwd_impl<float>(
        x, pooled, code, gamma, beta, running_mean, running_var, mean,
        invstd, momentum, eps, R, C, stream);
  return {pooled, mean, invstd, code};
}

// Returns (dx, dgamma, dbeta).
std::vector<torch::Tensor> fused_bn_relu_pool_bwd(
    torch::Tensor dpool, torch::Tensor code, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, torch::Tensor gamma) {
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  const PoolGeom g = pool_geom(x);
  TORCH_CHECK(dpool.dim() == 4 && dpool.size(0) == g.N &&
              dpool.size(1) == C && dpool.size(2) == g.OH &&
              dpool.size(3) == g.OW &&
              dpool.scalar_type() == x.scalar_type(),
              "fused_bn_relu_pool_bwd: bad pooled gradient");
  TORCH_CHECK(code.scalar_type() == at::kInt &&
              code.numel() == (long)g.N * g.OH * g.OW * (C / V),
              "fused_bn_relu_pool_bwd: bad code tensor");
  dpool = dpool.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  auto fopts = gamma.options().dtype(at::kFloat);
  auto dgamma = torch::empty({C}, fopts);
  auto dbeta = torch::empty({C}, fopts);
  if (x.scalar_type() == at::kBFloat16)
    bn_relu_pool_bwd_impl<__hip_bfloat16>(dpool, code, x, mean, invstd,
                                          gamma, dx, dgamma, dbeta, R, C,
                                          stream);
  else
    bn_relu_pool_bwd_impl<float>(dpool, code, x, mean, invstd, gamma, dx,
                                 dgamma, dbeta, R, C, stream);
  return {dx, dgamma, dbeta};
}

// y = relu(BN3(x3) + BNd(xd)), both BNs in training mode.
// Returns (y, mean3, invstd3, meand, invstdd, mask).
std::vector<torch::Tensor> fused_bn_dual_fwd(
    torch::Tensor x3, torch::Tensor xd, torch::Tensor gamma3,
    torch::Tensor beta3, torch::Tensor running_mean3,
    torch::Tensor running_var3, torch::Tensor gammad,
    torch::Tensor betad, torch::Tensor running_meand,
    torch::Tensor running_vard, double momentum3, double momentumd,
    double eps3, double epsd) {
  bn_check_input(x3, "fused_bn_dual");
  bn_check_input(xd, "fused_bn_dual");
  TORCH_CHECK(xd.sizes() == x3.sizes() &&
              xd.scalar_type() == x3.scalar_type(),
              "fused_bn_dual: the two inputs must match");
  const int C = (int)x3.size(1);
  const long R = x3.numel() / C;
  const int V = x3.scalar_type() == at::kBFloat16 ? 8 : 4;
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x3);
  auto mask = torch::empty({x3.numel() / V},
                           x3.options().dtype(at::kByte));
  auto fopts = gamma3.options().dtype(at::kFloat);
  auto mean3 = torch::empty({C}, fopts);
  auto invstd3 = torch::empty({C}, fopts);
  auto meand = torch::empty({C}, fopts);
  auto invstdd = torch::empty({C}, fopts);
  if (x3.scalar_type() == at::kBFloat16)
    bn_dual_fwd_impl<__hip_bfloat16>(
        x3, xd, y, mask, gamma3, beta3, running_mean3, running_var3,
        gammad, betad, running_meand, running_vard, mean3, invstd3,
        meand, invstdd, momentum3, momentumd, eps3, epsd, R, C, stream);
  else
    bn_dual_fwd_impl<float>(
        x3, xd, y, mask, gamma3, beta3, running_mean3, running_var3,
        gammad, betad, running_meand, running_vard, mean3, invstd3,
        meand, invstdd, momentum3, momentumd, eps3, epsd, R, C, stream);
  return {y, mean3, invstd3, meand, invstdd, mask};
}

// Returns (dx3, dxd, dgamma3, dbeta3, dgammad, dbetad).
std::vector<torch::Tensor> fused_bn_dual_bwd(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x3,
    torch::Tensor xd, torch::Tensor mean3, torch::Tensor invstd3,
    torch::Tensor gamma3, torch::Tensor meand, torch::Tensor invstdd,
    torch::Tensor gammad) {
  const int C = (int)x3.size(1);
  const long R = x3.numel() / C;
  const int V = x3.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(dy.sizes() == x3.sizes() && xd.sizes() == x3.sizes() &&
              dy.scalar_type() == x3.scalar_type(),
              "fused_bn_dual_bwd: bad gradient");
  TORCH_CHECK(mask.numel() == x3.numel() / V,
              "fused_bn_dual_bwd: needs the fwd mask");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto fopts = gamma3.options().dtype(at::kFloat);
  std::vector<torch::Tensor> out = {
      torch::empty_like(x3), torch::empty_like(xd),
      torch::empty({C}, fopts), torch::empty({C}, fopts),
      torch::empty({C}, fopts), torch::empty({C}, fopts)};
  if (x3.scalar_type() == at::kBFloat16)
    bn_dual_bwd_impl<__hip_bfloat16>(dy, mask, x3, xd, mean3, invstd3,
                                     gamma3, meand, invstdd, gammad, out,
                                     R, C, stream);
  else
    bn_dual_bwd_impl<float>(dy, mask, x3, xd, mean3, invstd3, gamma3,
                            meand, invstdd, gammad, out, R, C, stream);
  return out;
}

// x: [N, C, H, W] channels_last (viewed as [R, C]); gamma/beta fp32.
// Returns (y, save_mean, save_invstd).
std::vector<torch::Tensor> fused_bn_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor running_mean, torch::Tensor running_var,
    c10::optional<torch::Tensor> res, bool relu, bool training,
    double momentum, double eps) {
  TORCH_CHECK(x.dim() == 4, "fused_bn: 4-D input expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "fused_bn: channels_last input required");
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  const int V = x.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(C % V == 0 && C / V <= kT,
              "fused_bn: C=", C, " unsupported for vec", V);
  if (res.has_value()) {
    TORCH_CHECK(res->is_contiguous(at::MemoryFormat::ChannelsLast) &&
                res->scalar_type() == x.scalar_type() &&
                res->sizes() == x.sizes(), "fused_bn: bad residual");
  }
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x);  // keeps channels_last layout
  auto fopts = gamma.options().dtype(at::kFloat);
  auto mean = torch::empty({C}, fopts);
  auto invstd = torch::empty({C}, fopts);
  // ReLU bitmask (1 byte per V elems) replaces re-reading y in
  // backward: ~25% less bwd traffic
  torch::Tensor mask;
  if (relu && training)
    mask = torch::empty({x.numel() / V},
                        x.options().dtype(at::kByte));
  if (x.scalar_type() == at::kBFloat16)
    bn_fwd_impl<__hip_bfloat16>(x, y, gamma, beta, running_mean,
                                running_var, mean, invstd, res, mask,
                                relu, training, momentum, eps, R, C,
                                stream);
  else if (x.scalar_type() == at::kFloat)
    bn_fwd_impl<float>(x, y, gamma, beta, running_mean, running_var,
                       mean, invstd, res, mask, relu, training,
                       momentum, eps, R, C, stream);
  else
    TORCH_CHECK(false, "fused_bn: dtype must be bf16 or f32");
  if (!mask.defined())
    mask = torch::empty({0}, x.options().dtype(at::kByte));
  return {y, mean, invstd, mask};
}

// Returns (dx, dgamma, dbeta[, dres]). mask: ReLU bitmask from fwd
// (empty tensor when relu=false).
std::vector<torch::Tensor> fused_bn_bwd(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, torch::Tensor gamma,
    bool relu, bool has_res) {
  const int C = (int)x.size(1);
  const long R = x.numel() / C;
  TORCH_CHECK(!relu || mask.numel() > 0,
              "fused_bn_bwd: relu path needs the fwd mask");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  auto fopts = gamma.options().dtype(at::kFloat);
  auto dgamma = torch::empty({C}, fopts);
  auto dbeta = torch::empty({C}, fopts);
  c10::optional<torch::Tensor> dres;
  if (has_res) dres = torch::empty_like(x);
  if (x.scalar_type() == at::kBFloat16)
    bn_bwd_impl<__hip_bfloat16>(dy, mask, x, mean, invstd, gamma, dx,
                                dgamma, dbeta, dres, relu, R, C, stream);
  else
    bn_bwd_impl<float>(dy, mask, x, mean, invstd, gamma, dx, dgamma,
                       dbeta, dres, relu, R, C, stream);
  std::vector<torch::Tensor> out = {dx, dgamma, dbeta};
  if (has_res) out.push_back(*dres);
  return out;
}
