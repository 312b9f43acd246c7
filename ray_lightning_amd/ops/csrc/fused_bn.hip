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

// How the kT threads of a stage-1 block cover rows of [R, C]: tpr = C/V
// threads share a row, each with V channels from c0; a block holds
// rpb = kT/tpr rows. The host check admits only a power-of-two
// tpr <= kT, so tpr * rpb == kT and the tree of bn_block_fold, which
// halves rpb, reaches every row of the block.
template <int V>
struct BnRowMap {
  int tpr, rpb, slot, row_in_block, c0;
  __device__ __forceinline__ explicit BnRowMap(int C)
      : tpr(C / V), rpb(kT / tpr), slot(threadIdx.x % tpr),
        row_in_block(threadIdx.x / tpr), c0(slot * V) {}
};

// fold one per-thread accumulator across the rpb rows of a block that
// share a channel slot and store the block's row of a partial plane
template <int V>
__device__ __forceinline__ void bn_block_fold(
    float* __restrict__ lds, const float (&a)[V],
    float* __restrict__ plane_row, const BnRowMap<V>& map) {
  #pragma unroll
  for (int i = 0; i < V; ++i) lds[threadIdx.x * V + i] = a[i];
  __syncthreads();
  for (int s = map.rpb / 2; s > 0; s >>= 1) {
    if (map.row_in_block < s) {
      #pragma unroll
      for (int i = 0; i < V; ++i)
        lds[threadIdx.x * V + i] +=
            lds[(threadIdx.x + s * map.tpr) * V + i];
    }
    __syncthreads();
  }
  if (map.row_in_block == 0) {
    #pragma unroll
    for (int i = 0; i < V; ++i) plane_row[i] = lds[threadIdx.x * V + i];
  }
  __syncthreads();
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
  const BnRowMap<V> map(C);

  float acc[V], acc2[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { acc[i] = 0.f; acc2[i] = 0.f; }

  const long row_stride = (long)gridDim.x * map.rpb;
  for (long r = (long)blockIdx.x * map.rpb + map.row_in_block; r < R;
       r += row_stride) {
    T v[V];
    load_vec<T, V>(v, x + r * C + map.c0);
    #pragma unroll
    for (int i = 0; i < V; ++i) {
      const float f = bn_tof<T>(v[i]);
      acc[i] += f;
      acc2[i] += f * f;
    }
  }

  __shared__ float lds[kT * BnVec<T>::V];
  const long nbC = (long)gridDim.x * C;
  float* row = partial + (long)blockIdx.x * C + map.c0;
  bn_block_fold<V>(lds, acc, row, map);
  bn_block_fold<V>(lds, acc2, row + nbC, map);
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

// the two planes of a [2, kB2, C] second-level partial, folded for
// channel c
__device__ __forceinline__ void bn_fold_b2(
    const float* __restrict__ partial2, int C, int c, float& s,
    float& s2) {
  const long b2C = (long)kB2 * C;
  s = 0.f;
  s2 = 0.f;
  #pragma unroll
  for (int b = 0; b < kB2; ++b) {
    s += partial2[(long)b * C + c];
    s2 += partial2[b2C + (long)b * C + c];
  }
}

// per-channel operands and results of the forward coefficient kernels
struct BnFwdCoef {
  const float* gamma;
  const float* beta;
  float* running_mean;  // null: no running stats
  float* running_var;
  float* mean;
  float* invstd;
  float* scale;
  float* bias;
  float momentum, eps;
};

// mean/invstd, the apply pass's scale/bias and the running-stat update
// of channel c from its sums. Rf is the row count and Rm1 the row count
// less one, each converted to fp32 by the caller in its own way.
__device__ __forceinline__ void bn_fwd_coefs(const BnFwdCoef& a, int c,
                                             float s, float s2, float Rf,
                                             float Rm1) {
  const float m = s / Rf;
  const float var = fmaxf(s2 / Rf - m * m, 0.f);
  const float inv = rsqrtf(var + a.eps);
  a.mean[c] = m;
  a.invstd[c] = inv;
  const float sc = a.gamma[c] * inv;
  a.scale[c] = sc;
  a.bias[c] = a.beta[c] - m * sc;
  if (a.running_mean != nullptr) {
    // unbiased variance for running stats (torch semantics)
    const float var_unb = Rf > 1.f ? var * Rf / Rm1 : var;
    a.running_mean[c] =
        (1.f - a.momentum) * a.running_mean[c] + a.momentum * m;
    a.running_var[c] =
        (1.f - a.momentum) * a.running_var[c] + a.momentum * var_unb;
  }
}

__global__ void bn_stats_coef_kernel(
    const float* __restrict__ partial2, BnFwdCoef a, long R, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s, s2;
  bn_fold_b2(partial2, C, c, s, s2);
  bn_fwd_coefs(a, c, s, s2, (float)R, (float)(R - 1));
}

// --------------------------------------------------------------------
// synchronized BN: the forward and backward, cut where the per-channel
// sums exist so that they can be all-reduced across ranks.
// sums = [2C+1]: sum(x), sum(x^2), then the row count as one fp32 word
// (summed over ranks it is off by at most 2^-24 relative, below the
// rounding of the sums themselves). bsums = [2C]: sum(dy_eff),
// sum(dy_eff * xhat). The kB2 rows are folded and the coefficients
// formed by the device functions of the plain kernels: one rank gives
// their bits.
// --------------------------------------------------------------------
__global__ void bn_sync_fold_kernel(
    const float* __restrict__ partial2, float* __restrict__ sums, int C,
    float count, bool with_count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s, s2;
  bn_fold_b2(partial2, C, c, s, s2);
  sums[c] = s;
  sums[C + c] = s2;
  if (with_count && c == 0) sums[2 * C] = count;
}

// bn_stats_coef_kernel on reduced sums, the global row count read from
// the device
__global__ void bn_sync_stats_coef_kernel(
    const float* __restrict__ sums, BnFwdCoef a, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float R = sums[2 * C];
  bn_fwd_coefs(a, c, sums[c], sums[C + c], R, R - 1.f);
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
  const BnRowMap<V> map(C);

  float mu[V], is[V];
  load_coef<V>(mu, mean + map.c0);
  load_coef<V>(is, invstd + map.c0);

  float a0[V], a1[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a1[i] = 0.f; }

  const long row_stride = (long)gridDim.x * map.rpb;
  for (long r = (long)blockIdx.x * map.rpb + map.row_in_block; r < R;
       r += row_stride) {
    T dv[V], xv[V];
    load_vec<T, V>(dv, dy + r * C + map.c0);
    load_vec<T, V>(xv, x + r * C + map.c0);
    unsigned int m = 0xffu;
    if constexpr (RELU) m = mask[(r * C + map.c0) / V];
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
  float* row = partial + (long)blockIdx.x * C + map.c0;
  bn_block_fold<V>(lds, a0, row, map);
  bn_block_fold<V>(lds, a1, row + nbC, map);
}

// --------------------------------------------------------------------
// backward stage 2: fold partials -> dgamma/dbeta and the three
// per-channel dx coefficients, coef = [3, C] (P, Q, S):
//   dx = P*dy_eff + Q*x + S
//   P = gamma*invstd
//   Q = -P * invstd * (dxhat_sum/R)
//   S = -P * (dsum/R) - Q * mean
// --------------------------------------------------------------------
__device__ __forceinline__ void bn_bwd_pqs(
    float* __restrict__ coef, int C, int c, float dsum, float dxhat,
    float invR, float gamma, float mean, float invstd) {
  const float P = gamma * invstd;
  const float Q = -P * invstd * dxhat * invR;
  coef[c] = P;
  coef[C + c] = Q;
  // S = -P*dsum*invR - Q*mean with Q*mean the fused product: spelled
  // out, because left to contraction the compiler may fuse the other
  // product instead, and dx would differ in its last bit
  coef[2 * C + c] = fmaf(-mean, Q, -P * dsum * invR);
}

__global__ void bn_bwd_coef_kernel(
    const float* __restrict__ partial2,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ coef, long R, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float dsum, dxhat;
  bn_fold_b2(partial2, C, c, dsum, dxhat);
  dbeta[c] = dsum;
  dgamma[c] = dxhat;
  bn_bwd_pqs(coef, C, c, dsum, dxhat, 1.f / (float)R, gamma[c], mean[c],
             invstd[c]);
}

// bn_bwd_coef_kernel on reduced sums and the global row count;
// dgamma/dbeta stay the caller's local sums
__global__ void bn_sync_bwd_coef_kernel(
    const float* __restrict__ bsums, const float* __restrict__ count,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ coef, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_bwd_pqs(coef, C, c, bsums[c], bsums[C + c], 1.f / count[0],
             gamma[c], mean[c], invstd[c]);
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
  const BnRowMap<V> map(C);

  float mu[V], is[V];
  load_coef<V>(mu, mean + map.c0);
  load_coef<V>(is, invstd + map.c0);
  float a0[V], a1[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a1[i] = 0.f; }

  const long row_stride = (long)gridDim.x * map.rpb;
  long r = (long)blockIdx.x * map.rpb + map.row_in_block;
  int w = (int)(r % W);
  int h = (int)((r / W) % H);
  long n = r / W / H;
  const int dw = (int)(row_stride % W);
  const int dh = (int)((row_stride / W) % H);
  const long dn = row_stride / W / H;
  for (; r < R; r += row_stride) {
    T xv[V];
    load_vec<T, V>(xv, x + r * C + map.c0);
    float d[V];
    bn_pool_gather_dy<T>(d, dpool, code, n * OH * OW, h, w, OH, OW, C,
                         map.tpr, map.slot);
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
  float* row = partial + (long)blockIdx.x * C + map.c0;
  bn_block_fold<V>(lds, a0, row, map);
  bn_block_fold<V>(lds, a1, row + nbC, map);
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
  const BnRowMap<V> map(C);  // rows of a block: pixels of one line
  float P[V], Q[V], S[V];
  load_coef<V>(P, coefP + map.c0);
  load_coef<V>(Q, coefQ + map.c0);
  load_coef<V>(S, coefS + map.c0);
  for (int line = blockIdx.x; line < lines; line += gridDim.x) {
    const int n = line / H;
    const int h = line - n * H;
    const long obase = (long)n * OH * OW;
    for (int w = map.row_in_block; w < W; w += map.rpb) {
      const long idx = ((long)line * W + w) * C + map.c0;
      T xv[V];
      load_vec<T, V>(xv, x + idx);
      float d[V];
      bn_pool_gather_dy<T>(d, dpool, code, obase, h, w, OH, OW, C,
                           map.tpr, map.slot);
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
  const BnRowMap<V> map(C);

  float mu3[V], is3[V], mud[V], isd[V];
  load_coef<V>(mu3, mean3 + map.c0);
  load_coef<V>(is3, invstd3 + map.c0);
  load_coef<V>(mud, meand + map.c0);
  load_coef<V>(isd, invstdd + map.c0);
  float a0[V], a3[V], ad[V];
  #pragma unroll
  for (int i = 0; i < V; ++i) { a0[i] = 0.f; a3[i] = 0.f; ad[i] = 0.f; }

  const long row_stride = (long)gridDim.x * map.rpb;
  for (long r = (long)blockIdx.x * map.rpb + map.row_in_block; r < R;
       r += row_stride) {
    T dv[V], av[V], bv[V];
    load_vec<T, V>(dv, dy + r * C + map.c0);
    load_vec<T, V>(av, x3 + r * C + map.c0);
    load_vec<T, V>(bv, xd + r * C + map.c0);
    const unsigned int m = mask[(r * C + map.c0) / V];
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
  float* row = partial + (long)blockIdx.x * C + map.c0;
  bn_block_fold<V>(lds, a0, row, map);
  bn_block_fold<V>(lds, a3, row + nbC, map);
  bn_block_fold<V>(lds, a0, row + 2 * nbC, map);
  bn_block_fold<V>(lds, ad, row + 3 * nbC, map);
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

// ====================================================================
// host side. Every exported function validates all of its operands
// (bn_check_* below) before it allocates, copies or launches; what
// follows a check may reinterpret_cast and data_ptr<float>() freely.
// ====================================================================
int bn_vec_width(const torch::Tensor& x) {
  return x.scalar_type() == at::kBFloat16 ? 8 : 4;
}

// runs the statement once, with T bound to x's element type
#define BN_DISPATCH(x, ...)                                              \
  do {                                                                   \
    if ((x).scalar_type() == at::kBFloat16) {                            \
      using T = __hip_bfloat16;                                          \
      __VA_ARGS__;                                                       \
    } else {                                                             \
      using T = float;                                                   \
      __VA_ARGS__;                                                       \
    }                                                                    \
  } while (0)

template <typename T>
T* bn_ptr(const torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

float* fptr(const torch::Tensor& t) { return t.data_ptr<float>(); }

// "no running stats" reaches us as an undefined or an empty tensor
bool bn_absent(const torch::Tensor& t) {
  return !t.defined() || t.numel() == 0;
}
float* bn_running_ptr(const torch::Tensor& t) {
  return bn_absent(t) ? nullptr : fptr(t);
}

struct BnDims { int C, V; long R; };

// the activation: 4-D channels_last bf16/fp32 on the GPU, non-empty,
// C/V a power of two <= kT (see BnRowMap)
BnDims bn_check_input(const torch::Tensor& x, const char* what) {
  TORCH_CHECK(x.defined() && x.is_cuda() && x.dim() == 4, what,
              ": 4-D GPU input expected");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
              x.scalar_type() == at::kFloat, what,
              ": dtype must be bf16 or f32");
  TORCH_CHECK(x.numel() > 0, what, ": empty input");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), what,
              ": channels_last input required");
  const int C = (int)x.size(1);
  const int V = bn_vec_width(x);
  TORCH_CHECK(C % V == 0 && C / V <= kT, what, ": C=", C,
              " unsupported for vec", V);
  const int tpr = C / V;
  TORCH_CHECK((tpr & (tpr - 1)) == 0, what, ": C/", V,
              " must be a power of two");
  return {C, V, x.numel() / C};
}

// an fp32 vector of n elements on x's device
void bn_check_vec(const torch::Tensor& t, const torch::Tensor& x, long n,
                  const char* what, const char* name) {
  TORCH_CHECK(t.defined() && t.scalar_type() == at::kFloat &&
              t.device() == x.device() && t.is_contiguous() &&
              t.numel() == n, what, ": ", name, " must be fp32 [", n,
              "] on the input's device");
}

struct BnNamed { const char* name; const torch::Tensor& t; };

// per-channel operands: fp32 [C] on x's device
void bn_check_channel_vecs(const torch::Tensor& x, const char* what,
                           std::initializer_list<BnNamed> vecs) {
  for (const BnNamed& v : vecs) bn_check_vec(v.t, x, x.size(1), what, v.name);
}

// running stats: both or neither; `required` in eval mode
void bn_check_running(const torch::Tensor& running_mean,
                      const torch::Tensor& running_var,
                      const torch::Tensor& x, bool required,
                      const char* what) {
  TORCH_CHECK(bn_absent(running_mean) == bn_absent(running_var), what,
              ": running_mean and running_var go together");
  if (bn_absent(running_mean)) {
    TORCH_CHECK(!required, what, ": eval mode needs the running stats");
    return;
  }
  bn_check_channel_vecs(x, what, {{"running_mean", running_mean},
                                  {"running_var", running_var}});
}

// a second activation (residual, other input, gradient): x's sizes,
// dtype and device; channels_last too unless the caller converts it
void bn_check_like(const torch::Tensor& t, const torch::Tensor& x,
                   bool nhwc, const char* what, const char* msg) {
  TORCH_CHECK(t.defined() && t.sizes() == x.sizes() &&
              t.scalar_type() == x.scalar_type() &&
              t.device() == x.device() &&
              (!nhwc || t.is_contiguous(at::MemoryFormat::ChannelsLast)),
              what, ": ", msg);
}

// the forward's ReLU bitmask: one byte per V elements
void bn_check_mask(const torch::Tensor& mask, const torch::Tensor& x,
                   const char* what) {
  TORCH_CHECK(mask.defined() && mask.scalar_type() == at::kByte &&
              mask.device() == x.device() && mask.is_contiguous() &&
              mask.numel() == x.numel() / bn_vec_width(x),
              what, ": relu path needs the fwd mask");
}

// what every backward shares: x, the gradient, the saved statistics
// and, with ReLU, the mask
BnDims bn_check_bwd_args(const torch::Tensor& dy, const torch::Tensor& mask,
                         const torch::Tensor& x, const torch::Tensor& mean,
                         const torch::Tensor& invstd, bool relu,
                         const char* what) {
  const BnDims d = bn_check_input(x, what);
  bn_check_like(dy, x, false, what, "bad gradient");
  bn_check_channel_vecs(x, what, {{"mean", mean}, {"invstd", invstd}});
  if (relu) bn_check_mask(mask, x, what);
  return d;
}

struct PoolGeom { int N, H, W, OH, OW; };

PoolGeom pool_geom(const torch::Tensor& x) {
  PoolGeom g;
  g.N = (int)x.size(0); g.H = (int)x.size(2); g.W = (int)x.size(3);
  g.OH = (g.H - 1) / 2 + 1;   // kernel 3, stride 2, pad 1, floor mode
  g.OW = (g.W - 1) / 2 + 1;
  return g;
}

// the stem input: the pool kernels index pixels and code words in 32 bits
BnDims bn_check_pool_input(const torch::Tensor& x, const char* what) {
  const BnDims d = bn_check_input(x, what);
  TORCH_CHECK(x.numel() < (1L << 31), what, ": input too large");
  return d;
}

// ---- launches ------------------------------------------------------
int bn_stage1_blocks(const BnDims& d) {
  const int rpb = kT / (d.C / d.V);
  const long blocks = (d.R + rpb - 1) / rpb;
  return (int)std::min<long>(std::max<long>(blocks, 1), kMaxStage1);
}

long bn_grid_elems(long nvec) {
  long blocks = (nvec + kT - 1) / kT;
  return std::min<long>(std::max<long>(blocks, 1), 16384);
}

dim3 bn_grid_channels(int C) { return dim3((C + 255) / 256); }

at::TensorOptions bn_fopts(const torch::Tensor& x) {
  return x.options().dtype(at::kFloat);
}

// stage 2a: one [2, nb, C] stage-1 partial -> [2, kB2, C]
torch::Tensor bn_fold2(const float* partial, int nb, const torch::Tensor& x,
                       hipStream_t stream) {
  const int C = (int)x.size(1);
  auto partial2 = torch::empty({2, kB2, C}, bn_fopts(x));
  hipLaunchKernelGGL(bn_fold2_kernel,
                     dim3((C + kFoldC - 1) / kFoldC, kB2), dim3(kT), 0,
                     stream, partial, nb, fptr(partial2), C);
  CHECK_HIP_BN(hipGetLastError());
  return partial2;
}

// stats -> fold: the [2, kB2, C] second-level partials of sum / sumsq
torch::Tensor bn_stats_partial2(const torch::Tensor& x, const BnDims& d,
                                hipStream_t stream) {
  const int nb = bn_stage1_blocks(d);
  auto partial = torch::empty({2, nb, d.C}, bn_fopts(x));
  BN_DISPATCH(x, hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(nb),
                                    dim3(kT), 0, stream, bn_ptr<const T>(x),
                                    fptr(partial), d.R, d.C));
  CHECK_HIP_BN(hipGetLastError());
  return bn_fold2(fptr(partial), nb, x, stream);
}

// the per-channel results every forward returns or hands to its
// elementwise pass
struct BnFwdOut {
  torch::Tensor mean, invstd, scale, bias;
  explicit BnFwdOut(const torch::Tensor& x) {
    for (torch::Tensor* t : {&mean, &invstd, &scale, &bias})
      *t = torch::empty({x.size(1)}, bn_fopts(x));
  }
  BnFwdCoef args(const torch::Tensor& gamma, const torch::Tensor& beta,
                 const torch::Tensor& running_mean,
                 const torch::Tensor& running_var, double momentum,
                 double eps) const {
    return {fptr(gamma), fptr(beta), bn_running_ptr(running_mean),
            bn_running_ptr(running_var), fptr(mean), fptr(invstd),
            fptr(scale), fptr(bias), (float)momentum, (float)eps};
  }
};

// training-mode stats -> fold -> coef: batch mean/invstd, the apply
// pass's scale/bias, and the running-stat update
BnFwdOut bn_train_coefs(const torch::Tensor& x, const torch::Tensor& gamma,
                        const torch::Tensor& beta,
                        const torch::Tensor& running_mean,
                        const torch::Tensor& running_var, double momentum,
                        double eps, const BnDims& d, hipStream_t stream) {
  BnFwdOut o(x);
  torch::Tensor partial2 = bn_stats_partial2(x, d, stream);
  hipLaunchKernelGGL(bn_stats_coef_kernel, bn_grid_channels(d.C),
                     dim3(256), 0, stream, fptr(partial2),
                     o.args(gamma, beta, running_mean, running_var,
                            momentum, eps), d.R, d.C);
  CHECK_HIP_BN(hipGetLastError());
  return o;
}

// eval mode: scale/bias straight from the running stats; mean and
// invstd are returned unset
BnFwdOut bn_eval_coefs(const torch::Tensor& x, const torch::Tensor& gamma,
                       const torch::Tensor& beta,
                       const torch::Tensor& running_mean,
                       const torch::Tensor& running_var, double eps,
                       const BnDims& d, hipStream_t stream) {
  BnFwdOut o(x);
  hipLaunchKernelGGL(bn_eval_coef_kernel, bn_grid_channels(d.C), dim3(256),
                     0, stream, fptr(running_mean), fptr(running_var),
                     fptr(gamma), fptr(beta), fptr(o.scale), fptr(o.bias),
                     d.C, (float)eps);
  CHECK_HIP_BN(hipGetLastError());
  return o;
}

// the elementwise forward pass: y = [relu](scale*x + bias [+ res]);
// the mask is written when one is given
void bn_launch_apply(const torch::Tensor& x, torch::Tensor& y,
                     const BnFwdOut& o,
                     const c10::optional<torch::Tensor>& res,
                     const torch::Tensor& mask, bool relu, const BnDims& d,
                     hipStream_t stream) {
  const long total = d.R * (long)d.C;
  const long grid = bn_grid_elems(total / d.V);
  unsigned char* mp = mask.defined()
      ? mask.data_ptr<unsigned char>() : nullptr;
  const bool wm = relu && mp != nullptr;
  #define APPLY(RELU_, RES_, WM_)                                       \
    hipLaunchKernelGGL((bn_apply_kernel<T, RELU_, RES_, WM_>),          \
                       dim3(grid), dim3(kT), 0, stream,                 \
                       bn_ptr<const T>(x), bn_ptr<T>(y), fptr(o.scale), \
                       fptr(o.bias), resp, mp, total, d.C)
  BN_DISPATCH(x, {
    const T* resp = res.has_value() ? bn_ptr<const T>(*res) : nullptr;
    if (relu && resp) { if (wm) APPLY(true, true, true);
                        else APPLY(true, true, false); }
    else if (relu) { if (wm) APPLY(true, false, true);
                     else APPLY(true, false, false); }
    else if (resp) APPLY(false, true, false);
    else APPLY(false, false, false);
  });
  #undef APPLY
  CHECK_HIP_BN(hipGetLastError());
}

// backward reduce -> fold: the [2, kB2, C] second-level partials of
// sum(dy_eff) / sum(dy_eff * xhat)
torch::Tensor bn_bwd_partial(const torch::Tensor& dy,
                             const torch::Tensor& mask,
                             const torch::Tensor& x,
                             const torch::Tensor& mean,
                             const torch::Tensor& invstd, bool relu,
                             const BnDims& d, hipStream_t stream) {
  const int nb = bn_stage1_blocks(d);
  auto partial = torch::empty({2, nb, d.C}, bn_fopts(x));
  const unsigned char* mp = relu ? mask.data_ptr<unsigned char>() : nullptr;
  #define RED(RELU_)                                                     \
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, RELU_>), dim3(nb),       \
                       dim3(kT), 0, stream, bn_ptr<const T>(dy), mp,     \
                       bn_ptr<const T>(x), fptr(mean), fptr(invstd),     \
                       fptr(partial), d.R, d.C)
  BN_DISPATCH(x, { if (relu) RED(true); else RED(false); });
  #undef RED
  CHECK_HIP_BN(hipGetLastError());
  return partial;
}

// backward fold -> coef for one BN from its [2, nb, C] stage-1 partial:
// dgamma, dbeta and coef = [3, C] (P, Q, S)
struct BnBwdOut { torch::Tensor dgamma, dbeta, coef; };

BnBwdOut bn_bwd_fold_coefs(const float* partial, int nb,
                           const torch::Tensor& x,
                           const torch::Tensor& gamma,
                           const torch::Tensor& mean,
                           const torch::Tensor& invstd, const BnDims& d,
                           hipStream_t stream) {
  BnBwdOut o = {torch::empty({d.C}, bn_fopts(x)),
                torch::empty({d.C}, bn_fopts(x)),
                torch::empty({3, d.C}, bn_fopts(x))};
  torch::Tensor partial2 = bn_fold2(partial, nb, x, stream);
  hipLaunchKernelGGL(bn_bwd_coef_kernel, bn_grid_channels(d.C), dim3(256),
                     0, stream, fptr(partial2), fptr(gamma), fptr(mean),
                     fptr(invstd), fptr(o.dgamma), fptr(o.dbeta),
                     fptr(o.coef), d.R, d.C);
  CHECK_HIP_BN(hipGetLastError());
  return o;
}

// the elementwise backward pass: dx = P*dy_eff + Q*x + S [, dres];
// coef = [3, C]
void bn_launch_bwd_dx(const torch::Tensor& dy, const torch::Tensor& mask,
                      const torch::Tensor& x, const torch::Tensor& coef,
                      torch::Tensor& dx,
                      const c10::optional<torch::Tensor>& dres, bool relu,
                      const BnDims& d, hipStream_t stream) {
  const unsigned char* mp = relu ? mask.data_ptr<unsigned char>() : nullptr;
  const long total = d.R * (long)d.C;
  const long grid = bn_grid_elems(total / d.V);
  const float* cf = fptr(coef);
  #define DX(RELU_, RES_)                                                \
    hipLaunchKernelGGL((bn_bwd_dx_kernel<T, RELU_, RES_>), dim3(grid),   \
                       dim3(kT), 0, stream, bn_ptr<const T>(dy), mp,     \
                       bn_ptr<const T>(x), cf, cf + d.C, cf + 2 * d.C,   \
                       bn_ptr<T>(dx), dresp, total, d.C)
  BN_DISPATCH(x, {
    T* dresp = dres.has_value() ? bn_ptr<T>(*dres) : nullptr;
    if (relu && dresp) DX(true, true);
    else if (relu) DX(true, false);
    else if (dresp) DX(false, true);
    else DX(false, false);
  });
  #undef DX
  CHECK_HIP_BN(hipGetLastError());
}

}  // namespace

// x: [N, C, H, W] channels_last (viewed as [R, C]); gamma/beta fp32;
// the running stats may be absent in training mode.
// Returns (y, save_mean, save_invstd, mask).
std::vector<torch::Tensor> fused_bn_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor running_mean, torch::Tensor running_var,
    c10::optional<torch::Tensor> res, bool relu, bool training,
    double momentum, double eps) {
  const char* what = "fused_bn_fwd";
  const BnDims d = bn_check_input(x, what);
  bn_check_channel_vecs(x, what, {{"gamma", gamma}, {"beta", beta}});
  bn_check_running(running_mean, running_var, x, !training, what);
  if (res.has_value()) bn_check_like(*res, x, true, what, "bad residual");
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x);  // keeps channels_last layout
  // ReLU bitmask (1 byte per V elems) replaces re-reading y in
  // backward: ~25% less bwd traffic
  torch::Tensor mask;
  if (relu && training)
    mask = torch::empty({x.numel() / d.V}, x.options().dtype(at::kByte));
  const BnFwdOut o = training
      ? bn_train_coefs(x, gamma, beta, running_mean, running_var, momentum,
                       eps, d, stream)
      : bn_eval_coefs(x, gamma, beta, running_mean, running_var, eps, d,
                      stream);
  bn_launch_apply(x, y, o, res, mask, relu, d, stream);
  if (!mask.defined())
    mask = torch::empty({0}, x.options().dtype(at::kByte));
  return {y, o.mean, o.invstd, mask};
}

// Returns (dx, dgamma, dbeta[, dres]). mask: ReLU bitmask from fwd
// (empty tensor when relu=false).
std::vector<torch::Tensor> fused_bn_bwd(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, torch::Tensor gamma,
    bool relu, bool has_res) {
  const char* what = "fused_bn_bwd";
  const BnDims d = bn_check_bwd_args(dy, mask, x, mean, invstd, relu, what);
  bn_check_channel_vecs(x, what, {{"gamma", gamma}});
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  c10::optional<torch::Tensor> dres;
  if (has_res) dres = torch::empty_like(x);
  torch::Tensor partial =
      bn_bwd_partial(dy, mask, x, mean, invstd, relu, d, stream);
  BnBwdOut o = bn_bwd_fold_coefs(fptr(partial), (int)partial.size(1), x,
                                 gamma, mean, invstd, d, stream);
  bn_launch_bwd_dx(dy, mask, x, o.coef, dx, dres, relu, d, stream);
  std::vector<torch::Tensor> out = {dx, o.dgamma, o.dbeta};
  if (has_res) out.push_back(*dres);
  return out;
}

// ---- synchronized BN: forward and backward cut where the sums exist.
// No call below waits for the device or reads a value back.

// Returns sums = fp32 [2C+1]: sum(x), sum(x^2) per channel, then the
// row count N*H*W.
torch::Tensor fused_bn_sync_stats(torch::Tensor x) {
  const BnDims d = bn_check_input(x, "fused_bn_sync_stats");
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto sums = torch::empty({2 * (long)d.C + 1}, bn_fopts(x));
  torch::Tensor partial2 = bn_stats_partial2(x, d, stream);
  hipLaunchKernelGGL(bn_sync_fold_kernel, bn_grid_channels(d.C),
                     dim3(256), 0, stream, fptr(partial2), fptr(sums),
                     d.C, (float)d.R, true);
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
  const BnDims d = bn_check_input(x, what);
  bn_check_vec(sums, x, 2 * (long)d.C + 1, what, "sums");
  bn_check_channel_vecs(x, what, {{"gamma", gamma}, {"beta", beta}});
  bn_check_running(running_mean, running_var, x, false, what);
  if (res.has_value()) bn_check_like(*res, x, true, what, "bad residual");
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x);
  torch::Tensor mask = torch::empty({relu ? x.numel() / d.V : 0},
                                    x.options().dtype(at::kByte));
  BnFwdOut o(x);
  hipLaunchKernelGGL(bn_sync_stats_coef_kernel, bn_grid_channels(d.C),
                     dim3(256), 0, stream, fptr(sums),
                     o.args(gamma, beta, running_mean, running_var,
                            momentum, eps), d.C);
  CHECK_HIP_BN(hipGetLastError());
  bn_launch_apply(x, y, o, res, mask, relu, d, stream);
  return {y, o.mean, o.invstd, mask};
}

// Returns bsums = fp32 [2C]: sum(dy_eff) (this rank's dbeta), then
// sum(dy_eff * xhat) (its dgamma).
torch::Tensor fused_bn_sync_bwd_reduce(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, bool relu) {
  const BnDims d = bn_check_bwd_args(dy, mask, x, mean, invstd, relu,
                                     "fused_bn_sync_bwd_reduce");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto bsums = torch::empty({2 * (long)d.C}, bn_fopts(x));
  torch::Tensor partial =
      bn_bwd_partial(dy, mask, x, mean, invstd, relu, d, stream);
  torch::Tensor partial2 =
      bn_fold2(fptr(partial), (int)partial.size(1), x, stream);
  hipLaunchKernelGGL(bn_sync_fold_kernel, bn_grid_channels(d.C),
                     dim3(256), 0, stream, fptr(partial2), fptr(bsums),
                     d.C, 0.f, false);
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
  const BnDims d = bn_check_bwd_args(dy, mask, x, mean, invstd, relu, what);
  bn_check_channel_vecs(x, what, {{"gamma", gamma}});
  bn_check_vec(bsums, x, 2 * (long)d.C, what, "bsums");
  bn_check_vec(count, x, 1, what, "count");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  auto coef = torch::empty({3, d.C}, bn_fopts(x));
  c10::optional<torch::Tensor> dres;
  if (has_res) dres = torch::empty_like(x);
  hipLaunchKernelGGL(bn_sync_bwd_coef_kernel, bn_grid_channels(d.C),
                     dim3(256), 0, stream, fptr(bsums), fptr(count),
                     fptr(gamma), fptr(mean), fptr(invstd), fptr(coef),
                     d.C);
  CHECK_HIP_BN(hipGetLastError());
  bn_launch_bwd_dx(dy, mask, x, coef, dx, dres, relu, d, stream);
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
  const char* what = "fused_bn_relu_pool_fwd";
  const BnDims d = bn_check_pool_input(x, what);
  bn_check_channel_vecs(x, what, {{"gamma", gamma}, {"beta", beta}});
  bn_check_running(running_mean, running_var, x, false, what);
  const PoolGeom g = pool_geom(x);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto pooled = torch::empty({g.N, d.C, g.OH, g.OW}, x.options(),
                             at::MemoryFormat::ChannelsLast);
  const long nvec = (long)g.N * g.OH * g.OW * (d.C / d.V);
  auto code = torch::empty({nvec}, x.options().dtype(at::kInt));
  BnFwdOut o = bn_train_coefs(x, gamma, beta, running_mean, running_var,
                              momentum, eps, d, stream);
  BN_DISPATCH(x, hipLaunchKernelGGL(
      (bn_relu_pool_apply_kernel<T>), dim3(bn_grid_elems(nvec)), dim3(kT),
      0, stream, bn_ptr<const T>(x), bn_ptr<T>(pooled),
      bn_ptr<unsigned int>(code), fptr(o.scale), fptr(o.bias),
      (unsigned int)nvec, g.H, g.W, g.OH, g.OW, d.C));
  CHECK_HIP_BN(hipGetLastError());
  return {pooled, o.mean, o.invstd, code};
}

// Returns (dx, dgamma, dbeta).
std::vector<torch::Tensor> fused_bn_relu_pool_bwd(
    torch::Tensor dpool, torch::Tensor code, torch::Tensor x,
    torch::Tensor mean, torch::Tensor invstd, torch::Tensor gamma) {
  const char* what = "fused_bn_relu_pool_bwd";
  const BnDims d = bn_check_pool_input(x, what);
  const PoolGeom g = pool_geom(x);
  TORCH_CHECK(dpool.defined() && dpool.dim() == 4 &&
              dpool.size(0) == g.N && dpool.size(1) == d.C &&
              dpool.size(2) == g.OH && dpool.size(3) == g.OW &&
              dpool.scalar_type() == x.scalar_type() &&
              dpool.device() == x.device(),
              what, ": bad pooled gradient");
  TORCH_CHECK(code.defined() && code.scalar_type() == at::kInt &&
              code.device() == x.device() && code.is_contiguous() &&
              code.numel() == (long)g.N * g.OH * g.OW * (d.C / d.V),
              what, ": bad code tensor");
  bn_check_channel_vecs(x, what, {{"mean", mean}, {"invstd", invstd},
                                  {"gamma", gamma}});
  dpool = dpool.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx = torch::empty_like(x);
  const int lines = g.N * g.H;
  const int nb = bn_stage1_blocks(d);
  auto partial = torch::empty({2, nb, d.C}, bn_fopts(x));
  BN_DISPATCH(x, hipLaunchKernelGGL(
      (bn_pool_bwd_reduce_kernel<T>), dim3(nb), dim3(kT), 0, stream,
      bn_ptr<const T>(dpool), bn_ptr<const unsigned int>(code),
      bn_ptr<const T>(x), fptr(mean), fptr(invstd), fptr(partial), d.R,
      g.H, g.W, g.OH, g.OW, d.C));
  CHECK_HIP_BN(hipGetLastError());
  BnBwdOut o = bn_bwd_fold_coefs(fptr(partial), nb, x, gamma, mean, invstd,
                                 d, stream);
  const float* cf = fptr(o.coef);
  BN_DISPATCH(x, hipLaunchKernelGGL(
      (bn_pool_bwd_dx_kernel<T>), dim3(std::min(lines, 16384)), dim3(kT),
      0, stream, bn_ptr<const T>(dpool), bn_ptr<const unsigned int>(code),
      bn_ptr<const T>(x), cf, cf + d.C, cf + 2 * d.C, bn_ptr<T>(dx),
      lines, g.H, g.W, g.OH, g.OW, d.C));
  CHECK_HIP_BN(hipGetLastError());
  return {dx, o.dgamma, o.dbeta};
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
  const char* what = "fused_bn_dual_fwd";
  const BnDims d = bn_check_input(x3, what);
  bn_check_like(xd, x3, true, what, "the two inputs must match");
  bn_check_channel_vecs(x3, what, {{"gamma3", gamma3}, {"beta3", beta3},
                                   {"gammad", gammad}, {"betad", betad}});
  bn_check_running(running_mean3, running_var3, x3, false, what);
  bn_check_running(running_meand, running_vard, x3, false, what);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto y = torch::empty_like(x3);
  auto mask = torch::empty({x3.numel() / d.V},
                           x3.options().dtype(at::kByte));
  BnFwdOut od = bn_train_coefs(xd, gammad, betad, running_meand,
                               running_vard, momentumd, epsd, d, stream);
  BnFwdOut o3 = bn_train_coefs(x3, gamma3, beta3, running_mean3,
                               running_var3, momentum3, eps3, d, stream);
  const long total = d.R * (long)d.C;
  BN_DISPATCH(x3, hipLaunchKernelGGL(
      (bn_dual_apply_kernel<T>), dim3(bn_grid_elems(total / d.V)),
      dim3(kT), 0, stream, bn_ptr<const T>(x3), bn_ptr<const T>(xd),
      bn_ptr<T>(y), fptr(o3.scale), fptr(o3.bias), fptr(od.scale),
      fptr(od.bias), mask.data_ptr<unsigned char>(), total, d.C));
  CHECK_HIP_BN(hipGetLastError());
  return {y, o3.mean, o3.invstd, od.mean, od.invstd, mask};
}

// Returns (dx3, dxd, dgamma3, dbeta3, dgammad, dbetad).
std::vector<torch::Tensor> fused_bn_dual_bwd(
    torch::Tensor dy, torch::Tensor mask, torch::Tensor x3,
    torch::Tensor xd, torch::Tensor mean3, torch::Tensor invstd3,
    torch::Tensor gamma3, torch::Tensor meand, torch::Tensor invstdd,
    torch::Tensor gammad) {
  const char* what = "fused_bn_dual_bwd";
  const BnDims d =
      bn_check_bwd_args(dy, mask, x3, mean3, invstd3, true, what);
  bn_check_like(xd, x3, true, what, "the two inputs must match");
  bn_check_channel_vecs(x3, what, {{"gamma3", gamma3}, {"meand", meand},
                                   {"invstdd", invstdd},
                                   {"gammad", gammad}});
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto dx3 = torch::empty_like(x3);
  auto dxd = torch::empty_like(xd);
  const int nb = bn_stage1_blocks(d);
  auto partial = torch::empty({4, nb, d.C}, bn_fopts(x3));
  const unsigned char* mp = mask.data_ptr<unsigned char>();
  BN_DISPATCH(x3, hipLaunchKernelGGL(
      (bn_dual_bwd_reduce_kernel<T>), dim3(nb), dim3(kT), 0, stream,
      bn_ptr<const T>(dy), mp, bn_ptr<const T>(x3), bn_ptr<const T>(xd),
      fptr(mean3), fptr(invstd3), fptr(meand), fptr(invstdd),
      fptr(partial), d.R, d.C));
  CHECK_HIP_BN(hipGetLastError());
  const float* pp = fptr(partial);
  BnBwdOut o3 = bn_bwd_fold_coefs(pp, nb, x3, gamma3, mean3, invstd3, d,
                                  stream);
  BnBwdOut od = bn_bwd_fold_coefs(pp + 2 * (long)nb * d.C, nb, x3, gammad,
                                  meand, invstdd, d, stream);
  const long total = d.R * (long)d.C;
  BN_DISPATCH(x3, hipLaunchKernelGGL(
      (bn_dual_bwd_dx_kernel<T>), dim3(bn_grid_elems(total / d.V)),
      dim3(kT), 0, stream, bn_ptr<const T>(dy), mp, bn_ptr<const T>(x3),
      bn_ptr<const T>(xd), fptr(o3.coef), fptr(od.coef), bn_ptr<T>(dx3),
      bn_ptr<T>(dxd), total, d.C));
  CHECK_HIP_BN(hipGetLastError());
  return {dx3, dxd, o3.dgamma, o3.dbeta, od.dgamma, od.dbeta};
}
