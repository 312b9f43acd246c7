// Fused softmax cross-entropy over [R, V] logits rows on CDNA4, with
// ignore_index, label smoothing and z-loss. For a row z[0..V) with
// target t, smoothing e and z-loss weight l:
//
//   lse  = logsumexp(z)
//   loss = lse - (1-e) z_t - (e/V) sum_j z_j + l lse^2
//   dz_j = g ((1 + 2 l lse) exp(z_j - lse) - (1-e) [j==t] - e/V)
//
// and loss = 0, dz = 0 for a row whose target is ignore_index.
//
//   forward:  one pass over the row. Each thread keeps a running
//             (max, sum-exp, sum-z); the block combines them with
//             wave-64 shuffles and then through LDS across its four
//             waves, in a fixed order — no atomics, so the result is
//             bitwise reproducible.
//   backward: one pass, every value rounded once from fp32. May write
//             over the logits it reads (each lane stores exactly the
//             elements it loaded), so that pointer pair carries no
//             __restrict__.
//
// Rows are V contiguous elements of bf16/f32 and V is arbitrary (GPT-2:
// 50257, odd), so a row start is only element-aligned: each row is a
// scalar head up to the first 16-byte boundary, a body of 16-byte
// per-lane vectors, and a scalar tail. Row offsets are 64-bit.
//
// lse is kept as an unevaluated fp32 pair (lse, lse_lo) with
// lse + lse_lo = max + log(sum) to about twice fp32 precision: a single
// float at |lse| ~ 300 is only good to 1.5e-5, which exp(z - lse) would
// turn into a relative error of the same size in every probability.
//
// A target is only ever used as an index after it is checked against
// [0, V): an out-of-range target that is not ignore_index gives a NaN
// row loss and a zero gradient row.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <cstdint>
#include <limits>

namespace {

constexpr int kT = 256;          // 4 wave64
constexpr int kWaves = kT / 64;
constexpr long kMaxGrid = 8192;  // rows beyond this are grid-strided

template <typename T> struct CeVec;
template <> struct CeVec<float> { static constexpr int V = 4; };
template <> struct CeVec<__hip_bfloat16> { static constexpr int V = 8; };

template <typename T>
__device__ __forceinline__ float ce_tof(T v);
template <>
__device__ __forceinline__ float ce_tof<float>(float v) { return v; }
template <>
__device__ __forceinline__ float ce_tof<__hip_bfloat16>(
    __hip_bfloat16 v) { return __bfloat162float(v); }

template <typename T>
__device__ __forceinline__ T ce_fromf(float v);
template <>
__device__ __forceinline__ float ce_fromf<float>(float v) { return v; }
template <>
__device__ __forceinline__ __hip_bfloat16 ce_fromf<__hip_bfloat16>(
    float v) { return __float2bfloat16(v); }

// where a row's head / vector body / tail start and end
struct RowSplit {
  int head;   // scalar elements before the first 16-byte boundary
  int nvec;   // 16-byte vectors in the body
  int tail0;  // first element of the scalar tail
};

template <typename T>
__device__ __forceinline__ RowSplit split_row(const T* row, int V) {
  constexpr int VEC = CeVec<T>::V;
  const uintptr_t a = reinterpret_cast<uintptr_t>(row);
  int head = (int)(((16u - (unsigned)(a & 15u)) & 15u) / sizeof(T));
  if (head > V) head = V;
  RowSplit s;
  s.head = head;
  s.nvec = (V - head) / VEC;
  s.tail0 = head + s.nvec * VEC;
  return s;
}

// running softmax statistics: sum_j exp(z_j - m) with m the max so far
struct Stat {
  float m, s, sz;
};

// exp(a - b) that is 0, not NaN, when a is the empty state's -inf
__device__ __forceinline__ float exp_diff(float a, float b) {
  return a == -INFINITY ? 0.f : expf(a - b);
}

__device__ __forceinline__ void stat_add(Stat& st, float z) {
  if (z > st.m) {
    st.s *= exp_diff(st.m, z);
    st.m = z;
  }
  st.s += exp_diff(z, st.m);
  st.sz += z;
}

__device__ __forceinline__ Stat stat_merge(const Stat& a, const Stat& b) {
  Stat o;
  o.m = fmaxf(a.m, b.m);
  o.s = a.s * exp_diff(a.m, o.m) + b.s * exp_diff(b.m, o.m);
  o.sz = a.sz + b.sz;
  return o;
}

// --------------------------------------------------------------------
// forward: one block per row
// --------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void ce_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ targets,
    float* __restrict__ loss_rows, float* __restrict__ lse_out,
    float* __restrict__ lse_lo_out, long R, int V, int64_t ignore_index, float smoothing, float z_loss) {
  constexpr int VEC = CeVec<T>::V;
  __shared__ float lds[kWaves * 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const T* row = logits + r * (long)V;
    const RowSplit sp = split_row(row, V);
    Stat st{-INFINITY, 0.f, 0.f};

    for (int j = threadIdx.x; j < sp.head; j += kT)
      stat_add(st, ce_tof<T>(row[j]));
    const T* body = row + sp.head;
    for (int vi = threadIdx.x; vi < sp.nvec; vi += kT) {
      T zv[VEC];
      *reinterpret_cast<int4*>(zv) =
          *reinterpret_cast<const int4*>(body + (long)vi * VEC);
      float f[VEC];
      float vmax = -INFINITY;
      #pragma unroll
      for (int i = 0; i < VEC; ++i) {
        f[i] = ce_tof<T>(zv[i]);
        vmax = fmaxf(vmax, f[i]);
      }
      // one rescale per vector instead of one per element
      if (vmax > st.m) {
        st.s *= exp_diff(st.m, vmax);
        st.m = vmax;
      }
      #pragma unroll
      for (int i = 0; i < VEC; ++i) {
        st.s += exp_diff(f[i], st.m);
        st.sz += f[i];
      }
    }
    for (int j = sp.tail0 + threadIdx.x; j < V; j += kT)
      stat_add(st, ce_tof<T>(row[j]));

    // wave-64 butterfly, then the four wave results through LDS
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      Stat o;
      o.m = __shfl_xor(st.m, off, 64);
      o.s = __shfl_xor(st.s, off, 64);
      o.sz = __shfl_xor(st.sz, off, 64);
      st = stat_merge(st, o);
    }
    if (lane == 0) {
      lds[wave * 3 + 0] = st.m;
      lds[wave * 3 + 1] = st.s;
      lds[wave * 3 + 2] = st.sz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      Stat tot{lds[0], lds[1], lds[2]};
      #pragma unroll
      for (int w = 1; w < kWaves; ++w)
        tot = stat_merge(tot, Stat{lds[w * 3], lds[w * 3 + 1],
                                   lds[w * 3 + 2]});
      const float logs = logf(tot.s);
      // lse = m + log(s), and what that sum rounded away (TwoSum)
      const float lse = tot.m + logs;
      const float bv = lse - tot.m;
      lse_out[r] = lse;
      lse_lo_out[r] = (tot.m - (lse - bv)) + (logs - bv);
      const int64_t t = targets[r];
      float loss;
      if (t == ignore_index) {
        loss = 0.f;
      } else if (t < 0 || t >= (int64_t)V) {
        loss = std::numeric_limits<float>::quiet_NaN();
      } else {
        // lse - z_t as (m - z_t) + log(s): no cancellation against a
        // large max
        const float nll = (tot.m - ce_tof<T>(row[t])) + logs;
        const float smooth = lse - tot.sz / (float)V;
        loss = (1.f - smoothing) * nll + smoothing * smooth +
               z_loss * lse * lse;
      }
      loss_rows[r] = loss;
    }
    __syncthreads();  // lds is reused by the next row
  }
}

// --------------------------------------------------------------------
// backward: one block per row; `out` may alias `logits`
// --------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kT) void ce_bwd_kernel(
    const T* logits, T* out, const float* __restrict__ lse_in,
    const float* __restrict__ lse_lo_in,
    const int64_t* __restrict__ targets,
    const float* __restrict__ gscale, long R, int V,
    int64_t ignore_index, float smoothing, float z_loss) {
  constexpr int VEC = CeVec<T>::V;
  const float g = gscale[0];

  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const T* row = logits + r * (long)V;
    T* orow = out + r * (long)V;
    const RowSplit sp = split_row(row, V);
    const int64_t t64 = targets[r];
    // a target outside [0, V) is never turned into an index: the row
    // (ignored or invalid) is written as zeros
    const bool live = t64 != ignore_index && t64 >= 0 && t64 < (int64_t)V;
    const int t = live ? (int)t64 : -1;
    const float lse = lse_in[r];
    const float lse_lo = lse_lo_in[r];
    const float kp = 1.f + 2.f * z_loss * lse;
    const float kt = 1.f - smoothing;
    const float ku = smoothing / (float)V;

    auto grad = [&](float z, int j) -> float {
      if (!live) return 0.f;
      return g * (kp * expf((z - lse) - lse_lo) - (j == t ? kt : 0.f) - ku);
    };

    for (int j = threadIdx.x; j < sp.head; j += kT)
      orow[j] = ce_fromf<T>(grad(ce_tof<T>(row[j]), j));
    const T* body = row + sp.head;
    T* obody = orow + sp.head;
    for (int vi = threadIdx.x; vi < sp.nvec; vi += kT) {
      T zv[VEC];
      *reinterpret_cast<int4*>(zv) =
          *reinterpret_cast<const int4*>(body + (long)vi * VEC);
      const int j0 = sp.head + vi * VEC;
      #pragma unroll
      for (int i = 0; i < VEC; ++i)
        zv[i] = ce_fromf<T>(grad(ce_tof<T>(zv[i]), j0 + i));
      *reinterpret_cast<int4*>(obody + (long)vi * VEC) =
          *reinterpret_cast<const int4*>(zv);
    }
    for (int j = sp.tail0 + threadIdx.x; j < V; j += kT)
      orow[j] = ce_fromf<T>(grad(ce_tof<T>(row[j]), j));
  }
}

void check_common(const torch::Tensor& logits, const torch::Tensor& targets,
                  double label_smoothing, double z_loss) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              logits.is_contiguous(),
              "fused_ce: logits must be a contiguous [R, V] GPU tensor");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 ||
              logits.scalar_type() == at::kFloat,
              "fused_ce: logits must be bf16 or fp32");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == at::kLong &&
              targets.dim() == 1 && targets.is_contiguous() &&
              targets.size(0) == logits.size(0) &&
              targets.device() == logits.device(),
              "fused_ce: targets must be a contiguous int64 [R] tensor on "
              "the logits' device");
  TORCH_CHECK(logits.size(1) > 0 &&
              logits.size(1) <= std::numeric_limits<int>::max() / 2,
              "fused_ce: V out of range");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0 &&
              z_loss >= 0.0, "fused_ce: bad label_smoothing / z_loss");
}

inline unsigned ce_grid(long R) {
  return (unsigned)(R < kMaxGrid ? R : kMaxGrid);
}

}  // namespace

std::vector<torch::Tensor> fused_ce_fwd(torch::Tensor logits,
                                        torch::Tensor targets,
                                        int64_t ignore_index,
                                        double label_smoothing,
                                        double z_loss) {
  check_common(logits, targets, label_smoothing, z_loss);
  const long R = logits.size(0);
  const int V = (int)logits.size(1);
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss_rows = torch::empty({R}, fopt);
  auto lse = torch::empty({R}, fopt);
  auto lse_lo = torch::empty({R}, fopt);
  if (R == 0) return {loss_rows, lse, lse_lo};
  auto stream = at::hip::getCurrentHIPStream().stream();
  if (logits.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(ce_fwd_kernel<__hip_bfloat16>, dim3(ce_grid(R)),
        dim3(kT), 0, stream,
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        targets.data_ptr<int64_t>(), loss_rows.data_ptr<float>(),
        lse.data_ptr<float>(), lse_lo.data_ptr<float>(), R, V,
        ignore_index, (float)label_smoothing, (float)z_loss);
  } else {
    hipLaunchKernelGGL(ce_fwd_kernel<float>, dim3(ce_grid(R)), dim3(kT),
        0, stream, logits.data_ptr<float>(),
        targets.data_ptr<int64_t>(), loss_rows.data_ptr<float>(),
        lse.data_ptr<float>(), lse_lo.data_ptr<float>(), R, V,
        ignore_index, (float)label_smoothing, (float)z_loss);
  }
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "fused_ce_fwd: ", hipGetErrorString(e));
  return {loss_rows, lse, lse_lo};
}

torch::Tensor fused_ce_bwd(torch::Tensor logits, torch::Tensor lse,
                           torch::Tensor lse_lo, torch::Tensor targets, torch::Tensor gscale,
                           int64_t ignore_index, double label_smoothing,
                           double z_loss, bool inplace) {
  check_common(logits, targets, label_smoothing, z_loss);
  const long R = logits.size(0);
  const int V = (int)logits.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
              lse.is_contiguous() && lse.numel() == R &&
              lse.device() == logits.device(),
              "fused_ce_bwd: lse must be a contiguous fp32 [R] tensor");
  TORCH_CHECK(lse_lo.is_cuda() && lse_lo.scalar_type() == at::kFloat &&
              lse_lo.is_contiguous() && lse_lo.numel() == R &&
              lse_lo.device() == logits.device(),
              "fused_ce_bwd: lse_lo must be a contiguous fp32 [R] tensor");
  TORCH_CHECK(gscale.is_cuda() && gscale.scalar_type() == at::kFloat &&
              gscale.numel() == 1 && gscale.device() == logits.device(),
              "fused_ce_bwd: gscale must be a 1-element fp32 tensor on "
              "the logits' device");
  auto out = inplace ? logits : torch::empty_like(logits);
  // the 16-byte body of a row is located from the input's address; the
  // output must be congruent to it for its vector stores
  TORCH_CHECK(((reinterpret_cast<uintptr_t>(out.data_ptr()) ^
                reinterpret_cast<uintptr_t>(logits.data_ptr())) & 15u) == 0,
              "fused_ce_bwd: logits storage is not 16-byte aligned; use "
              "inplace=True or a fresh tensor");
  if (R == 0) return out;
  auto stream = at::hip::getCurrentHIPStream().stream();
  if (logits.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(ce_bwd_kernel<__hip_bfloat16>, dim3(ce_grid(R)),
        dim3(kT), 0, stream,
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
        lse.data_ptr<float>(), lse_lo.data_ptr<float>(),
        targets.data_ptr<int64_t>(),
        gscale.data_ptr<float>(), R, V, ignore_index,
        (float)label_smoothing, (float)z_loss);
  } else {
    hipLaunchKernelGGL(ce_bwd_kernel<float>, dim3(ce_grid(R)), dim3(kT),
        0, stream, logits.data_ptr<float>(), out.data_ptr<float>(),
        lse.data_ptr<float>(), lse_lo.data_ptr<float>(),
        targets.data_ptr<int64_t>(),
        gscale.data_ptr<float>(), R, V, ignore_index,
        (float)label_smoothing, (float)z_loss);
  }
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "fused_ce_bwd: ", hipGetErrorString(e));
  return out;
}
