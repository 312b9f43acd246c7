// Token sampling for generation in one launch: top-k, top-p (nucleus),
// a counter-based Philox draw, and the EOS / padding / output-write
// epilogue of the decode loop. bf16 or fp32 logits [B, V], V <= 65536,
// gfx950. docs/DESIGN.md §16 has the contract; in short, for row b:
//
//   K   = { i : l_i >= the top_k-th largest logit }         (ties kept)
//   w_i = exp2((l_i - max l) * c),  c = fp32(log2 e / temperature)
//   m_i = floor(w_i * 2^40) as a 64-bit integer, 0 outside K
//   P   = clamp(llrint(top_p * M), 1, M),  M = sum m_i
//   N   = { i in K : sum of m_j over l_j > l_i  <  P }      (ties kept)
//   x   = word 0 of Philox4x32-10(seeds[b], (step_lo, step_hi, 0, 0))
//   r   = floor(M_N * x / 2^32),  M_N = sum of m_i over N
//   token = lowest i in N whose inclusive mass prefix (index order) > r
//
// Every sum, histogram, scan and comparison of mass is 64-bit integer
// arithmetic, so no result depends on an order of summation: given the
// fp32 weights the token is exact, repeatable bit for bit, and a function
// of the row's logits, seeds[b] and step alone.
//
// The pipeline of one row in one workgroup, and the shape of the kernel,
// are in sample_core.h, which spec_decode.hip shares; this file holds
// the epilogue, the kernel around both and the one checked host path.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cfloat>
#include <cmath>

#include "sample_core.h"

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

struct SampleArgs {
  SampleCfg cfg;
  const void* logits;      // [B, V] bf16 or fp32
  const int64_t* seeds;    // [B]
  int64_t* tokens;         // [B]
  bool* finished;          // [B] or null: no epilogue
  int64_t* out;            // [B, L]
  const int64_t* col;      // [B]
  int64_t eos, pad;
  int L;
  uint32_t step_lo, step_hi;
};

__device__ __forceinline__ void sm_emit(const SampleArgs& a, int b,
                                        int64_t tok) {
  if (a.finished != nullptr) {
    if (a.finished[b]) tok = a.pad;
    else if (tok == a.eos) a.finished[b] = true;
    const int64_t col = a.col[b];
    if (col >= 0 && col < a.L) a.out[(long)b * a.L + col] = tok;
  }
  a.tokens[b] = tok;
}

template <bool BF16, int IPT>
__global__ __launch_bounds__(kSmThreads) void sample_kernel(SampleArgs a) {
  __shared__ SampleLds s;
  const int b = blockIdx.x;
  const char* rowp = reinterpret_cast<const char*>(a.logits) +
                     (long)b * a.cfg.V * (BF16 ? 2 : 4);
  sm_sample_row<BF16, IPT>(rowp, a.cfg, a.seeds + b, a.step_lo, a.step_hi,
                           s, [&](int64_t tok) { sm_emit(a, b, tok); });
}

}  // namespace

#pragma clang attribute pop

namespace {

template <bool BF16>
void sm_launch(int ipt, unsigned B, hipStream_t stream, const SampleArgs& a) {
  switch (ipt) {
    case 1:
      hipLaunchKernelGGL((sample_kernel<BF16, 1>), dim3(B), dim3(kSmThreads),
                         0, stream, a);
      break;
    case 4:
      hipLaunchKernelGGL((sample_kernel<BF16, 4>), dim3(B), dim3(kSmThreads),
                         0, stream, a);
      break;
    case 16:
      hipLaunchKernelGGL((sample_kernel<BF16, 16>), dim3(B), dim3(kSmThreads),
                         0, stream, a);
      break;
    default:
      hipLaunchKernelGGL((sample_kernel<BF16, 64>), dim3(B), dim3(kSmThreads),
                         0, stream, a);
  }
}

}  // namespace

// What sample_fwd would hold per thread for these logits; 0: not served.
long sample_items_per_thread(torch::Tensor logits) {
  if (logits.dim() != 2 || logits.size(1) < 1 || logits.size(1) > kSmMaxV)
    return 0;
  return sm_items_per_thread(
      reinterpret_cast<uintptr_t>(logits.data_ptr()), logits.size(1),
      logits.element_size());
}

torch::Tensor sample_fwd(torch::Tensor logits, torch::Tensor seeds,
                         int64_t step, double temperature,
                         c10::optional<int64_t> top_k,
                         c10::optional<double> top_p,
                         c10::optional<torch::Tensor> finished, int64_t eos,
                         int64_t pad, c10::optional<torch::Tensor> out,
                         c10::optional<torch::Tensor> col) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              logits.is_contiguous() &&
              (logits.scalar_type() == at::kBFloat16 ||
               logits.scalar_type() == at::kFloat),
              "sample_fwd: logits must be a contiguous bf16 or fp32 GPU "
              "tensor [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= kSmMaxV, "sample_fwd: V = ", V,
              " is outside [1, ", kSmMaxV, "]");
  TORCH_CHECK(B <= 65535, "sample_fwd: B = ", B,
              " exceeds the grid's extent");
  auto row_of_b = [&](const torch::Tensor& t, at::ScalarType ty,
                      const char* what) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device() &&
                t.scalar_type() == ty && t.dim() == 1 && t.size(0) == B &&
                t.is_contiguous(),
                "sample_fwd: ", what, " [B] on logits' device");
  };
  row_of_b(seeds, at::kLong, "seeds must be a contiguous int64");
  TORCH_CHECK(step >= 0, "sample_fwd: step must be >= 0");
  TORCH_CHECK(temperature >= 0.0 && std::isfinite(temperature),
              "sample_fwd: temperature must be finite and >= 0");
  const float c =
      temperature > 0.0 ? (float)(1.4426950408889634 / temperature) : 0.f;
  TORCH_CHECK(std::isfinite(c), "sample_fwd: temperature = ", temperature,
              " is too small for fp32");
  TORCH_CHECK(!top_k.has_value() || *top_k >= 1,
              "sample_fwd: top_k must be >= 1");
  TORCH_CHECK(!top_p.has_value() || (*top_p > 0.0 && *top_p <= 1.0),
              "sample_fwd: top_p must be in (0, 1]");
  const bool epilogue = finished.has_value();
  TORCH_CHECK(out.has_value() == epilogue && col.has_value() == epilogue,
              "sample_fwd: finished, out and col come together or not at "
              "all");
  int64_t L = 0;
  if (epilogue) {
    row_of_b(*finished, at::kBool, "finished must be a contiguous bool");
    row_of_b(*col, at::kLong, "col must be a contiguous int64");
    TORCH_CHECK(out->is_cuda() && out->device() == logits.device() &&
                out->scalar_type() == at::kLong && out->dim() == 2 &&
                out->size(0) == B && out->is_contiguous(),
                "sample_fwd: out must be a contiguous int64 [B, L] on "
                "logits' device");
    L = out->size(1);
    TORCH_CHECK(out->numel() < ((int64_t)1 << 31),
                "sample_fwd: 2^31 elements or more in out");
  }
  const int64_t ipt = sm_items_per_thread(
      reinterpret_cast<uintptr_t>(logits.data_ptr()), V,
      logits.element_size());
  TORCH_CHECK(ipt != 0, "sample_fwd: V = ", V, " needs rows that start on "
              "16-byte boundaries");

  auto tokens = torch::empty({B}, seeds.options());
  if (B == 0) return tokens;
  SampleArgs a;
  a.logits = logits.data_ptr();
  a.seeds = seeds.data_ptr<int64_t>();
  a.tokens = tokens.data_ptr<int64_t>();
  a.finished = epilogue ? finished->data_ptr<bool>() : nullptr;
  a.out = epilogue ? out->data_ptr<int64_t>() : nullptr;
  a.col = epilogue ? col->data_ptr<int64_t>() : nullptr;
  a.eos = eos;
  a.pad = pad;
  a.cfg.top_p = top_p.value_or(1.0);
  a.cfg.V = (int)V;
  a.L = (int)L;
  a.cfg.top_k =
      top_k.has_value() && *top_k < V ? (uint32_t)*top_k : 0u;
  a.step_lo = (uint32_t)step;
  a.step_hi = (uint32_t)((uint64_t)step >> 32);
  a.cfg.c = c;
  a.cfg.greedy = temperature == 0.0;
  auto stream = at::hip::getCurrentHIPStream().stream();
  if (logits.scalar_type() == at::kBFloat16)
    sm_launch<true>((int)ipt, (unsigned)B, stream, a);
  else
    sm_launch<false>((int)ipt, (unsigned)B, stream, a);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "sample_fwd: ", hipGetErrorString(e));
  return tokens;
}
