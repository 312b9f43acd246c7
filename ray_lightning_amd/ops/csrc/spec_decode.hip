// One step of prompt-lookup speculative decoding after the LM head, in
// one launch: sampling at the T1 = T + 1 positions of every row, the
// acceptance of the drafted tokens, the EOS / padding / output write, the
// repair of the KV cache's lengths, and the draft of the next step by
// n-gram lookup in the row's own history. gfx950. docs/DESIGN.md §17 has
// the contract; ops/spec_decode.py repeats it.
//
// Shape of the kernel:
//  - grid (T1, B), 1024 threads. Workgroup (t, b) runs the sampling
//    pipeline of sample_core.h on logits[b, t, :] with seed seeds[b] and
//    counter emitted[b] + t, and stores tok[b, t].
//  - hand-over without waiting: thread 0 stores the token, fences, and
//    adds 1 to done[b]. The workgroup that reads T1 - 1 back is the
//    row's last: all the row's tokens are visible to it. It puts done[b]
//    back to 0 and goes on; every other workgroup ends there. No
//    workgroup waits for another, so no order of scheduling can stall.
//  - commit: thread 0 of that workgroup counts the accepted drafts and
//    writes at most T1 tokens, then the row's scalars.
//  - draft: the row's history out[b, 0:col] is staged once as int32 in
//    LDS, over the sampler's histograms, which are dead by then: 64 KB
//    for the 16384 tokens at most, so two workgroups still share a CU's
//    160 KB. Thread i tests the candidate end positions i, i + 1024, ...:
//    it compares up to ngram tokens backwards against the history's
//    suffix, which it holds in registers, reading LDS only. The key
//    (match length << 32 | end position) is maximised by shuffles within
//    a wave and through 16 LDS words across the waves: the longest match,
//    and the latest among equals. Thread 0 writes the continuation, which
//    runs on into the draft itself when it passes the end of the history.
//  - integer work from the token on: exact and repeatable.
//  - every loop bound is a constant or an operand's extent.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>

#include "sample_core.h"

// fp32 math of this file stays on the scalar-per-lane VALU forms
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

namespace {

constexpr int kSpMaxT1 = 16;
constexpr int kSpMaxNgram = 8;
constexpr int kSpMaxL = 16384;

struct SpecArgs {
  SampleCfg cfg;
  const void* logits;     // [B, T1, V] bf16 or fp32
  const int64_t* seeds;   // [B]
  const int64_t* draft;   // [B, T1 - 1], rows draft_stride apart
  int64_t* tok;           // [B, T1]
  int* done;              // [B], 0 before and after
  bool* finished;         // [B]
  int64_t* out;           // [B, L]
  int64_t* col;           // [B]
  int64_t* emitted;       // [B]
  int* pos;               // [B]
  int64_t* n_commit;      // [B]
  int64_t* next_idx;      // [B, 1 + Tn]
  int64_t eos, pad, limit;
  long draft_stride;
  int L, T1, Tn, ngram;
};

struct SpecLds {
  union {
    SampleLds sample;
    int hist[kSpMaxL];
  } u;
  unsigned long long wave_key[kSmWaves];
  long long tok;
  int d[kSpMaxT1];
  int hn;    // tokens of history, after the commit
  int last;  // this workgroup is its row's last
};

template <bool BF16, int IPT>
__global__ __launch_bounds__(kSmThreads) void spec_kernel(SpecArgs a) {
  __shared__ SpecLds s;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int T1 = a.T1;
  // read before the hand-over: the row's last workgroup changes it
  const uint64_t step = (uint64_t)(a.emitted[b] + t);
  const char* rowp = reinterpret_cast<const char*>(a.logits) +
                     ((long)b * T1 + t) * a.cfg.V * (BF16 ? 2 : 4);
  sm_sample_row<BF16, IPT>(rowp, a.cfg, a.seeds + b, (uint32_t)step,
                           (uint32_t)(step >> 32), s.u.sample,
                           [&](int64_t tok) { s.tok = tok; });
  __syncthreads();
  int64_t* tok_row = a.tok + (long)b * T1;
  if (tid == 0) {
    tok_row[t] = s.tok;
    __threadfence();
    const bool last = atomicAdd(&a.done[b], 1) == T1 - 1;
    if (last) a.done[b] = 0;  // nobody else touches it in this launch
    s.last = last;
  }
  __syncthreads();
  if (!s.last) return;  // uniform

  // ---- commit: the row's T1 tokens are visible from here on
  if (tid == 0) {
    __threadfence();
    const int T = T1 - 1;
    bool fin = a.finished[b];
    int acc = 0;
    bool run = true;
    for (int j = 0; j < T; ++j) {
      const int64_t x = __hip_atomic_load(
          tok_row + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      run = run && (fin || x == a.draft[b * a.draft_stride + j]);
      acc += run;
    }
    const int64_t em = a.emitted[b], c = a.col[b];
    const int64_t room = a.limit - em;
    const int n = room <= 0 ? 0 : (int)(room < acc + 1 ? room : acc + 1);
    for (int j = 0; j < n; ++j) {
      int64_t x = __hip_atomic_load(tok_row + j, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
      if (fin) x = a.pad;
      fin = fin || x == a.eos;
      const int64_t cc = c + j;
      if (cc >= 0 && cc < a.L) a.out[(long)b * a.L + cc] = x;
    }
    a.finished[b] = fin;
    a.col[b] = c + n;
    a.emitted[b] = em + n;
    a.pos[b] += n - T1;
    a.n_commit[b] = n;
    const int64_t end = c + n;
    s.hn = end < 0 ? 0 : (int)(end > a.L ? a.L : end);
  }
  __syncthreads();  // also orders thread 0's stores to out before the loads

  // ---- draft: history into LDS, over the sampler's histograms
  const int hn = s.hn;
  int64_t* nx = a.next_idx + (long)b * (1 + a.Tn);
  if (hn == 0) {  // uniform: nothing to look up
    if (tid <= a.Tn) nx[tid] = a.pad;
    return;
  }
  const int64_t* h = a.out + (long)b * a.L;
  for (int i = tid; i < hn; i += kSmThreads) s.u.hist[i] = (int)h[i];
  __syncthreads();
  int suf[kSpMaxNgram];  // suf[k] = h[hn - 1 - k]
  #pragma unroll
  for (int k = 0; k < kSpMaxNgram; ++k)
    suf[k] = s.u.hist[hn - 1 - k > 0 ? hn - 1 - k : 0];
  // candidate e: the earlier occurrence ends at e <= hn - 2
  unsigned long long key = 0;
  for (int e = tid; e < hn - 1; e += kSmThreads) {
    unsigned m = 0;
    bool run = true;
    #pragma unroll
    for (int k = 0; k < kSpMaxNgram; ++k) {
      run = run && k < a.ngram && e - k >= 0 &&
            s.u.hist[e - k > 0 ? e - k : 0] == suf[k];
      m += run;
    }
    const unsigned long long mine =
        (unsigned long long)m << 32 | (unsigned)e;
    key = mine > key ? mine : key;
  }
  #pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if ((tid & 63) == 0) s.wave_key[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    #pragma unroll
    for (int w = 0; w < kSmWaves; ++w)
      key = s.wave_key[w] > key ? s.wave_key[w] : key;
    const bool match = (key >> 32) != 0;
    const int from = match ? (int)(uint32_t)key + 1 : hn - 1;
    nx[0] = s.u.hist[hn - 1];
    for (int j = 0; j < a.Tn; ++j) {
      // a match continues, into the draft itself past the history's end;
      // no match repeats the last token
      const int i = match ? from + j : from;
      const int x = i < hn ? s.u.hist[i] : s.d[i - hn];
      s.d[j] = x;
      nx[1 + j] = x;
    }
  }
}

}  // namespace

#pragma clang attribute pop

namespace {

template <bool BF16>
void sp_launch(int ipt, dim3 grid, hipStream_t stream, const SpecArgs& a) {
  switch (ipt) {
    case 1:
      hipLaunchKernelGGL((spec_kernel<BF16, 1>), grid, dim3(kSmThreads), 0,
                         stream, a);
      break;
    case 4:
      hipLaunchKernelGGL((spec_kernel<BF16, 4>), grid, dim3(kSmThreads), 0,
                         stream, a);
      break;
    case 16:
      hipLaunchKernelGGL((spec_kernel<BF16, 16>), grid, dim3(kSmThreads), 0,
                         stream, a);
      break;
    default:
      hipLaunchKernelGGL((spec_kernel<BF16, 64>), grid, dim3(kSmThreads), 0,
                         stream, a);
  }
}

}  // namespace

// What spec_step would hold per thread for logits [B, T1, V]: the worst
// alignment over all B * T1 rows decides; 0: not served.
long spec_items_per_thread(torch::Tensor logits) {
  if (logits.dim() != 3 || logits.size(1) < 1 ||
      logits.size(1) > kSpMaxT1 || logits.size(2) < 1 ||
      logits.size(2) > kSmMaxV)
    return 0;
  return sm_items_per_thread(
      reinterpret_cast<uintptr_t>(logits.data_ptr()), logits.size(2),
      logits.element_size());
}

// Returns (tok [B, T1], n_commit [B], next_idx [B, 1 + next_T]); updates
// done, finished, out, col, emitted and pos in place.
std::vector<torch::Tensor> spec_step(
    torch::Tensor logits, torch::Tensor draft, torch::Tensor seeds,
    torch::Tensor emitted, int64_t limit, double temperature,
    c10::optional<int64_t> top_k, c10::optional<double> top_p,
    torch::Tensor finished, int64_t eos, int64_t pad, torch::Tensor out,
    torch::Tensor col, torch::Tensor pos, torch::Tensor done, int64_t ngram,
    int64_t next_T) {
  TORCH_CHECK_VALUE(logits.is_cuda() && logits.dim() == 3 &&
                    logits.is_contiguous() &&
                    (logits.scalar_type() == at::kBFloat16 ||
                     logits.scalar_type() == at::kFloat),
                    "spec_step: logits must be a contiguous bf16 or fp32 "
                    "GPU tensor [B, T1, V]");
  const int64_t B = logits.size(0), T1 = logits.size(1), V = logits.size(2);
  TORCH_CHECK_VALUE(V >= 1 && V <= kSmMaxV, "spec_step: V = ", V,
                    " is outside [1, ", kSmMaxV, "]");
  TORCH_CHECK_VALUE(T1 >= 1 && T1 <= kSpMaxT1, "spec_step: T1 = ", T1,
                    " is outside [1, ", kSpMaxT1, "]");
  TORCH_CHECK_VALUE(B <= 65535, "spec_step: B = ", B,
                    " exceeds the grid's extent");
  auto row_of_b = [&](const torch::Tensor& t, at::ScalarType ty,
                      const char* what) {
    TORCH_CHECK_VALUE(t.is_cuda() && t.device() == logits.device() &&
                      t.scalar_type() == ty && t.dim() == 1 &&
                      t.size(0) == B && t.is_contiguous(),
                      "spec_step: ", what, " [B] on logits' device");
  };
  row_of_b(seeds, at::kLong, "seeds must be a contiguous int64");
  row_of_b(emitted, at::kLong, "emitted must be a contiguous int64");
  row_of_b(finished, at::kBool, "finished must be a contiguous bool");
  row_of_b(col, at::kLong, "col must be a contiguous int64");
  row_of_b(pos, at::kInt, "pos must be a contiguous int32");
  row_of_b(done, at::kInt, "done must be a contiguous int32");
  // rows may lie apart: the last call's next_idx[:, 1:] is served as is
  TORCH_CHECK_VALUE(draft.is_cuda() && draft.device() == logits.device() &&
                    draft.scalar_type() == at::kLong && draft.dim() == 2 &&
                    draft.size(0) == B && draft.size(1) == T1 - 1 &&
                    (T1 == 1 || draft.stride(1) == 1) &&
                    (T1 == 1 || B <= 1 || draft.stride(0) >= T1 - 1),
                    "spec_step: draft must be int64 [B, T1 - 1] on logits' "
                    "device with unit stride along a row");
  TORCH_CHECK_VALUE(out.is_cuda() && out.device() == logits.device() &&
                    out.scalar_type() == at::kLong && out.dim() == 2 &&
                    out.size(0) == B && out.is_contiguous(),
                    "spec_step: out must be a contiguous int64 [B, L] on "
                    "logits' device");
  const int64_t L = out.size(1);
  TORCH_CHECK_VALUE(L >= 1 && L <= kSpMaxL, "spec_step: out holds ", L,
                    " tokens per row, outside [1, ", kSpMaxL, "]");
  TORCH_CHECK_VALUE(limit >= 0, "spec_step: limit must be >= 0");
  TORCH_CHECK_VALUE(ngram >= 1 && ngram <= kSpMaxNgram,
                    "spec_step: ngram = ", ngram, " is outside [1, ",
                    kSpMaxNgram, "]");
  TORCH_CHECK_VALUE(next_T >= 0 && next_T < kSpMaxT1,
                    "spec_step: next_T = ", next_T, " is outside [0, ",
                    kSpMaxT1 - 1, "]");
  // the history is searched as int32
  TORCH_CHECK_VALUE(eos >= -1 && eos <= INT32_MAX,
                    "spec_step: eos must be -1 (none) or a token id");
  TORCH_CHECK_VALUE(pad >= 0 && pad <= INT32_MAX,
                    "spec_step: pad must be a token id");
  TORCH_CHECK_VALUE(temperature >= 0.0 && std::isfinite(temperature),
                    "spec_step: temperature must be finite and >= 0");
  const float c =
      temperature > 0.0 ? (float)(1.4426950408889634 / temperature) : 0.f;
  TORCH_CHECK_VALUE(std::isfinite(c), "spec_step: temperature = ",
                    temperature, " is too small for fp32");
  TORCH_CHECK_VALUE(!top_k.has_value() || *top_k >= 1,
                    "spec_step: top_k must be >= 1");
  TORCH_CHECK_VALUE(!top_p.has_value() || (*top_p > 0.0 && *top_p <= 1.0),
                    "spec_step: top_p must be in (0, 1]");
  const int64_t ipt = sm_items_per_thread(
      reinterpret_cast<uintptr_t>(logits.data_ptr()), V,
      logits.element_size());
  TORCH_CHECK_VALUE(ipt != 0, "spec_step: V = ", V, " needs rows that start "
                    "on 16-byte boundaries");

  auto tok = torch::empty({B, T1}, seeds.options());
  auto n_commit = torch::empty({B}, seeds.options());
  auto next_idx = torch::empty({B, 1 + next_T}, seeds.options());
  if (B == 0) return {tok, n_commit, next_idx};
  SpecArgs a;
  a.cfg.top_p = top_p.value_or(1.0);
  a.cfg.V = (int)V;
  a.cfg.top_k = top_k.has_value() && *top_k < V ? (uint32_t)*top_k : 0u;
  a.cfg.c = c;
  a.cfg.greedy = temperature == 0.0;
  a.logits = logits.data_ptr();
  a.seeds = seeds.data_ptr<int64_t>();
  a.draft = draft.data_ptr<int64_t>();
  a.tok = tok.data_ptr<int64_t>();
  a.done = done.data_ptr<int>();
  a.finished = finished.data_ptr<bool>();
  a.out = out.data_ptr<int64_t>();
  a.col = col.data_ptr<int64_t>();
  a.emitted = emitted.data_ptr<int64_t>();
  a.pos = pos.data_ptr<int>();
  a.n_commit = n_commit.data_ptr<int64_t>();
  a.next_idx = next_idx.data_ptr<int64_t>();
  a.eos = eos;
  a.pad = pad;
  a.limit = limit;
  a.draft_stride = T1 == 1 ? 0 : draft.stride(0);
  a.L = (int)L;
  a.T1 = (int)T1;
  a.Tn = (int)next_T;
  a.ngram = (int)ngram;
  auto stream = at::hip::getCurrentHIPStream().stream();
  const dim3 grid((unsigned)T1, (unsigned)B);
  if (logits.scalar_type() == at::kBFloat16)
    sp_launch<true>((int)ipt, grid, stream, a);
  else
    sp_launch<false>((int)ipt, grid, stream, a);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "spec_step: ", hipGetErrorString(e));
  return {tok, n_commit, next_idx};
}
