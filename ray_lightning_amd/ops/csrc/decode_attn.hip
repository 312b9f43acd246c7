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
// pos is read on the device only. A row whose pos[b] lies outside
// [0, max_pos] is inactive: all its positions are invalid, so it forms no
// address from pos[b], stores nothing and its output is zero.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cmath>

namespace {

constexpr int kDaThreads = 256;
constexpr int kDaWaves = kDaThreads / 64;
constexpr int kDaHs = 64;              // head size
constexpr int kDaStep = kDaWaves * 8;  // positions per workgroup load
constexpr int kDaPartial = kDaHs + 2;  // floats: 64 acc, max, sum
// KV positions per workgroup; profiles/gpt2_generate.md has the
// alternatives measured
constexpr int kDaChunk = 128;

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
torch::Tensor da_checked(torch::Tensor qkv, torch::Tensor k_cache,
                         torch::Tensor v_cache, torch::Tensor pos,
                         int64_t max_pos, double scale, int64_t chunk) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
              qkv.dim() == 2 && qkv.is_contiguous(),
              "decode_attn_fwd: qkv must be a contiguous bf16 GPU tensor "
              "[B, 3*H*64]");
  for (const torch::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(c->is_cuda() && c->device() == qkv.device() &&
                c->scalar_type() == at::kBFloat16 && c->dim() == 4 &&
                c->is_contiguous() && c->size(3) == kDaHs,
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
                              int64_t max_pos, double scale) {
  return da_checked(qkv, k_cache, v_cache, pos, max_pos, scale, kDaChunk);
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
