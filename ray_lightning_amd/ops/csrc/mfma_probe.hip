// MFMA fragment-layout probe for gfx950 (cdna4_isa.md is not shipped in
// this environment, so the lane->element maps used by flash_attn.hip
// are verified empirically: tests/test_flash_attn_gpu.py checks this
// kernel's 16x16 output against torch.matmul with ASYMMETRIC operands
// per the guide's A=I-check rule).
//
// Assumed maps (CDNA3 pattern extended to gfx950's 2xK):
//   mfma_f32_16x16x32_bf16:
//     A[16M x 32K]: lane l, elem i (of 8) -> row = l & 15,
//                                            k   = (l >> 4) * 8 + i
//     B[32K x 16N]: lane l, elem i        -> col = l & 15,
//                                            k   = (l >> 4) * 8 + i
//     C/D (4 f32): col = l & 15, row = (l >> 4) * 4 + reg   (guide §3)
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__global__ void mfma_probe_16x16x32(const __hip_bfloat16* __restrict__ A,
                                    const __hip_bfloat16* __restrict__ B,
                                    float* __restrict__ C) {
  // one wave; A is [16, 32] row-major, B is [32, 16] row-major
  const int l = threadIdx.x;
  if (l >= 64) return;
  bf16x8 a, b;
  const int arow = l & 15, kgrp = (l >> 4) * 8;
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = *reinterpret_cast<const __bf16*>(&A[arow * 32 + kgrp + i]);
    b[i] = *reinterpret_cast<const __bf16*>(&B[(kgrp + i) * 16 + (l & 15)]);
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = (l >> 4) * 4 + r;
    const int col = l & 15;
    C[row * 16 + col] = c[r];
  }
}

}  // namespace

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
              B.sizes() == torch::IntArrayRef({32, 16}) &&
              A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16);
  auto C = torch::zeros({16, 16},
                        A.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(mfma_probe_16x16x32, dim3(1), dim3(64), 0, stream,
                     reinterpret_cast<const __hip_bfloat16*>(A.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(B.data_ptr()),
                     C.data_ptr<float>());
  return C;
}

namespace {
// permlane{16,32}_swap semantics probe: a = 0x1000+lane, b = 0x2000+lane.
// Row 0/1: permlane32_swap results (r0, r1); row 2/3: permlane16_swap.
__global__ void permlane_swap_probe_kernel(unsigned* __restrict__ out) {
  const unsigned lane = threadIdx.x;
  if (lane >= 64) return;
  const unsigned a = 0x1000u + lane;
  const unsigned b = 0x2000u + lane;
  {
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    out[lane] = r[0];
    out[64 + lane] = r[1];
  }
  {
    auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    out[128 + lane] = r[0];
    out[192 + lane] = r[1];
  }
}
}  // namespace

torch::Tensor permlane_swap_probe() {
  auto out = torch::zeros({4, 64}, torch::dtype(at::kInt)
                                       .device(at::kCUDA));
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(permlane_swap_probe_kernel, dim3(1), dim3(64), 0,
                     stream,
                     reinterpret_cast<unsigned*>(out.data_ptr()));
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "permlane_swap_probe: ",
              hipGetErrorString(e));
  return out;
}

namespace {
// ds_read_b64_tr_b16 semantics probe: LDS u16[4096] filled with its own
// index; each lane reads 8 B at addr = a*lane + b*(lane&15) + c*(lane>>4)
// and we dump the 4 u16 element-indices each lane received.
__global__ void tr16_probe_kernel(unsigned short* __restrict__ out,
                                  int a, int b, int c) {
  __shared__ unsigned short lds[4096];
  for (int i = threadIdx.x; i < 4096; i += blockDim.x)
    lds[i] = (unsigned short)i;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const int addr = a * lane + b * (lane & 15) + c * (lane >> 4);
  // AS(3) pointer -> 32-bit LDS byte offset for the ds instruction
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  const unsigned base =
      (unsigned)(size_t)(__attribute__((address_space(3))) char*)
          (void*)lds;
  uint2v r;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %1\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r)
      : "v"(base + (unsigned)addr)
      : "memory");
  out[lane * 4 + 0] = (unsigned short)(r[0] & 0xffff);
  out[lane * 4 + 1] = (unsigned short)(r[0] >> 16);
  out[lane * 4 + 2] = (unsigned short)(r[1] & 0xffff);
  out[lane * 4 + 3] = (unsigned short)(r[1] >> 16);
}
}  // namespace

torch::Tensor tr16_probe(long a, long b, long c) {
  auto out = torch::zeros({64, 4}, torch::dtype(at::kShort)
                                       .device(at::kCUDA));
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(256), 0, stream,
                     reinterpret_cast<unsigned short*>(out.data_ptr()),
                     (int)a, (int)b, (int)c);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "tr16_probe: ", hipGetErrorString(e));
  return out;
}

namespace {
using f32x16 = __attribute__((ext_vector_type(16))) float;

// 32x32x16 bf16 layout probe. Assumed maps (guide §3 + CDNA pattern):
//   A[32M x 16K]: lane l elem i -> row = l & 31, k = (l >> 5) * 8 + i
//   B[16K x 32N]: lane l elem i -> col = l & 31, k = (l >> 5) * 8 + i
//   C (16 f32):   col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
__global__ void mfma_probe_32x32x16(const __hip_bfloat16* __restrict__ A,
                                    const __hip_bfloat16* __restrict__ B,
                                    float* __restrict__ C) {
  const int l = threadIdx.x;
  if (l >= 64) return;
  bf16x8 a, b;
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = (__bf16)(float)A[(l & 31) * 16 + (l >> 5) * 8 + i];
    b[i] = (__bf16)(float)B[((l >> 5) * 8 + i) * 32 + (l & 31)];
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    C[row * 32 + (l & 31)] = acc[r];
  }
}
}  // namespace

torch::Tensor mfma_probe32(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) &&
              B.sizes() == at::IntArrayRef({16, 32}));
  auto C = torch::zeros({32, 32},
                        A.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(mfma_probe_32x32x16, dim3(1), dim3(64), 0, stream,
      reinterpret_cast<const __hip_bfloat16*>(A.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(B.data_ptr()),
      C.data_ptr<float>());
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "mfma_probe32: ", hipGetErrorString(e));
  return C;
}
