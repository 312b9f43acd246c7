// Input gradient of a 1x1 stride-1 convolution in NHWC (channels_last),
// with the gradient of a second consumer of the same input added in the
// epilogue:
//
//   dx[r, c] = bf16( fp32(sum_k dy[r, k] * w[k, c]) + fp32(skip[r, c]) )
//
// r = (n, h, w) flattened (R rows), k over Cout, c over Cin. At a ResNet
// bottleneck junction this replaces MIOpen's zero-fill of dx, its
// backward-data kernel and autograd's add of the two block-input
// gradients by one pass: read dy, read skip, write dx. One rounding, no
// atomics, no pre-zeroed output, fixed summation order.
//
// Shape of the kernel (mfma_f32_16x16x32_bf16, maps as in mfma_probe.hip):
//  - a workgroup is 4 wave64; it owns BN columns of Cin for its whole
//    life and keeps w^T[BN][Cout] for them in LDS (transposed while
//    staging, so a B fragment is one 16-byte LDS read along k). It walks
//    over row tiles of BM = 64*MT rows; the row tiles of a launch are
//    dealt out so that the Cin/BN workgroups that share a row tile (and
//    so its dy) sit on one XCD and reach it at about the same time.
//  - a wave owns 16*MT rows x BN columns of a row tile. Its A fragments
//    are 16-byte global loads of dy (8 consecutive k of one row), used by
//    this wave alone; its skip values are loaded at the top of the tile,
//    in the layout of the stores, so they are in flight under the MFMAs.
//  - the accumulators go through a wave-private LDS scratch, 16 rows x
//    64 columns at a time, and leave as 16-byte stores, 8 lanes to a
//    128-byte row segment.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kC1Threads = 256;
constexpr int kC1Waves = kC1Threads / 64;
constexpr int kXcds = 8;            // workgroup b runs on XCD b % 8
constexpr int kScStride = 68;       // floats per scratch row (64 + pad)
constexpr int kScFloats = 16 * kScStride;
constexpr int kWPad = 8;            // bf16 elements of padding per w^T row

// LDS writes and reads of one wave execute in order; this only keeps
// the compiler from moving them across the hand-over between lanes.
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float bf16_bits_to_float(unsigned v) {
  return __uint_as_float(v << 16);
}

template <int COUT, int BN, int MT>
__global__ __launch_bounds__(kC1Threads) void conv1x1_bwd_data_kernel(
    const unsigned short* __restrict__ dy,    // [R, COUT]
    const unsigned short* __restrict__ w,     // [COUT, Cin]
    const unsigned short* __restrict__ skip,  // [R, Cin] or nullptr
    unsigned short* __restrict__ dx,          // [R, Cin]
    long R, int Cin, long n_row_tiles) {
  constexpr int WS = COUT + kWPad;  // w^T row stride in LDS, elements
  constexpr int NT = BN / 16;       // 16-column tiles per wave
  constexpr int KS = COUT / 32;     // MFMA k-steps
  constexpr int NCH = BN / 64;      // 64-column epilogue chunks
  constexpr int BM = kC1Waves * 16 * MT;
  constexpr int KU = KS <= 4 ? KS : 2;  // k-steps unrolled
  static_assert(COUT % 32 == 0 && BN % 64 == 0, "tile shape");

  __shared__ __attribute__((aligned(16))) unsigned short wl[BN * WS];
  __shared__ __attribute__((aligned(16))) float scratch[kC1Waves][kScFloats];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;      // MFMA row/col, k group
  const int er = lane >> 3, ec = (lane & 7) * 8; // epilogue row, column

  // column tile and row lane of this workgroup (see the head comment)
  const int nct = Cin / BN;
  const int b = blockIdx.x;
  const int q = b / kXcds;
  const int ct = q % nct;
  const long rl = (long)(q / nct) * kXcds + b % kXcds;
  const long nrl = gridDim.x / nct;
  const int col0 = ct * BN;

  // stage w^T[BN][COUT]: 8 k of one column per thread, lanes along Cin
  for (int it = tid; it < BN * (COUT / 8); it += kC1Threads) {
    const int c = it % BN, kg = it / BN;
    unsigned short v[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = w[(long)(kg * 8 + j) * Cin + col0 + c];
    *reinterpret_cast<int4*>(&wl[c * WS + kg * 8]) =
        *reinterpret_cast<const int4*>(v);
  }
  __syncthreads();

  float* sc = scratch[wave];
  for (long t = rl; t < n_row_tiles; t += nrl) {
    const long row0 = t * BM + wave * (16 * MT);

    // skip, in the layout of the stores; zeros where there is none
    int4 sk[MT][NCH][2];
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      #pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        #pragma unroll
        for (int p = 0; p < 2; ++p) {
          const long row = row0 + m * 16 + p * 8 + er;
          sk[m][ch][p] = int4{0, 0, 0, 0};
          if (skip != nullptr && row < R)
            sk[m][ch][p] = *reinterpret_cast<const int4*>(
                skip + row * Cin + col0 + ch * 64 + ec);
        }

    f32x4 acc[MT][NT];
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      #pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    #pragma unroll KU
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 a[MT];
      #pragma unroll
      for (int m = 0; m < MT; ++m) {
        const long row = row0 + m * 16 + lr;
        int4 raw = int4{0, 0, 0, 0};
        if (row < R)
          raw = *reinterpret_cast<const int4*>(
              dy + row * COUT + ks * 32 + lg * 8);
        a[m] = *reinterpret_cast<const bf16x8*>(&raw);
      }
      #pragma unroll
      for (int n = 0; n < NT; ++n) {
        const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &wl[(n * 16 + lr) * WS + ks * 32 + lg * 8]);
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[m], bfrag, acc[m][n], 0, 0, 0);
      }
    }

    // epilogue: C layout (col = lane & 15, row = 4 * (lane >> 4) + reg)
    // -> scratch -> rows of 8 lanes x 8 columns
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      #pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        #pragma unroll
        for (int n4 = 0; n4 < 4; ++n4)
          #pragma unroll
          for (int i = 0; i < 4; ++i)
            sc[(lg * 4 + i) * kScStride + n4 * 16 + lr] =
                acc[m][ch * 4 + n4][i];
        wave_lds_sync();
        #pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int rin = p * 8 + er;
          const float4 v0 =
              *reinterpret_cast<const float4*>(&sc[rin * kScStride + ec]);
          const float4 v1 = *reinterpret_cast<const float4*>(
              &sc[rin * kScStride + ec + 4]);
          const float v[8] = {v0.x, v0.y, v0.z, v0.w,
                              v1.x, v1.y, v1.z, v1.w};
          const int4 s = sk[m][ch][p];
          const unsigned su[4] = {(unsigned)s.x, (unsigned)s.y,
                                  (unsigned)s.z, (unsigned)s.w};
          bf16x8 o;
          #pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[2 * j] = (__bf16)(v[2 * j] +
                                bf16_bits_to_float(su[j] & 0xffffu));
            o[2 * j + 1] = (__bf16)(v[2 * j + 1] +
                                    bf16_bits_to_float(su[j] >> 16));
          }
          const long row = row0 + m * 16 + rin;
          if (row < R)
            *reinterpret_cast<bf16x8*>(dx + row * Cin + col0 + ch * 64 +
                                       ec) = o;
        }
        wave_lds_sync();
      }
  }
}

struct C1Config {
  int bn, mt;
};

// The instantiation for a channel pair; bn == 0: unsupported.
C1Config c1_config(long cout, long cin) {
  if (cin != 64 && cin != 256 && cin != 512 && cin != 1024 && cin != 2048)
    return {0, 0};
  switch (cout) {
    case 64: return cin % 256 == 0 ? C1Config{256, 1} : C1Config{64, 4};
    case 128: return cin % 128 == 0 ? C1Config{128, 2} : C1Config{64, 4};
    case 256: return {64, 4};
    case 512: return {64, 4};
    default: return {0, 0};
  }
}

template <int COUT, int BN, int MT>
void c1_launch(const torch::Tensor& dy, const torch::Tensor& w,
               const c10::optional<torch::Tensor>& skip, torch::Tensor& dx,
               long R, int Cin) {
  constexpr long BM = kC1Waves * 16 * MT;
  constexpr long lds = (long)BN * (COUT + kWPad) * 2 +
                       (long)kC1Waves * kScFloats * 4;
  static_assert(lds <= 160 * 1024, "LDS budget");
  const long n_row_tiles = (R + BM - 1) / BM;
  const int nct = Cin / BN;
  const long cus =
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long per_cu = std::min<long>(4, 160 * 1024 / lds);
  // row lanes: a multiple of the XCD count, no more than there are row
  // tiles, and about per_cu workgroups per CU over all column tiles
  const long want = std::max<long>(kXcds,
                                   cus * per_cu / nct / kXcds * kXcds);
  const long most = (n_row_tiles + kXcds - 1) / kXcds * kXcds;
  const long nrl = std::min(want, most);
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(
      (conv1x1_bwd_data_kernel<COUT, BN, MT>), dim3(nrl * nct),
      dim3(kC1Threads), 0, stream,
      reinterpret_cast<const unsigned short*>(dy.data_ptr()),
      reinterpret_cast<const unsigned short*>(w.data_ptr()),
      skip.has_value()
          ? reinterpret_cast<const unsigned short*>(skip->data_ptr())
          : nullptr,
      reinterpret_cast<unsigned short*>(dx.data_ptr()), R, Cin,
      n_row_tiles);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "conv1x1_bwd_data: ",
              hipGetErrorString(e));
}

}  // namespace

bool conv1x1_bwd_data_supported(long cout, long cin) {
  return c1_config(cout, cin).bn != 0;
}

// rows per workgroup tile for a channel pair (0: unsupported)
long conv1x1_bwd_data_row_tile(long cout, long cin) {
  return (long)kC1Waves * 16 * c1_config(cout, cin).mt;
}

torch::Tensor conv1x1_bwd_data(torch::Tensor dy, torch::Tensor w,
                               c10::optional<torch::Tensor> skip) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 &&
              dy.scalar_type() == at::kBFloat16 &&
              dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv1x1_bwd_data: dy must be a channels_last bf16 GPU "
              "tensor [N, Cout, H, W]");
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.size(2) == 1 &&
              w.size(3) == 1 && w.scalar_type() == at::kBFloat16 &&
              w.is_contiguous() && w.size(0) == dy.size(1) &&
              w.device() == dy.device(),
              "conv1x1_bwd_data: w must be a contiguous bf16 "
              "[Cout, Cin, 1, 1] on dy's device");
  const long cout = w.size(0), cin = w.size(1);
  const C1Config cfg = c1_config(cout, cin);
  TORCH_CHECK(cfg.bn != 0, "conv1x1_bwd_data: unsupported channels Cout=",
              cout, " Cin=", cin);
  const long N = dy.size(0), H = dy.size(2), W = dy.size(3);
  if (skip.has_value())
    TORCH_CHECK(skip->is_cuda() && skip->device() == dy.device() &&
                skip->scalar_type() == at::kBFloat16 && skip->dim() == 4 &&
                skip->size(0) == N && skip->size(1) == cin &&
                skip->size(2) == H && skip->size(3) == W &&
                skip->is_contiguous(at::MemoryFormat::ChannelsLast),
                "conv1x1_bwd_data: skip must be a channels_last bf16 "
                "[N, Cin, H, W] on dy's device");
  auto dx = torch::empty(
      {N, cin, H, W},
      dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  const long R = N * H * W;
  if (R == 0) return dx;

#define C1_CASE(COUT, BN, MT)                                   \
  if (cout == COUT && cfg.bn == BN && cfg.mt == MT) {           \
    c1_launch<COUT, BN, MT>(dy, w, skip, dx, R, (int)cin);      \
    return dx;                                                  \
  }
  C1_CASE(64, 256, 1)
  C1_CASE(64, 64, 4)
  C1_CASE(128, 128, 2)
  C1_CASE(128, 64, 4)
  C1_CASE(256, 64, 4)
  C1_CASE(512, 64, 4)
#undef C1_CASE
  TORCH_CHECK(false, "conv1x1_bwd_data: no kernel for Cout=", cout,
              " Cin=", cin);
  return dx;
}
