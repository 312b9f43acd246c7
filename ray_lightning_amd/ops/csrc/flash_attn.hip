// Flash attention (causal, hs=64, bf16) — hand-written CDNA4 MFMA
// kernels, the "v3" design (the r01 32-rows-per-wave kernels lost to it
// 2.7x and live in git history; profiles/r02_flash_v3.md has the
// measurements).
//
// Kernels: flash_fwd_v3_kernel, flash_bwd_pre_kernel (D = rowsum(dO o
// O)), flash_bwd_dkv_v3_kernel, flash_bwd_dq_v3_kernel. Each of the
// three v3 kernels is instantiated for DROPOUT false (p = 0, the
// default training path) and true (Philox mask on the probabilities),
// and for USE_PERMLANE true (what training runs) and false (the
// ds_bpermute redistribution, RLA_FLASH_SHFL=1, debug), and for DOCS
// false (causal over the whole row) and true (packed rows: causal
// within each document, tiles wholly in another document skipped; see
// "document masking" below).
// All three share one structure: a workgroup owns 64 rows (4 waves x
// 16), walks the other axis in tiles of 64 staged through
// double-buffered XOR-swizzled LDS images (issue-early / write-late),
// computes the TRANSPOSED score tile with 16x16x32 MFMAs so that the
// softmax axis is lane-local, and turns the C-layout result into the
// next MFMA's B-fragment in registers (permlane32/16 swaps) instead of
// through LDS. Tiles above the causal diagonal are skipped per wave.
//
// Host side (after the kernels): one set of operand checks, one forward
// and one backward launcher, and the eight exported entry points
// flash_attn_{fwd,bwd}_v3[_docs][_dropout] that ops/flash_attn.py calls.
//
// Last in the file: flash_fwd_v4_kernel / flash_attn_fwd_v4, the
// 32x32x16 forward experiment (slower than v3, forward only, not wired
// into ops/flash_attn.py).
//
// Layout: q, k, v are [B, H, T, 64] bf16 contiguous, T % 64 == 0.
// Causal only.
// Fragment maps verified by mfma_probe (tests/test_flash_attn_gpu.py):
//   A[16Mx32K]: lane l elem i -> row l&15,  k (l>>4)*8+i
//   B[32Kx16N]: lane l elem i -> col l&15,  k (l>>4)*8+i
//   C  [16x16]: lane l reg  r -> row (l>>4)*4+r, col l&15
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <ATen/hip/HIPGraphsUtils.cuh>

#include "philox_dropout.h"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int HS = 64;      // head size (fixed)
constexpr int BN = 64;      // key/value rows per tile
constexpr float kNegInf = -1e30f;

// Raw v_exp_f32 (2^x): libm exp2f carries ~5 range-guard instructions
// per call (ldexp/cmp/cndmask) — the fwd softmax issues 17 of them per
// tile and the guards are dead weight here (inputs are <= 8 by the
// defer-max bound and masked entries sit at ~-1.8e29, which the raw
// instruction correctly underflows to 0).
__device__ __forceinline__ float fast_exp2(float x) {
  return __builtin_amdgcn_exp2f(x);
}

__device__ __forceinline__ void wait_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// 16 bytes per lane from a [rows, HS] row-major bf16 tile:
// row = base_row + (l&15), k = kk*32 + (l>>4)*8 .. +8
__device__ __forceinline__ bf16x8 load_frag_rowmajor(
    const __hip_bfloat16* __restrict__ p, int base_row, int kk,
    int lane, long row_stride) {
  const long row = base_row + (lane & 15);
  const long off = row * row_stride + kk * 32 + (lane >> 4) * 8;
  bf16x8 v;
  *reinterpret_cast<int4*>(&v) =
      *reinterpret_cast<const int4*>(p + off);
  return v;
}

// --- XOR-swizzled transpose image (v3) --------------------------------
// Image: img[d][kv] bf16, row = 128 B. Bank index depends on byte%256
// (two rows), so consecutive d alternate half-banks; the granule sel
// (((d>>1)^(d>>3))&7) spreads the 8 same-parity rows of a 16-row
// fragment read over all 8 granules -> conflict-free ds_read_b128,
// and distinct granules for the d / d+8 write groups.
__device__ __forceinline__ int swz_off(int d, int byte_in_row) {
  // sel = (d>>1)*3 ^ (d>>3): within any 4 consecutive rows (one
  // ds_read_b64_tr_b16 block) the same-parity pair differs by XOR 3
  // -> granule sets disjoint (the previous (d>>1)^(d>>3) left rows
  // d/d+2 sharing a granule pair: 2-way tr conflicts); 3 is coprime
  // to 8 so 8 consecutive same-parity rows still spread over all 8
  // granules for the b128 fragment reads, and the d vs d+32 staging
  // groups still split via the (d>>3) term.
  return d * (2 * BN) +
         (byte_in_row ^ (((((d >> 1) * 3) ^ (d >> 3)) & 7) << 4));
}

// Split staging (T14 issue-early/write-late): load the next tile's
// piece into registers at the top of the current tile's compute, write
// it to the other LDS buffer after the compute — HBM latency hides
// under the MFMA/softmax phase instead of sitting in front of the
// barrier.
struct StageRegsR {   // row-major staging piece (rows r, r+32)
  bf16x8 r0, r1;
};

__device__ __forceinline__ StageRegsR stage_r_load(
    const __hip_bfloat16* src, int row0) {
  const int r = threadIdx.x >> 3;
  const int c0 = (threadIdx.x & 7) * 8;
  StageRegsR t;
  *reinterpret_cast<int4*>(&t.r0) = *reinterpret_cast<const int4*>(
      src + (long)(row0 + r) * HS + c0);
  *reinterpret_cast<int4*>(&t.r1) = *reinterpret_cast<const int4*>(
      src + (long)(row0 + r + 32) * HS + c0);
  return t;
}

// Row-major swizzled image (for A-fragment reads via read_frag_swz):
// img[row][hs], b128 writes land in one granule each.
__device__ __forceinline__ void stage_r_write(__bf16* dst,
                                              const StageRegsR& t) {
  const int r = threadIdx.x >> 3;
  const int c0 = (threadIdx.x & 7) * 8;
  char* base = reinterpret_cast<char*>(dst);
  *reinterpret_cast<int4*>(base + swz_off(r, c0 * 2)) =
      *reinterpret_cast<const int4*>(&t.r0);
  *reinterpret_cast<int4*>(base + swz_off(r + 32, c0 * 2)) =
      *reinterpret_cast<const int4*>(&t.r1);
}

// b128 fragment read from the swizzled image: row = row16 + (lane&15),
// bytes [16*(4c+... ) fixed 16-byte granule at (32c+8g)*2.
__device__ __forceinline__ bf16x8 read_frag_swz(const __bf16* img,
                                                int row16, int c,
                                                int lane) {
  const int d = row16 + (lane & 15);
  const int g = lane >> 4;
  bf16x8 v;
  *reinterpret_cast<int4*>(&v) = *reinterpret_cast<const int4*>(
      reinterpret_cast<const char*>(img) + swz_off(d, 64 * c + 16 * g));
  return v;
}

// Transposed A-fragment straight from the swizzled ROW-major image via
// ds_read_b64_tr_b16 (guide T10; semantics verified by tr16_probe:
// per 16-lane group the 16 8-byte segments form a [4 src-rows][16 col]
// block — rows = lanes 4r..4r+3 — and lane j receives column j).
// Fragment: row = col16 + (lane&15), k elems i = source rows
// krow0 + 8*(lane>>4) + i. Rows are swizzle-independent (each lane
// addresses its own 8 B segment inside one granule). The readers below
// batch several such fragments in front of a single lgkm drain.
//
// Paired variant for the fwd PV loop: BOTH kv chunks' transposed
// fragments of one 16-col block from one image, single lgkm drain
// (separate absolute row bases keep the swizzle sel correct).
__device__ __forceinline__ void read_frag_tr_2row(const __bf16* img,
                                                  int krow0a,
                                                  int krow0b, int col16,
                                                  int lane, bf16x8& va,
                                                  bf16x8& vb) {
  const int j = lane & 15;
  const int g = lane >> 4;
  const unsigned base =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)img;
  const int cb = (col16 + 4 * (j & 3)) * 2;
  const int ra = krow0a + 8 * g + (j >> 2);
  const int rb = krow0b + 8 * g + (j >> 2);
  const unsigned a0 = base + (unsigned)swz_off(ra, cb);
  const unsigned a1 = base + (unsigned)swz_off(ra + 4, cb);
  const unsigned b0 = base + (unsigned)swz_off(rb, cb);
  const unsigned b1 = base + (unsigned)swz_off(rb + 4, cb);
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  uint2v ra0, ra1, rb0, rb1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n"
      "ds_read_b64_tr_b16 %1, %5\n"
      "ds_read_b64_tr_b16 %2, %6\n"
      "ds_read_b64_tr_b16 %3, %7\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(ra0), "=&v"(ra1), "=&v"(rb0), "=&v"(rb1)
      : "v"(a0), "v"(a1), "v"(b0), "v"(b1)
      : "memory");
  unsigned* wa = reinterpret_cast<unsigned*>(&va);
  wa[0] = ra0[0]; wa[1] = ra0[1]; wa[2] = ra1[0]; wa[3] = ra1[1];
  unsigned* wb = reinterpret_cast<unsigned*>(&vb);
  wb[0] = rb0[0]; wb[1] = rb0[1]; wb[2] = rb1[0]; wb[3] = rb1[1];
}

// =====================================================================
// forward v3 — swapped-operand S^T design (profiles/r01_flash_attn_notes
// round-2 plan; guide T12 structure adapted to the verified 16x16x32
// fragment maps):
//   S^T = mfma(K, Q^T): C gives each lane 16 kv entries of ONE q column
//   -> softmax over kv is lane-local + 2 cross-lane combines (vs 64
//   shfl per tile in the r01 design), and P^T feeds the PV B-operand
//   after an in-register redistribution (no P LDS round-trip, no extra
//   barrier).
// Per workgroup: 64 q rows, 4 waves x 16 q columns; KV tiles of 64.
// =====================================================================
constexpr int WQ = 16;     // q columns per wave
constexpr int BM3 = 64;    // q rows per workgroup

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  union { unsigned u; __bf16 h[2]; } t;
  t.h[0] = (__bf16)lo;
  t.h[1] = (__bf16)hi;
  return t.u;   // compiler emits v_cvt_pk_bf16_f32
}

// Redistribute the P^T C-layout (lane holds q = lane&15; kv =
// 16*sub + 4*(lane>>4) + r) into the PV B-fragment layout (lane needs
// 8 consecutive kv of its q column: kv = 32*blk + 8*(lane>>4) + i).
// X_j / Y_j are the packed dwords of kv-subtiles 2*blk / 2*blk+1
// (j = dword within the 4-run). Exchange is across the lane>>4 group
// bits only (fixed per-register partner — the property that broke the
// naive bpermute scheme, see r01 notes).
//
// Derivation (target group g needs source pack of group 2g mod 4,
// register X for g<2 / Y for g>=2, dwords j then j of group 2g+1):
//   D1 = {g0:X@g0, g1:X@g2, g2:Y@g0, g3:Y@g2}  -> B-frag dwords j
//   D2 = {g0:X@g1, g1:X@g3, g2:Y@g1, g3:Y@g3}  -> B-frag dwords 2+j
template <bool USE_PERMLANE>
__device__ __forceinline__ void redist_pair(unsigned xj, unsigned yj,
                                            int lane, unsigned& d1,
                                            unsigned& d2) {
  if (USE_PERMLANE) {
    // (P,S) = pl32swap(X,Y): P = {g01: X own, g23: Y of g-2};
    //                        S = {g01: X of g+2, g23: Y own}
    // (D1,D2) = pl16swap(P,S): D1 = even 16-rows interleave, D2 = odd
    auto ps = __builtin_amdgcn_permlane32_swap(xj, yj, false, false);
    auto dd = __builtin_amdgcn_permlane16_swap(ps[0], ps[1], false,
                                               false);
    d1 = dd[0];
    d2 = dd[1];
  } else {
    // ds_bpermute fallback (known-correct semantics): source lane =
    // same q, group 2*(g&1) [+1 for d2]; register by target bit5.
    const int src = (lane & 15) | ((lane & 16) << 1);
    const unsigned x1 = __shfl(xj, src, 64);
    const unsigned y1 = __shfl(yj, src, 64);
    const unsigned x2 = __shfl(xj, src + 16, 64);
    const unsigned y2 = __shfl(yj, src + 16, 64);
    d1 = (lane & 32) ? y1 : x1;
    d2 = (lane & 32) ? y2 : x2;
  }
}

// --- attention dropout (DROPOUT instantiations of the v3 kernels) -----
// The mask is the fused-LN convention (philox_dropout.h) applied to the
// [B, H, T, T] probability matrix: flat i = ((bh*T + q)*T + kv), one
// Philox call per aligned group of four kv of one q row (T % 64 == 0,
// so a group never straddles rows). Group index of (row q, kv group
// kv4 = kv >> 2) is (bh*T + q) * (T/4) + kv4, in 64 bits: B*H*T*T
// passes 2^32 at shapes in use. The kernels only differ in which lane
// makes which call; the mask is a function of (seed, offset, i) alone.
__device__ __forceinline__ uint64_t drop_row_group(int bh, int T,
                                                   int row) {
  return ((uint64_t)bh * (uint64_t)T + (uint64_t)row) *
         (uint64_t)(T >> 2);
}

__device__ __forceinline__ uint4 drop_words(const DropArgs& d,
                                            uint64_t grp) {
  return philox4x32_10(
      d.k0, d.k1,
      make_uint4(d.o0, d.o1, (uint32_t)grp, (uint32_t)(grp >> 32)));
}

// keep nibble of one call: bit w = word w kept
__device__ __forceinline__ unsigned drop_nibble(const DropArgs& d,
                                                uint64_t grp) {
  const uint4 w = drop_words(d, grp);
  return (unsigned)(w.x >= d.thr) | ((unsigned)(w.y >= d.thr) << 1) |
         ((unsigned)(w.z >= d.thr) << 2) | ((unsigned)(w.w >= d.thr) << 3);
}

// --- document masking (DOCS instantiations of the v3 kernels) ---------
// A packed row holds several documents; q may attend kv iff
// doc_start[b, q] <= kv <= q (doc_end[b, kv] is the mirror image the dkv
// kernel needs). The kernels get one per-position int32 bound [B, T]
// and H (b = bh / H). A bound is only ever (1) compared with a position
// and (2) turned into the first / last TILE of a workgroup's loop after
// a clamp into the range the causal loop already walks, so no value in
// it, however wrong, moves an address outside the operands: wrong
// bounds give wrong numbers, never a stray access. Wave-uniform bounds
// go through readfirstlane so that they live in SGPRs.
__device__ __forceinline__ int uniform_bound(const int* bnd, int pos) {
  return __builtin_amdgcn_readfirstlane(bnd[pos]);
}

template <bool USE_PERMLANE, bool DROPOUT = false, bool DOCS = false>
// min 4 waves/EU: keeps the allocator at <=128 regs so occupancy stays
// at the LDS-allowed 4 waves/SIMD (131 regs would drop it to 3). The
// DOCS instantiations fit too (121-128 VGPRs, no scratch;
// profiles/flash_attn_docs.md).
__global__ __launch_bounds__(256, 4) void flash_fwd_v3_kernel(
    const __hip_bfloat16* __restrict__ Q,
    const __hip_bfloat16* __restrict__ K,
    const __hip_bfloat16* __restrict__ V,
    __hip_bfloat16* __restrict__ O, float* __restrict__ LSE,
    int T, float scale, DropArgs drop,
    const int* __restrict__ doc_start, int H) {
  const int bh = blockIdx.y;
  const int qm0 = blockIdx.x * BM3;
  if (qm0 >= T) return;
  const long base = (long)bh * T * HS;
  const __hip_bfloat16* q = Q + base;
  const __hip_bfloat16* k = K + base;
  const __hip_bfloat16* v = V + base;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = qm0 + wave * WQ;      // wave's first (of 16) q column
  const int myq = q0 + (lane & 15);    // this lane's q column
  const int g = lane >> 4;             // kv group 0..3

  __shared__ __bf16 lds_v[2][BN * HS];    // V row-major db buffer, 16 KB
  __shared__ __bf16 lds_k[2][BN * HS];    // K row-major db buffer, 16 KB
  __shared__ __bf16 lds_o[4][WQ * HS];    // epilogue transpose, 8 KB

  // Q^T B-fragments (col = q = lane&15, k = hs): straight row-major
  // 16-byte loads from Q (same bytes as an A-fragment of row q).
  bf16x8 qf[2];
  #pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    qf[kk] = load_frag_rowmajor(q, q0, kk, lane, HS);

  float m_i = kNegInf, l_i = 0.f;
  f32x4 o_acc[4];   // O^T: row d = 16*n + 4*g + r, col q (lane&15)
  #pragma unroll
  for (int n = 0; n < 4; ++n)
    o_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float l2e = 1.4426950408889634f * scale;
  const int kv_end = (qm0 + BM3 < T) ? qm0 + BM3 : T;
  // DOCS: this lane's doc_start, the wave's smallest and largest (starts
  // do not decrease with q), and the first tile of the workgroup's loop:
  // the one that holds doc_start[qm0], clamped into [0, qm0]
  int mystart = 0, wstart_lo = 0, wstart_hi = 0, kv_begin = 0;
  if constexpr (DOCS) {
    const int* ds = doc_start + (long)(bh / H) * T;
    mystart = ds[myq];
    wstart_lo = uniform_bound(ds, q0);
    wstart_hi = uniform_bound(ds, q0 + WQ - 1);
    const int s0 = uniform_bound(ds, qm0);
    kv_begin = (s0 < 0 ? 0 : (s0 > qm0 ? qm0 : s0)) & ~(BN - 1);
  }
  // prologue: the first tile staged through registers, then the loop
  // keeps one tile in flight (issue loads -> compute current -> write
  // other buf)
  {
    StageRegsR vt = stage_r_load(v, kv_begin);
    StageRegsR kt = stage_r_load(k, kv_begin);
    stage_r_write(lds_v[0], vt);
    stage_r_write(lds_k[0], kt);
  }
  __syncthreads();
  int buf = 0;
  for (int kn0 = kv_begin; kn0 < kv_end; kn0 += BN, buf ^= 1) {
    const int next = (kn0 + BN < kv_end) ? kn0 + BN : kn0;
    StageRegsR vt = stage_r_load(v, next);
    StageRegsR kt = stage_r_load(k, next);
    // DOCS: a tile that ends before the wave's smallest start is dead
    // work for the whole wave, like one above the diagonal
    const bool active = kn0 <= q0 + WQ - 1 &&
                        (!DOCS || kn0 + BN - 1 >= wstart_lo);
    if (active) {
      // --- S^T = K Q^T: lane gets kv = kn0+16*sub+4*g+r of column myq
      // (T5: favor the MFMA-entering wave over waves in their
      // memory/softmax phases)
      // dropout: the tile's 16 keep bits (bit 4*sub + r) first, while
      // only the loop-carried state is live: the generator's registers
      // are dead again before S^T and the softmax need theirs, which
      // keeps these instantiations at 4 waves without scratch (drawn
      // next to the softmax they need 135 VGPRs). This lane's four r
      // of one sub are one aligned kv group of row myq: one lane-local
      // call per sub. Group index = wave-uniform 64-bit part + 32-bit
      // lane part.
      unsigned keep = 0;
      if constexpr (DROPOUT) {
        const uint64_t grp0 =
            drop_row_group(bh, T, q0) + (uint64_t)(kn0 >> 2) +
            (uint64_t)((unsigned)(lane & 15) * (unsigned)(T >> 2) +
                       (unsigned)g);
        #pragma unroll
        for (int sub = 0; sub < 4; ++sub)
          keep |= drop_nibble(drop, grp0 + 4 * sub) << (4 * sub);
        __builtin_amdgcn_sched_barrier(0);
      }
      f32x4 st[4];
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        bf16x8 kf0 = read_frag_swz(lds_k[buf], 16 * sub, 0, lane);
        bf16x8 kf1 = read_frag_swz(lds_k[buf], 16 * sub, 1, lane);
        st[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf0, qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        st[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf1, qf[1], st[sub], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
      // --- causal mask (only tiles overlapping the diagonal) ---------
      if constexpr (DOCS) {
        // ... or holding a kv before the start of one of the wave's q
        if (kn0 + BN - 1 > q0 || kn0 < wstart_hi) {
          #pragma unroll
          for (int sub = 0; sub < 4; ++sub)
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int kv = kn0 + 16 * sub + 4 * g + r;
              if (kv > myq || kv < mystart) st[sub][r] = kNegInf;
            }
        }
      } else if (kn0 + BN - 1 > q0) {
        #pragma unroll
        for (int sub = 0; sub < 4; ++sub)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kn0 + 16 * sub + 4 * g + r > myq)
              st[sub][r] = kNegInf;
      }
      // --- online softmax: lane-local over 16 kv + 2 combines --------
      float mx = kNegInf;
      #pragma unroll
      for (int sub = 0; sub < 4; ++sub)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          mx = fmaxf(mx, st[sub][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // T13 defer-max: if no lane's max grew by more than 8 exponent
      // units, keep the old running max and skip the O rescale —
      // P is then bounded by 2^8, which the f32 accumulators absorb.
      // Decision covers THIS tile's P before it is exponentiated
      // (textbook-safe order); first tile never defers (m_i = -1e30).
      const bool defer = __all((mx - m_i) * l2e <= 8.0f);
      float m_new, corr;
      if (defer) {
        m_new = m_i;
        corr = 1.0f;
      } else {
        m_new = fmaxf(m_i, mx);
        corr = fast_exp2((m_i - m_new) * l2e);
        #pragma unroll
        for (int n = 0; n < 4; ++n)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            o_acc[n][r] *= corr;
      }
      float rowsum = 0.f;
      #pragma unroll
      for (int sub = 0; sub < 4; ++sub)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          // masked entries are kNegInf: the raw exp2 underflows the
          // ~-1.8e29 exponent to exactly 0 — no guard needed (without
          // DOCS every lane's FIRST tile contains kv<=q, so m_new is
          // finite; with DOCS see `dead` below)
          const float p = fast_exp2((st[sub][r] - m_new) * l2e);
          st[sub][r] = p;
          rowsum += p;
        }
      rowsum += __shfl_xor(rowsum, 16, 64);
      rowsum += __shfl_xor(rowsum, 32, 64);
      // DOCS: a lane whose whole tile lies before its doc_start (`dead`;
      // T=128, documents [0,70) [70,128): rows 70..79 on tile 0, which
      // their wave walks for rows 64..69) has mx = m_i = kNegInf, so
      // m_new = kNegInf whether the wave defers or not, every p above is
      // exp2(0) = 1 and the PV below adds 64 rows of V to its o_acc.
      // The lane is put back to its initial state instead: rowsum 0
      // here (corr is 1, so l_i stays 0; m_i stays kNegInf) and o_acc
      // zeroed by a SELECT after the PV, which also holds when those V
      // rows are Inf/NaN, where the rescale by exp2(kNegInf - m) = 0 of
      // the lane's first live tile would not. The T13 vote cannot keep
      // the bad maximum: the dead lane's vote is (kNegInf - kNegInf)
      // * l2e = 0 <= 8, so it never blocks a deferral of the others,
      // and on its first live tile (mx - kNegInf) * l2e is ~1e29 > 8,
      // so the wave does not defer and m_new becomes the finite mx. Its
      // p = 1 columns stay out of every other lane's result: an MFMA
      // column depends on that column of B alone.
      bool dead = false;
      if constexpr (DOCS) {
        dead = kn0 + BN - 1 < mystart;
        rowsum = dead ? 0.f : rowsum;
      }
      l_i = l_i * corr + rowsum;
      m_i = m_new;
      if constexpr (DROPOUT) {
        // m, l (and LSE) are those of the undropped P; the mask goes
        // on P alone
        #pragma unroll
        for (int sub = 0; sub < 4; ++sub)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            st[sub][r] =
                ((keep >> (4 * sub + r)) & 1u) ? st[sub][r] : 0.f;
      }
      // --- P^T -> PV B-fragments, in registers -----------------------
      bf16x8 pb[2];
      #pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        const unsigned x0 = pack_bf16(st[2 * blk][0], st[2 * blk][1]);
        const unsigned x1 = pack_bf16(st[2 * blk][2], st[2 * blk][3]);
        const unsigned y0 = pack_bf16(st[2 * blk + 1][0],
                                      st[2 * blk + 1][1]);
        const unsigned y1 = pack_bf16(st[2 * blk + 1][2],
                                      st[2 * blk + 1][3]);
        unsigned d0, d2, d1, d3;
        redist_pair<USE_PERMLANE>(x0, y0, lane, d0, d2);
        redist_pair<USE_PERMLANE>(x1, y1, lane, d1, d3);
        unsigned* pw = reinterpret_cast<unsigned*>(&pb[blk]);
        pw[0] = d0; pw[1] = d1; pw[2] = d2; pw[3] = d3;
      }
      // --- O^T += V^T P^T: both kv chunks' V^T fragments per
      // d-block with one drain
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int n = 0; n < 4; ++n) {
        bf16x8 va0, va1;
        read_frag_tr_2row(lds_v[buf], 0, 32, 16 * n, lane, va0, va1);
        o_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            va0, pb[0], o_acc[n], 0, 0, 0);
        o_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            va1, pb[1], o_acc[n], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
      if constexpr (DOCS) {
        // dead lanes back to zero (above); only tiles that have one
        if (kn0 + BN - 1 < wstart_hi) {
          #pragma unroll
          for (int n = 0; n < 4; ++n)
            #pragma unroll
            for (int r = 0; r < 4; ++r)
              o_acc[n][r] = dead ? 0.f : o_acc[n][r];
        }
      }
    }
    // write-late: next tile's regs -> the other buffers, one barrier
    stage_r_write(lds_v[buf ^ 1], vt);
    stage_r_write(lds_k[buf ^ 1], kt);
    __syncthreads();
  }

  // --- epilogue: transpose O^T -> O rows through LDS ------------------
  float inv_l = (l_i > 0.f) ? 1.f / l_i : 0.f;
  if constexpr (DROPOUT) inv_l *= drop.scale;   // 1/(1-p) on kept P
  __bf16* ow = lds_o[wave];
  #pragma unroll
  for (int n = 0; n < 4; ++n)
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      ow[(lane & 15) * HS + 16 * n + 4 * g + r] =
          (__bf16)(o_acc[n][r] * inv_l);
  wait_lds();
  // 64 lanes x 2 b128: row = lane>>2 (16 rows), 16 bf16 per read
  {
    const int row = lane >> 2;           // wave-local q row 0..15
    const int c0 = (lane & 3) * 16;
    int4 t0 = *reinterpret_cast<const int4*>(ow + row * HS + c0);
    int4 t1 = *reinterpret_cast<const int4*>(ow + row * HS + c0 + 8);
    *reinterpret_cast<int4*>(O + base + (long)(q0 + row) * HS + c0) = t0;
    *reinterpret_cast<int4*>(
        O + base + (long)(q0 + row) * HS + c0 + 8) = t1;
  }
  if (g == 0)
    LSE[(long)bh * T + myq] =
        m_i * scale + logf(fmaxf(l_i, 1e-30f));
}

// =====================================================================
// backward v3 — same swapped-C-layout + in-register redistribution
// structure as fwd v3 (no P^T/dS^T LDS round-trips, no per-element
// softmax shuffles; lse/D land lane-resident where the layout allows).
// =====================================================================

// D = rowsum(dO * O), fp32 (shared by the DROPOUT instantiations: O
// already carries the mask)
__global__ __launch_bounds__(256) void flash_bwd_pre_kernel(
    const __hip_bfloat16* __restrict__ dO,
    const __hip_bfloat16* __restrict__ O, float* __restrict__ D,
    long total_rows) {
  const long row = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (row >= total_rows) return;
  const int c0 = (threadIdx.x & 3) * 16;
  float s = 0.f;
  #pragma unroll
  for (int c = 0; c < 16; c += 8) {
    bf16x8 a, b;
    *reinterpret_cast<int4*>(&a) = *reinterpret_cast<const int4*>(
        dO + row * HS + c0 + c);
    *reinterpret_cast<int4*>(&b) = *reinterpret_cast<const int4*>(
        O + row * HS + c0 + c);
    #pragma unroll
    for (int i = 0; i < 8; ++i)
      s += (float)a[i] * (float)b[i];
  }
  #pragma unroll
  for (int w = 1; w <= 2; w <<= 1)
    s += __shfl_xor(s, w, 64);
  if ((threadIdx.x & 3) == 0) D[row] = s;
}

// Batched variant for dkv: TWO 16-row blocks' transposed fragments
// from two images with ONE lgkm drain (half the drains of per-n
// reads; the full 4-block batch costs ~195 regs -> 2 waves/SIMD,
// worse than the LDS-capped 3).
__device__ __forceinline__ void read_frag_tr2x2(
    const __bf16* imgA, const __bf16* imgB, int krow0, int n0,
    int lane, bf16x8 (&va)[2], bf16x8 (&vb)[2]) {
  const int j = lane & 15;
  const int g = lane >> 4;
  const unsigned baseA =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)imgA;
  const unsigned baseB =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)imgB;
  const int r0 = krow0 + 8 * g + (j >> 2);
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  uint2v a[4], b[4];
  unsigned addrA[4], addrB[4];
  #pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int cb = (16 * (n0 + n) + 4 * (j & 3)) * 2;
    addrA[2 * n] = baseA + (unsigned)swz_off(r0, cb);
    addrA[2 * n + 1] = baseA + (unsigned)swz_off(r0 + 4, cb);
    addrB[2 * n] = baseB + (unsigned)swz_off(r0, cb);
    addrB[2 * n + 1] = baseB + (unsigned)swz_off(r0 + 4, cb);
  }
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n"
      "ds_read_b64_tr_b16 %1, %9\n"
      "ds_read_b64_tr_b16 %2, %10\n"
      "ds_read_b64_tr_b16 %3, %11\n"
      "ds_read_b64_tr_b16 %4, %12\n"
      "ds_read_b64_tr_b16 %5, %13\n"
      "ds_read_b64_tr_b16 %6, %14\n"
      "ds_read_b64_tr_b16 %7, %15\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]),
        "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
      : "v"(addrA[0]), "v"(addrA[1]), "v"(addrA[2]), "v"(addrA[3]),
        "v"(addrB[0]), "v"(addrB[1]), "v"(addrB[2]), "v"(addrB[3])
      : "memory");
  #pragma unroll
  for (int n = 0; n < 2; ++n) {
    unsigned* wa = reinterpret_cast<unsigned*>(&va[n]);
    wa[0] = a[2 * n][0]; wa[1] = a[2 * n][1];
    wa[2] = a[2 * n + 1][0]; wa[3] = a[2 * n + 1][1];
    unsigned* wb = reinterpret_cast<unsigned*>(&vb[n]);
    wb[0] = b[2 * n][0]; wb[1] = b[2 * n][1];
    wb[2] = b[2 * n + 1][0]; wb[3] = b[2 * n + 1][1];
  }
}

// Value of lane (lane ^ X) of the same quad, X = 1 or 2. DPP quad_perm
// ([1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E) in the permlane build,
// ds_bpermute (__shfl_xor) in the bpermute build; same result.
template <bool USE_PERMLANE, int X>
__device__ __forceinline__ unsigned quad_xchg(unsigned v) {
  static_assert(X == 1 || X == 2, "quad_xchg: X is 1 or 2");
  if (USE_PERMLANE)
    return (unsigned)__builtin_amdgcn_update_dpp(
        0, (int)v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, true);
  return (unsigned)__shfl_xor((int)v, X, 64);
}

// dK/dV v3: workgroup = 64 KV rows, 4 waves x 16 kv columns; iterate
// q tiles of 64. C layouts put kv in lane&15 throughout:
//   S[q][kv]   = mfma(Q_frag,  K^T B-frag)   (both direct row-major)
//   dP[q][kv]  = mfma(dO_frag, V^T B-frag)
//   dV^T[d][kv]= mfma(dO^T A-frag(lds), redist(P) B-frag)
//   dK^T[d][kv]= mfma(Q^T  A-frag(lds), redist(dS) B-frag)
template <bool USE_PERMLANE, bool DROPOUT = false, bool DOCS = false>
// min 3 waves/EU (the LDS cap): the pair-batched tr reads push regs to
// ~172 which rounds to 2 waves without the bound. Postmortem rule:
// verified ScratchSize stays 0 under this bound (spills + hand asm
// were the r02 nondeterminism bug). DROPOUT spills at 170 (44-68
// bytes), so those instantiations take 2 waves; so does DOCS in the
// bpermute build (8 bytes at 3 waves; the permlane one fits in 168).
__global__ __launch_bounds__(
    256, (DROPOUT || (DOCS && !USE_PERMLANE)) ? 2 : 3)
void flash_bwd_dkv_v3_kernel(
    const __hip_bfloat16* __restrict__ Qg,
    const __hip_bfloat16* __restrict__ Kg,
    const __hip_bfloat16* __restrict__ Vg,
    const __hip_bfloat16* __restrict__ dOg,
    const float* __restrict__ LSE, const float* __restrict__ Dg,
    __hip_bfloat16* __restrict__ dK, __hip_bfloat16* __restrict__ dV,
    int T, float scale, DropArgs drop,
    const int* __restrict__ doc_end, int H) {
  const int bh = blockIdx.y;
  const int kb0 = blockIdx.x * BM3;      // 64 KV rows per workgroup
  if (kb0 >= T) return;
  const long base = (long)bh * T * HS;
  const __hip_bfloat16* q = Qg + base;
  const __hip_bfloat16* k = Kg + base;
  const __hip_bfloat16* v = Vg + base;
  const __hip_bfloat16* dO = dOg + base;
  const float* lse = LSE + (long)bh * T;
  const float* Drow = Dg + (long)bh * T;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int kv0 = kb0 + wave * WQ;       // wave's first kv column
  const int mykv = kv0 + (lane & 15);
  const int g = lane >> 4;

  __shared__ __bf16 lds_do[2][BN * HS];  // dO row-major db, 16 KB
  __shared__ __bf16 lds_q[2][BN * HS];   // Q  row-major db, 16 KB
  __shared__ float lds_lse[2][BN];
  __shared__ float lds_d[2][BN];
  __shared__ __bf16 lds_ep[4][WQ * HS];  // epilogue, 8 KB

  // K^T / V^T B-fragments (col = kv = lane&15): kernel-resident
  bf16x8 kf[2], vf[2];
  #pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    kf[kk] = load_frag_rowmajor(k, kv0, kk, lane, HS);
    vf[kk] = load_frag_rowmajor(v, kv0, kk, lane, HS);
  }

  f32x4 dv_acc[4], dk_acc[4];   // ^T: row d = 16n+4g+r, col kv
  #pragma unroll
  for (int n = 0; n < 4; ++n) {
    dv_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    dk_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const float l2e = 1.4426950408889634f;

  {  // prologue: first q tile through registers
    StageRegsR dt = stage_r_load(dO, kb0);
    StageRegsR qt = stage_r_load(q, kb0);
    stage_r_write(lds_do[0], dt);
    stage_r_write(lds_q[0], qt);
    if (threadIdx.x < BN) {
      lds_lse[0][threadIdx.x] = lse[kb0 + threadIdx.x];
      lds_d[0][threadIdx.x] = Drow[kb0 + threadIdx.x];
    }
  }
  __syncthreads();
  // DOCS: this lane's doc_end, the wave's largest (ends do not decrease
  // with kv), and the end of the workgroup's loop: after the tile that
  // holds doc_end[kb0 + 63], clamped into [kb0, T - 1]
  int myend = 0, wend_hi = 0, q_stop = T;
  if constexpr (DOCS) {
    const int* de = doc_end + (long)(bh / H) * T;
    myend = de[mykv];
    wend_hi = uniform_bound(de, kv0 + WQ - 1);
    const int e1 = uniform_bound(de, kb0 + BM3 - 1);
    q_stop = ((e1 < kb0 ? kb0 : (e1 > T - 1 ? T - 1 : e1)) & ~(BN - 1)) +
             BN;
  }
  int buf = 0;
  for (int qm0 = kb0; qm0 < q_stop; qm0 += BN, buf ^= 1) {
    const int next = (qm0 + BN < q_stop) ? qm0 + BN : qm0;
    StageRegsR dt = stage_r_load(dO, next);
    StageRegsR qt = stage_r_load(q, next);
    float nlse = 0.f, nd = 0.f;
    if (threadIdx.x < BN) {
      nlse = lse[next + threadIdx.x];
      nd = Drow[next + threadIdx.x];
    }
    // DOCS: a q tile that begins after the wave's largest end is dead
    // work for the whole wave
    const bool active = kv0 <= qm0 + BN - 1 && (!DOCS || qm0 <= wend_hi);
    if (active) {
      float pv[4][4], dsv[4][4];
      #pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        bf16x8 aq0 = read_frag_swz(lds_q[buf], 16 * sub, 0, lane);
        bf16x8 aq1 = read_frag_swz(lds_q[buf], 16 * sub, 1, lane);
        bf16x8 ad0 = read_frag_swz(lds_do[buf], 16 * sub, 0, lane);
        bf16x8 ad1 = read_frag_swz(lds_do[buf], 16 * sub, 1, lane);
        __builtin_amdgcn_s_setprio(1);
        f32x4 sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            aq0, kf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            aq1, kf[1], sacc, 0, 0, 0);
        f32x4 dpacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ad0, vf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ad1, vf[1], dpacc, 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        // lse/D for this lane's 4 consecutive q rows: one b128 each
        // instead of 8 scalar ds_read_b32 (the bwd census showed the
        // per-element reads + their waits dominating non-MFMA issue)
        const float4 lse4 = *reinterpret_cast<const float4*>(
            &lds_lse[buf][16 * sub + 4 * g]);
        const float4 d4 = *reinterpret_cast<const float4*>(
            &lds_d[buf][16 * sub + 4 * g]);
        const float lse_a[4] = {lse4.x, lse4.y, lse4.z, lse4.w};
        const float d_a[4] = {d4.x, d4.y, d4.z, d4.w};
        // dropout: bit 4r of keep16 = keep(q row r of this sub, mykv).
        // The layout is the forward's transposed: a lane holds ONE kv
        // and four consecutive q rows, and the four lanes of a quad
        // hold the four kv of one aligned group. Lane j = lane&3 makes
        // the call for row r = j (all four words are used: they are
        // the quad's four kv), reduces it to a keep nibble at bits
        // 4j..4j+3, and two quad exchanges OR the four nibbles
        // together: one call per lane per sub, as in the forward.
        unsigned keep16 = 0;
        if constexpr (DROPOUT) {
          const int j = lane & 3;
          // wave-uniform 64-bit part + 32-bit lane part
          const uint64_t grp =
              drop_row_group(bh, T, qm0 + 16 * sub) +
              (uint64_t)((unsigned)(4 * g + j) * (unsigned)(T >> 2) +
                         (unsigned)(mykv >> 2));
          unsigned nib = drop_nibble(drop, grp) << (4 * j);
          nib |= quad_xchg<USE_PERMLANE, 1>(nib);
          nib |= quad_xchg<USE_PERMLANE, 2>(nib);
          keep16 = nib >> j;    // word (kv & 3) = j of every row
        }
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = 16 * sub + 4 * g + r;     // tile-local q
          const bool valid = (qm0 + qi) >= mykv &&
                             (!DOCS || (qm0 + qi) <= myend);
          // mask the EXPONENT instead of p and ds: raw exp2 of -1e30
          // is exactly 0, and ds = scale*p*(...) inherits the zero —
          // one select instead of two per element
          const float e = valid
              ? (scale * sacc[r] - lse_a[r]) * l2e : -1e30f;
          const float p = fast_exp2(e);
          if constexpr (DROPOUT) {
            // dV += (P o M/(1-p))^T dO: the 1/(1-p) waits for the
            // epilogue; dS = scale * P o (M/(1-p) o dP - D)
            const bool keep = (keep16 >> (4 * r)) & 1u;
            pv[sub][r] = keep ? p : 0.f;
            dsv[sub][r] = scale * p *
                ((keep ? dpacc[r] * drop.scale : 0.f) - d_a[r]);
          } else {
            pv[sub][r] = p;
            dsv[sub][r] = scale * p * (dpacc[r] - d_a[r]);
          }
        }
      }
      // redistribute over the q axis -> B-fragments (k = q)
      #pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        bf16x8 pb, db;
        {
          const unsigned x0 = pack_bf16(pv[2 * blk][0], pv[2 * blk][1]);
          const unsigned x1 = pack_bf16(pv[2 * blk][2], pv[2 * blk][3]);
          const unsigned y0 = pack_bf16(pv[2 * blk + 1][0],
                                        pv[2 * blk + 1][1]);
          const unsigned y1 = pack_bf16(pv[2 * blk + 1][2],
                                        pv[2 * blk + 1][3]);
          unsigned d0, d1, d2, d3;
          redist_pair<USE_PERMLANE>(x0, y0, lane, d0, d2);
          redist_pair<USE_PERMLANE>(x1, y1, lane, d1, d3);
          unsigned* pw = reinterpret_cast<unsigned*>(&pb);
          pw[0] = d0; pw[1] = d1; pw[2] = d2; pw[3] = d3;
        }
        {
          const unsigned x0 = pack_bf16(dsv[2 * blk][0],
                                        dsv[2 * blk][1]);
          const unsigned x1 = pack_bf16(dsv[2 * blk][2],
                                        dsv[2 * blk][3]);
          const unsigned y0 = pack_bf16(dsv[2 * blk + 1][0],
                                        dsv[2 * blk + 1][1]);
          const unsigned y1 = pack_bf16(dsv[2 * blk + 1][2],
                                        dsv[2 * blk + 1][3]);
          unsigned d0, d1, d2, d3;
          redist_pair<USE_PERMLANE>(x0, y0, lane, d0, d2);
          redist_pair<USE_PERMLANE>(x1, y1, lane, d1, d3);
          unsigned* pw = reinterpret_cast<unsigned*>(&db);
          pw[0] = d0; pw[1] = d1; pw[2] = d2; pw[3] = d3;
        }
        // d-blocks in pairs: dO^T / Q^T fragments, one drain per pair
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int np = 0; np < 2; ++np) {
          bf16x8 adot[2], aqt[2];
          read_frag_tr2x2(lds_do[buf], lds_q[buf], 32 * blk, 2 * np,
                          lane, adot, aqt);
          #pragma unroll
          for (int n = 0; n < 2; ++n) {
            dv_acc[2 * np + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                adot[n], pb, dv_acc[2 * np + n], 0, 0, 0);
            dk_acc[2 * np + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                aqt[n], db, dk_acc[2 * np + n], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // write-late: next tile -> other buffers, one barrier per tile
    stage_r_write(lds_do[buf ^ 1], dt);
    stage_r_write(lds_q[buf ^ 1], qt);
    if (threadIdx.x < BN) {
      lds_lse[buf ^ 1][threadIdx.x] = nlse;
      lds_d[buf ^ 1][threadIdx.x] = nd;
    }
    __syncthreads();
  }

  // epilogue: transpose dV^T then dK^T through per-wave LDS
  __bf16* ew = lds_ep[wave];
  const int erow = lane >> 2;            // wave-local kv row
  const int ec0 = (lane & 3) * 16;
  #pragma unroll
  for (int which = 0; which < 2; ++which) {
    f32x4* acc = which ? dk_acc : dv_acc;
    __hip_bfloat16* out = which ? dK : dV;
    #pragma unroll
    for (int n = 0; n < 4; ++n)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (DROPOUT)   // dV carries the deferred 1/(1-p)
          ew[(lane & 15) * HS + 16 * n + 4 * g + r] =
              (__bf16)(which ? acc[n][r] : acc[n][r] * drop.scale);
        else
          ew[(lane & 15) * HS + 16 * n + 4 * g + r] =
              (__bf16)acc[n][r];
      }
    wait_lds();
    int4 t0 = *reinterpret_cast<const int4*>(ew + erow * HS + ec0);
    int4 t1 = *reinterpret_cast<const int4*>(ew + erow * HS + ec0 + 8);
    *reinterpret_cast<int4*>(
        out + base + (long)(kv0 + erow) * HS + ec0) = t0;
    *reinterpret_cast<int4*>(
        out + base + (long)(kv0 + erow) * HS + ec0 + 8) = t1;
    wait_lds();
  }
}

// Column-paired tr reads for dq: two 16-col blocks of the SAME rows
// from one image, single lgkm drain.
__device__ __forceinline__ void read_frag_tr_2col(const __bf16* img,
                                                  int krow0, int col16a,
                                                  int col16b, int lane,
                                                  bf16x8& va,
                                                  bf16x8& vb) {
  const int j = lane & 15;
  const int g = lane >> 4;
  const unsigned base =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)img;
  const int r0 = krow0 + 8 * g + (j >> 2);
  const int cba = (col16a + 4 * (j & 3)) * 2;
  const int cbb = (col16b + 4 * (j & 3)) * 2;
  const unsigned a0 = base + (unsigned)swz_off(r0, cba);
  const unsigned a1 = base + (unsigned)swz_off(r0 + 4, cba);
  const unsigned b0 = base + (unsigned)swz_off(r0, cbb);
  const unsigned b1 = base + (unsigned)swz_off(r0 + 4, cbb);
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  uint2v ra0, ra1, rb0, rb1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n"
      "ds_read_b64_tr_b16 %1, %5\n"
      "ds_read_b64_tr_b16 %2, %6\n"
      "ds_read_b64_tr_b16 %3, %7\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(ra0), "=&v"(ra1), "=&v"(rb0), "=&v"(rb1)
      : "v"(a0), "v"(a1), "v"(b0), "v"(b1)
      : "memory");
  unsigned* wa = reinterpret_cast<unsigned*>(&va);
  wa[0] = ra0[0]; wa[1] = ra0[1]; wa[2] = ra1[0]; wa[3] = ra1[1];
  unsigned* wb = reinterpret_cast<unsigned*>(&vb);
  wb[0] = rb0[0]; wb[1] = rb0[1]; wb[2] = rb1[0]; wb[3] = rb1[1];
}

// dQ v3: workgroup = 64 q rows, 4 waves x 16 q columns; iterate kv
// tiles of 64. lse/D are lane-resident (q fixed per lane).
//   S^T[kv][q]  = mfma(K_frag,  Q^T B-frag)
//   dP^T[kv][q] = mfma(V_frag,  dO^T B-frag)
//   dQ^T[d][q]  = mfma(K^T A-frag(lds), redist(dS^T) B-frag)
template <bool USE_PERMLANE, bool DROPOUT = false, bool DOCS = false>
// min 4 waves/EU: LDS allows 6, keep the allocator under 128 regs
__global__ __launch_bounds__(256, 4) void flash_bwd_dq_v3_kernel(
    const __hip_bfloat16* __restrict__ Qg,
    const __hip_bfloat16* __restrict__ Kg,
    const __hip_bfloat16* __restrict__ Vg,
    const __hip_bfloat16* __restrict__ dOg,
    const float* __restrict__ LSE, const float* __restrict__ Dg,
    __hip_bfloat16* __restrict__ dQ, int T, float scale,
    DropArgs drop, const int* __restrict__ doc_start, int H) {
  const int bh = blockIdx.y;
  const int qm0 = blockIdx.x * BM3;
  if (qm0 >= T) return;
  const long base = (long)bh * T * HS;
  const __hip_bfloat16* q = Qg + base;
  const __hip_bfloat16* k = Kg + base;
  const __hip_bfloat16* v = Vg + base;
  const __hip_bfloat16* dO = dOg + base;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = qm0 + wave * WQ;
  const int myq = q0 + (lane & 15);
  const int g = lane >> 4;

  __shared__ __bf16 lds_kk[2][BN * HS];  // K row-major db, 16 KB
  __shared__ __bf16 lds_vv[2][BN * HS];  // V row-major db, 16 KB
  __shared__ __bf16 lds_ep[4][WQ * HS];  // epilogue      8 KB

  bf16x8 qf[2], dof[2];
  #pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk] = load_frag_rowmajor(q, q0, kk, lane, HS);
    dof[kk] = load_frag_rowmajor(dO, q0, kk, lane, HS);
  }
  const float lse_q = LSE[(long)bh * T + myq];
  const float d_q = Dg[(long)bh * T + myq];

  f32x4 dq_acc[4];    // dQ^T: row d, col q
  #pragma unroll
  for (int n = 0; n < 4; ++n)
    dq_acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float l2e = 1.4426950408889634f;
  const int kv_end = (qm0 + BM3 < T) ? qm0 + BM3 : T;
  // DOCS: as in the forward (no dead-lane care needed here: a masked
  // entry's exponent is -1e30 against the finite lse_q, so its dS is 0)
  int mystart = 0, wstart_lo = 0, kv_begin = 0;
  if constexpr (DOCS) {
    const int* ds = doc_start + (long)(bh / H) * T;
    mystart = ds[myq];
    wstart_lo = uniform_bound(ds, q0);
    const int s0 = uniform_bound(ds, qm0);
    kv_begin = (s0 < 0 ? 0 : (s0 > qm0 ? qm0 : s0)) & ~(BN - 1);
  }
  {
    StageRegsR kt = stage_r_load(k, kv_begin);
    StageRegsR vt = stage_r_load(v, kv_begin);
    stage_r_write(lds_kk[0], kt);
    stage_r_write(lds_vv[0], vt);
  }
  __syncthreads();
  int buf = 0;
  for (int kn0 = kv_begin; kn0 < kv_end; kn0 += BN, buf ^= 1) {
    const int next = (kn0 + BN < kv_end) ? kn0 + BN : kn0;
    StageRegsR kt = stage_r_load(k, next);
    StageRegsR vt = stage_r_load(v, next);
    const bool active = kn0 <= q0 + WQ - 1 &&
                        (!DOCS || kn0 + BN - 1 >= wstart_lo);
    if (active) {
      float dsv[4][4];
      #pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        bf16x8 ak0 = read_frag_swz(lds_kk[buf], 16 * sub, 0, lane);
        bf16x8 ak1 = read_frag_swz(lds_kk[buf], 16 * sub, 1, lane);
        bf16x8 av0 = read_frag_swz(lds_vv[buf], 16 * sub, 0, lane);
        bf16x8 av1 = read_frag_swz(lds_vv[buf], 16 * sub, 1, lane);
        f32x4 st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ak0, qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ak1, qf[1], st, 0, 0, 0);
        f32x4 dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            av0, dof[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            av1, dof[1], dpt, 0, 0, 0);
        if constexpr (DROPOUT) {
          // the forward's layout: this lane's four r are one aligned
          // kv group of row myq -> one lane-local call per sub;
          // dS = scale * P o (M/(1-p) o dP - D)
          // (group index = wave-uniform 64-bit + 32-bit lane part)
          const uint4 w = drop_words(
              drop, drop_row_group(bh, T, q0) +
                        (uint64_t)((kn0 >> 2) + 4 * sub) +
                        (uint64_t)((unsigned)(lane & 15) *
                                       (unsigned)(T >> 2) +
                                   (unsigned)g));
          dpt[0] = w.x >= drop.thr ? dpt[0] * drop.scale : 0.f;
          dpt[1] = w.y >= drop.thr ? dpt[1] * drop.scale : 0.f;
          dpt[2] = w.z >= drop.thr ? dpt[2] * drop.scale : 0.f;
          dpt[3] = w.w >= drop.thr ? dpt[3] * drop.scale : 0.f;
        }
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kvr = kn0 + 16 * sub + 4 * g + r;
          const bool valid = kvr <= myq && (!DOCS || kvr >= mystart);
          const float e = valid
              ? (scale * st[r] - lse_q) * l2e : -1e30f;
          dsv[sub][r] = scale * fast_exp2(e) * (dpt[r] - d_q);
        }
      }
      #pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        bf16x8 db;
        const unsigned x0 = pack_bf16(dsv[2 * blk][0], dsv[2 * blk][1]);
        const unsigned x1 = pack_bf16(dsv[2 * blk][2], dsv[2 * blk][3]);
        const unsigned y0 = pack_bf16(dsv[2 * blk + 1][0],
                                      dsv[2 * blk + 1][1]);
        const unsigned y1 = pack_bf16(dsv[2 * blk + 1][2],
                                      dsv[2 * blk + 1][3]);
        unsigned d0, d1, d2, d3;
        redist_pair<USE_PERMLANE>(x0, y0, lane, d0, d2);
        redist_pair<USE_PERMLANE>(x1, y1, lane, d1, d3);
        unsigned* pw = reinterpret_cast<unsigned*>(&db);
        pw[0] = d0; pw[1] = d1; pw[2] = d2; pw[3] = d3;
        // K^T fragments (row d, k = kv) in column pairs: one drain
        // per pair instead of one per d-block
        #pragma unroll
        for (int np = 0; np < 2; ++np) {
          bf16x8 ak0, ak1;
          read_frag_tr_2col(lds_kk[buf], 32 * blk, 32 * np,
                            32 * np + 16, lane, ak0, ak1);
          dq_acc[2 * np] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ak0, db, dq_acc[2 * np], 0, 0, 0);
          dq_acc[2 * np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ak1, db, dq_acc[2 * np + 1], 0, 0, 0);
        }
      }
    }
    stage_r_write(lds_kk[buf ^ 1], kt);
    stage_r_write(lds_vv[buf ^ 1], vt);
    __syncthreads();
  }

  // epilogue transpose
  __bf16* ew = lds_ep[wave];
  #pragma unroll
  for (int n = 0; n < 4; ++n)
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      ew[(lane & 15) * HS + 16 * n + 4 * g + r] = (__bf16)dq_acc[n][r];
  wait_lds();
  const int erow = lane >> 2;
  const int ec0 = (lane & 3) * 16;
  int4 t0 = *reinterpret_cast<const int4*>(ew + erow * HS + ec0);
  int4 t1 = *reinterpret_cast<const int4*>(ew + erow * HS + ec0 + 8);
  *reinterpret_cast<int4*>(
      dQ + base + (long)(q0 + erow) * HS + ec0) = t0;
  *reinterpret_cast<int4*>(
      dQ + base + (long)(q0 + erow) * HS + ec0 + 8) = t1;
}

// =====================================================================
// host side: one set of operand checks, one launcher per direction
// =====================================================================

// The kernels index every operand with q's extents, so every operand
// must have them; blockIdx.y carries B*H. p is the dropout entry points'
// probability (the p = 0 entry points pass 0), checked right after q.
void check_flash_q(const torch::Tensor& q, double p) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 &&
                  q.is_contiguous(),
              "flash_attn_v3: bf16 contiguous GPU tensors");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == HS,
              "flash_attn_v3: [B,H,T,64] expected");
  TORCH_CHECK(q.size(2) % BM3 == 0 && q.size(2) > 0,
              "flash_attn_v3: T % 64 == 0");
  TORCH_CHECK(q.size(0) * q.size(1) <= 65535,
              "flash_attn_v3: B*H > 65535");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "flash_attn_v3: p must be in [0, 1)");
}

void check_flash_operand(const torch::Tensor& t, const torch::Tensor& q,
                         const char* what) {
  TORCH_CHECK(t.sizes() == q.sizes() &&
                  t.scalar_type() == q.scalar_type() &&
                  t.device() == q.device() && t.is_contiguous(),
              "flash_attn_v3: ", what,
              " must be contiguous with q's sizes, dtype and device");
}

void check_flash_fwd(const torch::Tensor& q, const torch::Tensor& k,
                     const torch::Tensor& v, double p = 0.0) {
  check_flash_q(q, p);
  check_flash_operand(k, q, "k");
  check_flash_operand(v, q, "v");
}

// dout is the caller's dout.contiguous()
void check_flash_bwd(const torch::Tensor& dout, const torch::Tensor& q,
                     const torch::Tensor& k, const torch::Tensor& v,
                     const torch::Tensor& o, const torch::Tensor& lse,
                     double p = 0.0) {
  check_flash_fwd(q, k, v, p);
  check_flash_operand(o, q, "o");
  check_flash_operand(dout, q, "dout");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.device() == q.device() &&
                  lse.numel() == q.size(0) * q.size(1) * q.size(2),
              "flash_attn_v3: lse must be fp32 [B,H,T] on q's device");
}

// A document bound (doc_start or doc_end) of the DOCS entry points. Only
// its layout is checked: the kernels never index with its values (see
// "document masking" above).
void check_flash_bound(const torch::Tensor& t, const torch::Tensor& q,
                       const char* what) {
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous() &&
                  t.device() == q.device() && t.dim() == 2 &&
                  t.size(0) == q.size(0) && t.size(1) == q.size(2),
              "flash_attn_v3: ", what,
              " must be int32 contiguous [B,T] on q's device");
}

const __hip_bfloat16* bf16_in(const torch::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
__hip_bfloat16* bf16_out(torch::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

// The instantiation for (use_permlane, dropout, docs): all eight of a
// kernel have one signature.
#define RLA_PICK_V3(KERNEL, pl, dr, dc)                                  \
  ((dc) ? ((dr) ? ((pl) ? KERNEL<true, true, true>                       \
                        : KERNEL<false, true, true>)                     \
                : ((pl) ? KERNEL<true, false, true>                      \
                        : KERNEL<false, false, true>))                   \
        : ((dr) ? ((pl) ? KERNEL<true, true, false>                      \
                        : KERNEL<false, true, false>)                    \
                : ((pl) ? KERNEL<true, false, false>                     \
                        : KERNEL<false, false, false>)))

const int* bound_ptr(const torch::Tensor* t) {
  return t ? t->data_ptr<int>() : nullptr;
}

// Operands are already checked. Returns (o, lse); with dropout, lse is
// that of the undropped softmax. doc_start (checked too) selects the
// DOCS instantiation; nullptr is plain causal attention.
std::pair<torch::Tensor, torch::Tensor> launch_flash_fwd(
    const torch::Tensor& q, const torch::Tensor& k,
    const torch::Tensor& v, double scale, const DropArgs& drop,
    bool dropout, bool use_permlane,
    const torch::Tensor* doc_start = nullptr) {
  const int B = (int)q.size(0), H = (int)q.size(1), T = (int)q.size(2);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid(T / BM3, B * H);
  auto* kern = RLA_PICK_V3(flash_fwd_v3_kernel, use_permlane, dropout,
                           doc_start != nullptr);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, bf16_in(q),
                     bf16_in(k), bf16_in(v), bf16_out(o),
                     lse.data_ptr<float>(), T, (float)scale, drop,
                     bound_ptr(doc_start), H);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "flash_fwd_v3: ", hipGetErrorString(e));
  return {o, lse};
}

// Operands are already checked. D = rowsum(dO o O), then dK/dV, then dQ.
// doc_start and doc_end (checked too) come together or not at all.
std::vector<torch::Tensor> launch_flash_bwd(
    const torch::Tensor& dout, const torch::Tensor& q,
    const torch::Tensor& k, const torch::Tensor& v,
    const torch::Tensor& o, const torch::Tensor& lse, double scale,
    const DropArgs& drop, bool dropout, bool use_permlane,
    const torch::Tensor* doc_start = nullptr,
    const torch::Tensor* doc_end = nullptr) {
  const bool docs = doc_start != nullptr;
  const int B = (int)q.size(0), H = (int)q.size(1), T = (int)q.size(2);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto D = torch::empty({B, H, T}, q.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  const long total_rows = (long)B * H * T;
  hipLaunchKernelGGL(flash_bwd_pre_kernel,
                     dim3((total_rows + 63) / 64), dim3(256), 0, stream,
                     bf16_in(dout), bf16_in(o), D.data_ptr<float>(),
                     total_rows);
  dim3 grid(T / BM3, B * H);
  auto* kdkv = RLA_PICK_V3(flash_bwd_dkv_v3_kernel, use_permlane,
                           dropout, docs);
  auto* kdq = RLA_PICK_V3(flash_bwd_dq_v3_kernel, use_permlane, dropout,
                          docs);
  hipLaunchKernelGGL(kdkv, grid, dim3(256), 0, stream, bf16_in(q),
                     bf16_in(k), bf16_in(v), bf16_in(dout),
                     lse.data_ptr<float>(), D.data_ptr<float>(),
                     bf16_out(dk), bf16_out(dv), T, (float)scale, drop,
                     bound_ptr(doc_end), H);
  hipLaunchKernelGGL(kdq, grid, dim3(256), 0, stream, bf16_in(q),
                     bf16_in(k), bf16_in(v), bf16_in(dout),
                     lse.data_ptr<float>(), D.data_ptr<float>(),
                     bf16_out(dq), T, (float)scale, drop,
                     bound_ptr(doc_start), H);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "flash_bwd_v3: ", hipGetErrorString(e));
  return {dq, dk, dv};
}

}  // namespace

std::vector<torch::Tensor> flash_attn_fwd_v3(torch::Tensor q,
                                             torch::Tensor k,
                                             torch::Tensor v,
                                             double scale,
                                             bool use_permlane) {
  check_flash_fwd(q, k, v);
  auto [o, lse] = launch_flash_fwd(q, k, v, scale, DropArgs{}, false,
                                   use_permlane);
  return {o, lse};
}

std::vector<torch::Tensor> flash_attn_bwd_v3(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor o, torch::Tensor lse, double scale,
    bool use_permlane) {
  dout = dout.contiguous();
  check_flash_bwd(dout, q, k, v, o, lse);
  return launch_flash_bwd(dout, q, k, v, o, lse, scale, DropArgs{},
                          false, use_permlane);
}

// Forward with dropout on the attention probabilities. Draws (seed,
// offset) from the default generator of q's device, exactly as
// fused_ln_fwd does for p > 0, and returns (o, lse, seed, offset).
namespace {
std::tuple<torch::Tensor, torch::Tensor, uint64_t, uint64_t>
flash_fwd_dropout(const torch::Tensor& q, const torch::Tensor& k,
                  const torch::Tensor& v, double scale, double p,
                  bool use_permlane, const torch::Tensor* doc_start) {
  // graph-capture-safe RNG (device-side offset) is not implemented
  at::cuda::assertNotCapturing(
      "flash_attn_v3_dropout: drawing the dropout seed");
  std::pair<uint64_t, uint64_t> rng;
  {
    auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
        c10::nullopt,
        at::cuda::detail::getDefaultCUDAGenerator(q.get_device()));
    std::lock_guard<std::mutex> lock(gen->mutex_);
    rng = gen->philox_engine_inputs(4);
  }
  auto [o, lse] = launch_flash_fwd(
      q, k, v, scale, make_drop_args(p, rng.first, rng.second), true,
      use_permlane, doc_start);
  return {o, lse, rng.first, rng.second};
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor, uint64_t, uint64_t>
flash_attn_fwd_v3_dropout(torch::Tensor q, torch::Tensor k,
                          torch::Tensor v, double scale, double p,
                          bool use_permlane) {
  check_flash_fwd(q, k, v, p);
  return flash_fwd_dropout(q, k, v, scale, p, use_permlane, nullptr);
}

// Backward of flash_attn_fwd_v3_dropout: the mask is drawn again from
// the (seed, offset) the forward returned.
std::vector<torch::Tensor> flash_attn_bwd_v3_dropout(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor o, torch::Tensor lse, double scale,
    double p, uint64_t seed, uint64_t offset, bool use_permlane) {
  dout = dout.contiguous();
  check_flash_bwd(dout, q, k, v, o, lse, p);
  return launch_flash_bwd(dout, q, k, v, o, lse, scale,
                          make_drop_args(p, seed, offset), true,
                          use_permlane);
}

// Document-masked variants (the DOCS instantiations): q attends kv iff
// doc_start[b, q] <= kv <= q; doc_end[b, kv] is the last q that attends
// kv. Both are int32 [B, T]; ops/flash_attn.py derives them.
std::vector<torch::Tensor> flash_attn_fwd_v3_docs(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor doc_start, double scale, bool use_permlane) {
  check_flash_fwd(q, k, v);
  check_flash_bound(doc_start, q, "doc_start");
  auto [o, lse] = launch_flash_fwd(q, k, v, scale, DropArgs{}, false,
                                   use_permlane, &doc_start);
  return {o, lse};
}

std::vector<torch::Tensor> flash_attn_bwd_v3_docs(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor o, torch::Tensor lse,
    torch::Tensor doc_start, torch::Tensor doc_end, double scale,
    bool use_permlane) {
  dout = dout.contiguous();
  check_flash_bwd(dout, q, k, v, o, lse);
  check_flash_bound(doc_start, q, "doc_start");
  check_flash_bound(doc_end, q, "doc_end");
  return launch_flash_bwd(dout, q, k, v, o, lse, scale, DropArgs{},
                          false, use_permlane, &doc_start, &doc_end);
}

std::tuple<torch::Tensor, torch::Tensor, uint64_t, uint64_t>
flash_attn_fwd_v3_docs_dropout(torch::Tensor q, torch::Tensor k,
                               torch::Tensor v, torch::Tensor doc_start,
                               double scale, double p,
                               bool use_permlane) {
  check_flash_fwd(q, k, v, p);
  check_flash_bound(doc_start, q, "doc_start");
  return flash_fwd_dropout(q, k, v, scale, p, use_permlane, &doc_start);
}

std::vector<torch::Tensor> flash_attn_bwd_v3_docs_dropout(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor o, torch::Tensor lse,
    torch::Tensor doc_start, torch::Tensor doc_end, double scale,
    double p, uint64_t seed, uint64_t offset, bool use_permlane) {
  dout = dout.contiguous();
  check_flash_bwd(dout, q, k, v, o, lse, p);
  check_flash_bound(doc_start, q, "doc_start");
  check_flash_bound(doc_end, q, "doc_end");
  return launch_flash_bwd(dout, q, k, v, o, lse, scale,
                          make_drop_args(p, seed, offset), true,
                          use_permlane, &doc_start, &doc_end);
}

// =====================================================================
// forward v4 — 32x32x16 MFMA shape: half the MFMA instructions per
// query of v3 (fwd v3 is issue-bound: SQ_WAIT_INST 42%, MFMA-busy 19%).
// Same swapped-operand structure; P^T -> PV B-fragments need only ONE
// permlane32_swap per dword pair (lanes l and l+32 share the q column
// in BOTH the S^T C-layout and the PV B-layout).
// Layouts (mfma_probe32-verified):
//   A[32Mx16K]: lane l elem i -> row l&31, k (l>>5)*8+i
//   B[16Kx32N]: lane l elem i -> col l&31, k (l>>5)*8+i
//   C (16 f32): col l&31, row (r&3) + 8*(r>>2) + 4*(l>>5)
// =====================================================================
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int WQ4 = 32;    // q columns per wave
constexpr int BM4 = 128;   // q rows per workgroup (4 waves)

// b128 A-fragment from the swizzled row-major image, 32-row block:
// row = row0 + (lane&31), k-chunk c of 16: byte = c*32 + (lane>>5)*16
__device__ __forceinline__ bf16x8 read_frag_swz32(const __bf16* img,
                                                  int row0, int c,
                                                  int lane) {
  const int row = row0 + (lane & 31);
  bf16x8 v;
  *reinterpret_cast<int4*>(&v) = *reinterpret_cast<const int4*>(
      reinterpret_cast<const char*>(img) +
      swz_off(row, 32 * c + 16 * (lane >> 5)));
  return v;
}

// Paired tr4: two adjacent kv chunks of the same 16-col block with a
// single lgkm drain (8 serial drains per tile were parking v4 75%).
__device__ __forceinline__ void read_frag_tr4x2(const __bf16* img,
                                                int krow0a, int krow0b,
                                                int col16, int lane,
                                                bf16x8& va, bf16x8& vb) {
  const int j = lane & 15;
  const unsigned base =
      (unsigned)(size_t)(__attribute__((address_space(3))) const char*)
          (const void*)img;
  const int cb = (col16 + 4 * (j & 3)) * 2;
  const unsigned a0 = base + (unsigned)swz_off(krow0a + (j >> 2), cb);
  const unsigned a1 =
      base + (unsigned)swz_off(krow0a + 4 + (j >> 2), cb);
  const unsigned b0 = base + (unsigned)swz_off(krow0b + (j >> 2), cb);
  const unsigned b1 =
      base + (unsigned)swz_off(krow0b + 4 + (j >> 2), cb);
  typedef __attribute__((ext_vector_type(2))) unsigned uint2v;
  uint2v ra0, ra1, rb0, rb1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n"
      "ds_read_b64_tr_b16 %1, %5\n"
      "ds_read_b64_tr_b16 %2, %6\n"
      "ds_read_b64_tr_b16 %3, %7\n"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(ra0), "=&v"(ra1), "=&v"(rb0), "=&v"(rb1)
      : "v"(a0), "v"(a1), "v"(b0), "v"(b1)
      : "memory");
  unsigned* wa = reinterpret_cast<unsigned*>(&va);
  wa[0] = ra0[0]; wa[1] = ra0[1]; wa[2] = ra1[0]; wa[3] = ra1[1];
  unsigned* wb = reinterpret_cast<unsigned*>(&vb);
  wb[0] = rb0[0]; wb[1] = rb0[1]; wb[2] = rb1[0]; wb[3] = rb1[1];
}

// NOTE: no forced min-waves — occupancy pressure made the allocator
// spill, and spill-reload of address registers around in-flight ops
// produced stray writes (the r02 dk nondeterminism, profiles/
// r02_flash_v3.md postmortem). Keep hand-asm kernels spill-free.
__global__ __launch_bounds__(256) void flash_fwd_v4_kernel(
    const __hip_bfloat16* __restrict__ Q,
    const __hip_bfloat16* __restrict__ K,
    const __hip_bfloat16* __restrict__ V,
    __hip_bfloat16* __restrict__ O, float* __restrict__ LSE,
    int T, float scale) {
  const int bh = blockIdx.y;
  const int qm0 = blockIdx.x * BM4;
  if (qm0 >= T) return;
  const long base = (long)bh * T * HS;
  const __hip_bfloat16* q = Q + base;
  const __hip_bfloat16* k = K + base;
  const __hip_bfloat16* v = V + base;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = qm0 + wave * WQ4;
  const int myq = q0 + (lane & 31);
  const int hi = lane >> 5;

  __shared__ __bf16 lds_v[2][BN * HS];   // V row-major db, 16 KB
  __shared__ __bf16 lds_k[2][BN * HS];   // K row-major db, 16 KB

  // Q^T B-fragments: col = q = lane&31, k = hs = 4 chunks of 16
  bf16x8 qf[4];
  #pragma unroll
  for (int c = 0; c < 4; ++c) {
    *reinterpret_cast<int4*>(&qf[c]) =
        *reinterpret_cast<const int4*>(
            q + (long)(q0 + (lane & 31)) * HS + c * 16 + hi * 8);
  }

  float m_i = kNegInf, l_i = 0.f;
  f32x16 o_acc[2];   // O^T: row d = 32*dt + (r&3)+8*(r>>2)+4*hi
  o_acc[0] = f32x16{};
  o_acc[1] = f32x16{};

  const float l2e = 1.4426950408889634f * scale;
  const int kv_end = (qm0 + BM4 < T) ? qm0 + BM4 : T;
  {
    StageRegsR vt = stage_r_load(v, 0);
    StageRegsR kt = stage_r_load(k, 0);
    stage_r_write(lds_v[0], vt);
    stage_r_write(lds_k[0], kt);
  }
  __syncthreads();
  int buf = 0;
  for (int kn0 = 0; kn0 < kv_end; kn0 += BN, buf ^= 1) {
    const int next = (kn0 + BN < kv_end) ? kn0 + BN : kn0;
    StageRegsR vt = stage_r_load(v, next);
    StageRegsR kt = stage_r_load(k, next);
    const bool active = kn0 <= q0 + WQ4 - 1;
    if (active) {
      // --- S^T = K Q^T: lane holds 32 kv of column myq --------------
      f32x16 st[2];
      #pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        st[sub] = f32x16{};
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
          bf16x8 kf = read_frag_swz32(lds_k[buf], 32 * sub, c, lane);
          st[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              kf, qf[c], st[sub], 0, 0, 0);
        }
      }
      // --- causal mask ----------------------------------------------
      if (kn0 + BN - 1 > q0) {
        #pragma unroll
        for (int sub = 0; sub < 2; ++sub)
          #pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kn0 + 32 * sub + (r & 3) + 8 * (r >> 2) +
                           4 * hi;
            if (kv > myq) st[sub][r] = kNegInf;
          }
      }
      // --- online softmax: lane-local over 32 + ONE cross-lane ------
      float mx = kNegInf;
      #pragma unroll
      for (int sub = 0; sub < 2; ++sub)
        #pragma unroll
        for (int r = 0; r < 16; ++r)
          mx = fmaxf(mx, st[sub][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const bool defer = __all((mx - m_i) * l2e <= 8.0f);
      float m_new, corr;
      if (defer) {
        m_new = m_i;
        corr = 1.0f;
      } else {
        m_new = fmaxf(m_i, mx);
        corr = fast_exp2((m_i - m_new) * l2e);
        #pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          #pragma unroll
          for (int r = 0; r < 16; ++r)
            o_acc[dt][r] *= corr;
      }
      float rowsum = 0.f;
      #pragma unroll
      for (int sub = 0; sub < 2; ++sub)
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2((st[sub][r] - m_new) * l2e);
          st[sub][r] = p;
          rowsum += p;
        }
      rowsum += __shfl_xor(rowsum, 32, 64);
      l_i = l_i * corr + rowsum;
      m_i = m_new;
      // --- P^T -> PV B-fragments: one pl32swap per dword pair -------
      // chunk t (kv 16t..16t+15): lane(hi) needs kv 16t+8*hi+i.
      // From C regs of sub=t>>1: rows 16*(t&1)+{0..3}+4hi (regs
      // 8*(t&1)+0..3) and 16*(t&1)+{8..11}+4hi (regs 8*(t&1)+4..7):
      //   L_j = pack(rows 4j block), H_j = pack(rows 8+4j block)
      //   (P_j, S_j) = pl32swap(L_j, H_j) -> frag = [P0, P1, S0, S1]
      bf16x8 pb[4];
      #pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float* sv = reinterpret_cast<const float*>(&st[t >> 1]);
        const int rb = 8 * (t & 1);
        const unsigned l0 = pack_bf16(sv[rb + 0], sv[rb + 1]);
        const unsigned l1 = pack_bf16(sv[rb + 2], sv[rb + 3]);
        const unsigned h0 = pack_bf16(sv[rb + 4], sv[rb + 5]);
        const unsigned h1 = pack_bf16(sv[rb + 6], sv[rb + 7]);
        auto ps0 = __builtin_amdgcn_permlane32_swap(l0, h0, false,
                                                    false);
        auto ps1 = __builtin_amdgcn_permlane32_swap(l1, h1, false,
                                                    false);
        unsigned* w = reinterpret_cast<unsigned*>(&pb[t]);
        w[0] = ps0[0]; w[1] = ps1[0]; w[2] = ps0[1]; w[3] = ps1[1];
      }
      // --- O^T += V^T P^T -------------------------------------------
      const int g = lane >> 4;
      #pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        #pragma unroll
        for (int t = 0; t < 4; t += 2) {
          bf16x8 va, vb;
          read_frag_tr4x2(lds_v[buf], 16 * t + 8 * (g >> 1),
                          16 * (t + 1) + 8 * (g >> 1),
                          32 * dt + 16 * (g & 1), lane, va, vb);
          o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              va, pb[t], o_acc[dt], 0, 0, 0);
          o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              vb, pb[t + 1], o_acc[dt], 0, 0, 0);
        }
      }
    }
    stage_r_write(lds_v[buf ^ 1], vt);
    stage_r_write(lds_k[buf ^ 1], kt);
    __syncthreads();
  }

  // --- epilogue: transpose O^T -> O rows via dead K image LDS -------
  __bf16* ow = lds_k[0] + wave * (WQ4 * HS);
  const float inv_l = (l_i > 0.f) ? 1.f / l_i : 0.f;
  #pragma unroll
  for (int dt = 0; dt < 2; ++dt)
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = 32 * dt + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ow[(lane & 31) * HS + d] = (__bf16)(o_acc[dt][r] * inv_l);
    }
  wait_lds();
  {
    const int row = lane >> 1;           // wave-local q row 0..31
    const int c0 = (lane & 1) * 32;
    int4 t0 = *reinterpret_cast<const int4*>(ow + row * HS + c0);
    int4 t1 = *reinterpret_cast<const int4*>(ow + row * HS + c0 + 8);
    int4 t2 = *reinterpret_cast<const int4*>(ow + row * HS + c0 + 16);
    int4 t3 = *reinterpret_cast<const int4*>(ow + row * HS + c0 + 24);
    __hip_bfloat16* op = O + base + (long)(q0 + row) * HS + c0;
    *reinterpret_cast<int4*>(op) = t0;
    *reinterpret_cast<int4*>(op + 8) = t1;
    *reinterpret_cast<int4*>(op + 16) = t2;
    *reinterpret_cast<int4*>(op + 24) = t3;
  }
  if (hi == 0)
    LSE[(long)bh * T + myq] = m_i * scale + logf(fmaxf(l_i, 1e-30f));
}

}  // namespace

std::vector<torch::Tensor> flash_attn_fwd_v4(torch::Tensor q,
                                             torch::Tensor k,
                                             torch::Tensor v,
                                             double scale) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 &&
              q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous(), "flash_attn_fwd_v4: bf16 contiguous");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == HS,
              "flash_attn_fwd_v4: [B,H,T,64] expected");
  const int B = (int)q.size(0), H = (int)q.size(1), T = (int)q.size(2);
  TORCH_CHECK(T % BM4 == 0, "flash_attn_fwd_v4: T % 128 == 0");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid(T / BM4, B * H);
  hipLaunchKernelGGL(flash_fwd_v4_kernel, grid, dim3(256), 0, stream,
                     reinterpret_cast<const __hip_bfloat16*>(q.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(k.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(v.data_ptr()),
                     reinterpret_cast<__hip_bfloat16*>(o.data_ptr()),
                     lse.data_ptr<float>(), T, (float)scale);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "flash_fwd_v4: ", hipGetErrorString(e));
  return {o, lse};
}
