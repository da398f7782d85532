// 256x256-tile MXFP8 GEMM (e4m3 elements, one E8M0 scale per 32 k-values of every operand row):
//   C[m][n] = epilogue( sum_k 2^(sa[m][k/32]-127) * 2^(sb[n][k/32]-127) * A[m][k] * B[n][k] )
// A [M][K], B [N][K] K-contiguous bytes, sa [M][K/32], sb [N][K/32] row-major bytes, K % 128 == 0 (the
// quantiser in mxfp8.hip pads to that), N % 4 == 0.
//
// The operand pipeline is gemm_fp8_256_kernel's: one 512-thread workgroup per tile, 8 waves as 2 (M) x 4 (N)
// with 128 x 64 outputs each, operand tiles of 256 rows x 128 k-bytes (one v_mfma_scale_f32_16x16x128_f8f6f4
// k-step) by LDS-DMA into two 64 KiB stages with the 16-B chunk swizzle c ^ ((r & 6) | ((r >> 3) & 1)), a
// counted vmcnt per wave and raw barriers, so the copy of tile k+2 is in flight across tile k+1.
//
// What is new is the scales.  The MFMA takes one scale byte per lane per operand (op_sel 0: bits 7:0 of the
// scale register): lane l's byte scales row l & 15, k-values 32 (l >> 4) .. +32 of the k-step.  The operand
// registers are laid out differently: lane l's first four VGPRs hold k = 16 (l >> 4) .. +16 and its last
// four k = 64 + 16 (l >> 4) .. +16 (found from the GEMM test: with 32 contiguous k-bytes per lane, as the
// per-tensor kernel loads them - any k order serves unit scales - the result matched block scales applied
// in exactly this order).  So a stage row holds memory chunk g of its 128 k-bytes at position 2g and chunk
// 4 + g at position 2g + 1 (before the swizzle): the fragment reads and their bank pattern stay those of the
// per-tensor kernel, and the permutation costs nothing - it is folded into the DMA source addresses.  Per k-step the workgroup needs 512 rows x 4 bytes = 2 KiB, and one row's
// four bytes are one aligned dword of the row-major scale array.  They travel THROUGH THE DMA STAGE: each
// wave adds one global_load_lds_dword (64 rows x 1 dword) to the 8 operand copies of a stage, landing in a
// 2 KiB area behind the operand stages (LDS: 2 x 64 KiB + 2 x 2 KiB = 132 KiB), and reads its 12 bytes per
// k-step back with ds_read_u8 at compile-time offsets from one per-lane address.  Why this way:
//   * nothing lands on the MFMA issue path: a ds_read_u8 delivers the zero-extended byte the MFMA wants, no
//     shift, v_perm or v_bfe per tile, and the 12 reads ride the lgkmcnt wait of the 24 fragment reads;
//   * loads straight into registers would be compiler-visible VMEM between the hand-counted DMA copies (its
//     own vmcnt waits would then drain the copy of the next tile) and would hold 24 more VGPRs one k-step
//     ahead next to the 128 accumulators;
//   * a quantiser-side swizzle (one dword per lane for four tiles through op_sel) ties the scale layout to this
//     kernel's wave tiling; row-major scales serve both GEMM operands of every orientation and stay checkable
//     byte for byte.
// The counted wait becomes vmcnt(9).  The four 16-lane groups of a wave read the four bytes of the same 16
// dwords: a broadcast, no bank conflict.
//
// Epilogue: gemm256_store without the e4m3-output path (bias, GELU, residual, pre-activation copy; split-K fp32
// partial planes), dequantisation scale 1 - the block scales are already applied inside the MFMA.  Edge
// tiles: source rows are clamped (operands and scales), rows / columns past the edge are dropped on store.
// A second instantiation (MXOUT) ends in gemm256_store_mx instead: the same values leave as MXFP8 in both
// orientations (what mx_quantize would make of the bf16 C), with their column sums, for the next GEMMs.
#include <algorithm>

#include "device_common.h"
#include "gemm256_epilogue.h"
#include "kernels.h"

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

constexpr int TM = 256, TN = 256, TK = 128;  // TK in bytes (= e4m3 values) = 4 MX blocks
constexpr int STAGE = (TM + TN) * TK;        // 64 KiB: A rows then B rows, 128 B each
constexpr int SCALES = (TM + TN) * 4;        // 2 KiB: one dword (the k-step's 4 block scales) per stage row
constexpr int DMA_PER_WAVE = (TM + TN) * TK / 1024 / 8;  // 8 operand wave-instructions of 1 KiB per stage
constexpr int GROUP_M = 4;

typedef int i32x8 __attribute__((ext_vector_type(8)));

// per lane global -> LDS at (wave-uniform LDS base + lane * 16 / lane * 4) from (wave-uniform global base + this
// lane's 32-bit byte offset): the sources of a stage cost one VGPR each.  M0 is set inside the asm.
__device__ __forceinline__ void glds16(const void* gbase, unsigned off, const void* lds_wave_base) {
  const unsigned base = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)((const __attribute__((address_space(3))) char*)(lds_wave_base)));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(base), "v"(off), "s"(gbase)
               : "memory");
}
__device__ __forceinline__ void glds4(const void* gbase, unsigned off, const void* lds_wave_base) {
  const unsigned base = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)((const __attribute__((address_space(3))) char*)(lds_wave_base)));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(base), "v"(off), "s"(gbase)
               : "memory");
}

__device__ __forceinline__ int chunk_swz(int r) { return (r & 6) | ((r >> 3) & 1); }

__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// MXOUT: the epilogue writes MXFP8 (gemm256_store_mx) instead of bf16 / fp32 / split-K planes
template <bool MXOUT>
__global__ __launch_bounds__(512, 1) void gemm_mxfp8_256_kernel(const uint8_t* __restrict__ A,
                                                               const uint8_t* __restrict__ SA,
                                                               const uint8_t* __restrict__ B,
                                                               const uint8_t* __restrict__ SB, GemmEpilogue ep, int M,
                                                               int N, int K, int tiles_m, int tiles_n,
                                                               int k_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + 2 * SCALES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int split = blockIdx.y;
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  int tm, tn;
  grouped_tile(t, tiles_m, tiles_n, GROUP_M, tm, tn);  // L2 reuse across the XCD's concurrent tiles
  const int m0 = tm * TM, n0 = tn * TN;
  const int kbeg = split * k_per_split, kend = min(K, kbeg + k_per_split);
  const int nkt = max(0, (kend - kbeg) / TK);
  const int64_t lds = K / 32;  // scale row stride

  // DMA sources.  Operand wave instruction i = 8*wave + j covers stage rows 8*i .. 8*i+7 (A rows for i < 32,
  // i.e. waves 0-3, then B rows); lane -> row 8*i + (lane >> 3), physical chunk lane & 7 = position
  // (lane & 7) ^ f(row) of the row's chunk order 0, 4, 1, 5, 2, 6, 3, 7 (see the header).  Scales: wave w covers stage rows 64 w .. 64 w + 63, one dword per lane.  Rows past
  // the edge re-read the last one (dropped on store).  Offsets are relative to the tile's first row: < 2^32.
  const bool is_a = wave < 4;  // wave-uniform
  const int row0 = is_a ? m0 : n0, rows = is_a ? M : N;
  const uint8_t* obase = (is_a ? A : B) + (int64_t)row0 * K + kbeg;
  const uint8_t* sbase = (is_a ? SA : SB) + (int64_t)row0 * lds + kbeg / 32;
  unsigned off[DMA_PER_WAVE];
#pragma unroll
  for (int j = 0; j < DMA_PER_WAVE; ++j) {
    const int r = 8 * ((DMA_PER_WAVE * wave + j) & 31) + (lane >> 3);
    const int pos = (lane & 7) ^ chunk_swz(r);       // un-swizzled stage position of this lane's chunk
    const int mc = (pos >> 1) + 4 * (pos & 1);       // ... which holds memory chunk g (pos 2g) or 4 + g (pos 2g + 1)
    off[j] = (unsigned)(min(r, rows - 1 - row0)) * (unsigned)K + mc * 16;
  }
  const unsigned soff = (unsigned)min(64 * (wave & 3) + lane, rows - 1 - row0) * (unsigned)lds;
  auto issue = [&](int kt, int s) {
    char* st = smem + s * STAGE + DMA_PER_WAVE * wave * 1024;
    const uint8_t* ob = obase + (int64_t)kt * TK;
#pragma unroll
    for (int j = 0; j < DMA_PER_WAVE; ++j) glds16(ob, off[j], st + j * 1024);
    glds4(sbase + kt * 4, soff, smem + 2 * STAGE + s * SCALES + wave * 256);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero_f32x4();

  // fragment byte offsets inside a stage: row R = tile row + (lane & 15), positions 2*(lane>>4) and +1 (memory
  // chunks lane >> 4 and 4 + (lane >> 4)); scale byte lane >> 4 of the row's dword
  const int c0 = 2 * (lane >> 4), fr = chunk_swz(lane & 15);
  const int sw0 = ((c0 ^ fr) << 4), sw1 = (((c0 + 1) ^ fr) << 4);
  const int a_off = (wm * 128 + (lane & 15)) * TK;
  const int b_off = TM * TK + (wn * 64 + (lane & 15)) * TK;
  const int sa_off = (wm * 128 + (lane & 15)) * 4 + (lane >> 4);
  const int sb_off = (TM + wn * 64 + (lane & 15)) * 4 + (lane >> 4);

  if (nkt > 0) issue(0, 0);
  if (nkt > 1) issue(1, 1);
  for (int kt = 0; kt < nkt; ++kt) {
    const int s = kt & 1;
    if (kt + 1 < nkt)
      asm volatile("s_waitcnt vmcnt(9)" ::: "memory");  // tile kt has landed; kt + 1 may be in flight
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    raw_barrier();  // every wave's copies of tile kt are in LDS
    const char* st = smem + s * STAGE;
    const uint8_t* sc = reinterpret_cast<const uint8_t*>(smem + 2 * STAGE + s * SCALES);
    i32x8 fb[4];
    int xb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const char* p = st + b_off + j * 16 * TK;
      const int4 lo = *reinterpret_cast<const int4*>(p + sw0);
      const int4 hi = *reinterpret_cast<const int4*>(p + sw1);
      fb[j] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      xb[j] = sc[sb_off + j * 64];
    }
#pragma unroll
    for (int mh = 0; mh < 2; ++mh) {
      i32x8 fa[4];
      int xa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* p = st + a_off + (4 * mh + i) * 16 * TK;
        const int4 lo = *reinterpret_cast<const int4*>(p + sw0);
        const int4 hi = *reinterpret_cast<const int4*>(p + sw1);
        fa[i] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        xa[i] = sc[sa_off + (4 * mh + i) * 64];
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)  // C^T tile: lane ends with 4 consecutive n of one m
          acc[4 * mh + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[4 * mh + i][j], 0,
                                                                                0, 0, xb[j], 0, xa[i]);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of stage s retired
    raw_barrier();                                       // every wave is done reading stage s
    if (kt + 2 < nkt) issue(kt + 2, s);                  // lands while tile kt + 1 computes
  }

  // ---------------- epilogue: lane holds C[m][n..n+3], m = m0 + wm*128 + 16i + (lane&15),
  //                  n = n0 + wn*64 + 16j + 4*(lane>>4)
  const int mrow = m0 + wm * 128 + (lane & 15);
  const int ncol = n0 + wn * 64 + 4 * (lane >> 4);
  if constexpr (MXOUT)
    gemm256_store_mx(acc, ep, M, N, mrow, ncol, smem + wave * 16384);
  else
    gemm256_store<false, false>(acc, ep, M, N, split, 0, mrow, ncol, 1.f, smem + wave * 16384);
}

}  // namespace

int gemm_mxfp8_256(const uint8_t* A, const uint8_t* sa, const uint8_t* B, const uint8_t* sb, int M, int N, int Kbytes,
                   const GemmEpilogue& ep, int splits, hipStream_t s) {
  const int tiles_m = (M + TM - 1) / TM, tiles_n = (N + TN - 1) / TN;
  const bool mxout = ep.mx_q != nullptr;
  if (mxout && ep.mode != GemmEpilogue::kStore) return 0;
  splits = mxout ? 1 : std::max(1, splits);
  int kps = (Kbytes + splits - 1) / splits;
  kps = (kps + TK - 1) / TK * TK;
  splits = (Kbytes + kps - 1) / kps;
  GemmEpilogue e2 = ep;
  e2.store_mode = 1;  // bf16 output: 16-B stores after a lane exchange, as the per-tensor e4m3 kernel
  e2.store_rot = true;
  e2.store_cache = gemm_store_cache();
  const dim3 grid(tiles_m * tiles_n, splits);
  if (mxout)
    gemm_mxfp8_256_kernel<true><<<grid, 512, 0, s>>>(A, sa, B, sb, e2, M, N, Kbytes, tiles_m, tiles_n, kps);
  else
    gemm_mxfp8_256_kernel<false><<<grid, 512, 0, s>>>(A, sa, B, sb, e2, M, N, Kbytes, tiles_m, tiles_n, kps);
  return splits;
}

}  // namespace kern
}  // namespace ringdp
