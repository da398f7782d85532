// bf16 ConvNet (design: convnet_fwd.hip): what more than one of its units (convnet_fwd.hip, convnet_bwd12.hip,
// convnet_bwd3.hip) uses on the device - the packed-weight layout, the LDS-DMA copies, the a2 and conv1 input
// staging, the sparse MFMA's wrapper, the a1 / pool1-code image sizes and the phase-stamp macro.
#pragma once

#include "device_common.h"

namespace ringdp::kern {
using namespace ringdp::dev;
namespace {

// ------------------------------------------------------------------ packed weight layout
// bf16 element offsets inside the packed buffer.  Fragment order: [n-tile][k-step][lane][8].
constexpr int P1_OFF = 0, P1_N = 2 * 2 * 512;                   // conv1 fwd   (K = kh*8 + kw, 2 k-steps)
constexpr int P2F_OFF = P1_OFF + P1_N, P2F_N = 4 * 9 * 512;     // conv2 fwd   (N 64, K 288)
constexpr int P3F_OFF = P2F_OFF + P2F_N, P3F_N = 8 * 18 * 512;  // conv3 fwd   (N 128, K 576)
constexpr int P2D_OFF = P3F_OFF + P3F_N, P2D_N = 2 * 18 * 512;  // conv2 dgrad (N 32, K 576)
constexpr int P3D_OFF = P2D_OFF + P2D_N, P3D_N = 4 * 36 * 512;  // conv3 dgrad (N 64, K 1152)
constexpr int PFC_OFF = P3D_OFF + P3D_N, PFC_N = 16 * 128 * 10; // fc1 [window][co][n] (backward)
constexpr int PFF_OFF = PFC_OFF + PFC_N, PFF_N = 64 * 64 * 8;    // fc1 fwd B fragments, k = w*128 + co
constexpr int PACK_TOTAL = PFF_OFF + PFF_N;

// window-ordered GEMM row r = 4*window + i of a pooled (2x2/s2) 8x8 map -> spatial y*pw + x
__device__ __forceinline__ int win_pos(int r, int pw) {
  const int w = r >> 2, i = r & 3;
  return (2 * (w >> 2) + (i >> 1)) * pw + 2 * (w & 3) + (i & 1);
}

// Async global -> LDS copy of 16 B per lane (global_load_lds_dwordx4): the LDS destination is the
// wave-uniform base + lane * 16, so the image it fills is lane-linear (no padding inside a wave's 1 KiB).
// Issued from inline asm.  With __builtin_amdgcn_global_load_lds the compiler sees an LDS write on the VM counter
// and drains it (s_waitcnt vmcnt(0)) before the next LDS read, however unrelated - the prefetch then never
// overlaps the compute it was issued ahead of (seen in the ISA of conv1_wgrad / conv3_fwd).  Here the copy
// is invisible to the compiler: the consumer must `s_waitcnt vmcnt(0)` itself before the barrier that
// publishes the buffer (c_dma_wait).  M0 is set inside the asm; no kernel using this sets M0 otherwise
// (the ISA of these kernels has no other M0 writer: checked when this was introduced).
__device__ __forceinline__ void glds16_async(const void* gsrc, void* lds_wave_base) {
  const unsigned base = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)((__attribute__((address_space(3))) char*)(lds_wave_base)));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(base), "v"(gsrc) : "memory");
}
__device__ __forceinline__ void c_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the same with the wave's N newest vector-memory operations (stores issued after its DMAs) left in flight
template <int N>
__device__ __forceinline__ void c_dma_wait_but() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The same copy from a wave-uniform base (SGPR pair) plus a 32-bit per-lane byte offset: the per-lane part of
// an image's copy is the same for every image, so it is computed once and no 64-bit address math runs per copy.
__device__ __forceinline__ void glds16_sv(const void* sbase, uint32_t voff, void* lds_wave_base) {
  const unsigned base = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)((__attribute__((address_space(3))) char*)(lds_wave_base)));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(base), "v"(voff), "s"(sbase)
               : "memory");
}

// barrier for LDS hand-offs: this wave's LDS operations drained, global stores left in flight (the release
// fence of __syncthreads() would also wait for those)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// v_smfmac_f32_16x16x64_bf16, D[16 x 16] += A[16 x 64, 2:4 sparse] * B[64 x 16], as measured on gfx950 by
// tools/smfmac_probe.hip (profiles/r10/c3_wgrad_sparse/probe.md); it issues at the dense 16x16x32's rate.
//   A (8 bf16 per lane): lane l holds row l % 16.  Slots 2r, 2r+1 are the two kept values of the four dense
//     columns k = 16 (l / 16) + 4r .. + 3, r = 0..3.
//   index VGPR of the same lane: bits [2e+1 : 2e] = which of its four columns slot e stands for.  abid = 0 takes
//     these 16 bits from the low half of the register, abid = 1 from the high half; cbsz is ignored.  The two
//     indices of a group need not be ascending or distinct: every slot is simply multiplied with the B row it
//     names (all 16 pairs checked), so one live value per group goes in slot 2r whatever its position, with a
//     zero in slot 2r+1.
//   B (16 bf16 per lane): lane l holds column l % 16; slots 0-7 are rows k = 8 (l / 16) + s, slots 8-15 rows
//     32 + 8 (l / 16) + (s - 8): the B fragments of two consecutive dense 16x16x32 k-steps, back to back.
//   D: as the dense instruction (lane l: column l % 16, rows 4 (l / 16) .. + 3).
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x4 smfmac16x16x64(const bf16x8& a, const bf16x16& b, const f32x4& c, int idx) {
  return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, c, idx, 0, 0);
}

constexpr int C3_XRS = 72;  // bf16 per padded LDS row of a2 (backward wgrad role)

// a2 image -> LDS staging buffer R (lane-linear 16-B chunks, LDS-DMA: no VGPRs, lands while the
// previous image computes); nthreads threads issue the 13 wave-instructions (the last half full).
__device__ __forceinline__ void a2_glds(const bf16* __restrict__ a2, int b, bf16* R, int wave, int lane,
                                        int nwaves) {
  const bf16* src = a2 + (int64_t)b * 6400;
  for (int k = wave; k < 13; k += nwaves) {
    const int slot = k * 64 + lane;
    if (slot < 800) glds16_async(src + slot * 8, R + k * 512);
  }
}

// staging buffer -> padded MFMA rows (RS elements per row, C3_XRS by default): the padding keeps the 16
// rows of a fragment read on distinct banks, which a lane-linear DMA image cannot have
template <int RS = C3_XRS>
__device__ __forceinline__ void a2_relayout(const bf16* R, bf16* X, int tid, int nthreads) {
  for (int c = tid; c < 800; c += nthreads)
    *reinterpret_cast<bf16x8*>(X + (c >> 3) * RS + (c & 7) * 8) = reinterpret_cast<const bf16x8*>(R)[c];
}

// ------------------------------------------------------------------ conv1 input staging (forward and conv1 wgrad)
// The zero-ringed 30x30 input is staged as 8 copies shifted by s = 0..7 columns (rows of 32):
// copy s holds xpad[r][c + s].  Eight consecutive pixels xpad[r][ow .. ow+7] are then ONE aligned
// ds_read_b128 at copy (ow & 7), column (ow & ~7) - this is the im2col of a 5-wide filter row, so
// the GEMM K is laid out as k = kh*8 + kw (kw < 5 valid): 2 k-steps of 32, no per-element gather.
constexpr int XC_W = 32, XC_SZ = 30 * XC_W;  // one shifted copy (bf16)

template <bool U8>
__device__ __forceinline__ void c1_load(const void* xin, int b, int tid, uint32_t& u, float4& f) {
  if (tid < 196) {
    if (U8)
      u = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(xin) + (int64_t)b * 784)[tid];
    else
      f = reinterpret_cast<const float4*>(static_cast<const float*>(xin) + (int64_t)b * 784)[tid];
  }
}

// Normalise this thread's 4 pixels (one row segment: columns pc0 .. pc0+3, pc0 = 4*(tid%7) + 1) and
// write them into copies 0..NC-1.  pc0 = 1 (mod 4), so each copy's alignment is known at compile time:
// one ds_write_b64 (s = 1 mod 4), two b32 (s = 3 mod 4) or b16 + b32 + b16 - instead of 4 b16 per copy.
// A segment starting at pc0 = 1 writes columns 1-s .. < 0 of copy s "before" its row, i.e. into columns
// 33-s+k of the previous row: those are only ever read as filter columns kw >= 5 (zero weights in the
// forward, zero dC rows >= 26 in wgrad), so the spill is harmless and the zero ring (copy column 29-s,
// column 0 of copy 0, rows 0/29) is never written.
template <bool U8, int NC, int RS = XC_W, int CS = XC_SZ>
__device__ __forceinline__ void c1_store(bf16* xc, int tid, uint32_t u, float4 f, float mean, float inv_std,
                                         float in_scale) {
  if (tid < 196) {
    float v[4];
    if (U8) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (float)((u >> (8 * k)) & 0xff) * in_scale;
    } else {
      v[0] = f.x;
      v[1] = f.y;
      v[2] = f.z;
      v[3] = f.w;
    }
    bf16 xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = (bf16)((v[k] - mean) * inv_std);
    const uint32_t lo16 = __builtin_bit_cast(uint16_t, xv[0]), m1 = __builtin_bit_cast(uint16_t, xv[1]),
                   m2 = __builtin_bit_cast(uint16_t, xv[2]), hi16 = __builtin_bit_cast(uint16_t, xv[3]);
    const uint32_t p01 = lo16 | (m1 << 16), p23 = m2 | (hi16 << 16), p12 = m1 | (m2 << 16);
    const int pr = tid / 7 + 1, pc0 = 4 * (tid % 7) + 1;
#pragma unroll
    for (int s = 0; s < NC; ++s) {
      bf16* d = xc + s * CS + pr * RS + pc0 - s;  // may point before the row (see above)
      if ((s & 3) == 1) {
        *reinterpret_cast<uint2*>(d) = make_uint2(p01, p23);
      } else if ((s & 3) == 3) {
        reinterpret_cast<uint32_t*>(d)[0] = p01;
        reinterpret_cast<uint32_t*>(d)[1] = p23;
      } else {
        d[0] = xv[0];
        *reinterpret_cast<uint32_t*>(d + 1) = p12;
        d[3] = xv[3];
      }
    }
  }
}

// conv1 pool/ReLU codes for the backward: [B][py 13][co/2 16][px 16] bytes (px 13..15 zero), one nibble per
// channel (low: even co, high: odd co), each 1 << argmax (dy*2+dx) if the pooled value is > 0, else 0 (the
// gradient's destination, one-hot).  Window rows per channel pair let conv1 wgrad read the codes of 4
// neighbouring windows of one channel as one 4-byte load.  (Nibbles, not bytes: conv1 forward is bound by
// its HBM writes, 17.4 -> 14.1 KB per image.)
constexpr int C1I_IMG = 13 * 256;      // 3328 bytes per image
constexpr int C1A_IMG = 169 * 32;      // a1 elements per image
constexpr int C2_XRS = 48;  // bf16 per LDS row of the a1 image (32 + 16 pad): 96-B rows, see c2f_tile_pos

// Phase stamps of the diagnostic builds (FF_ST / C3_ST / C12_ST, each enabled by its own -DRINGDP_*_STAMPS and
// empty otherwise): lane 0 of every wave records s_memtime at phase point k of step s, for the 8 steps from s0,
// as [wave][step][slots] 8-byte words in the kernel's LDS array `smem` past its lds_end bytes.
#define CN_STAMP(lds_end, s0, slots, s, k)                                                                         \
  do {                                                                                                             \
    if ((s) >= (s0) && (s) < (s0) + 8 && (threadIdx.x & 63) == 0)                                                  \
      reinterpret_cast<unsigned long long*>(smem + (lds_end))[((threadIdx.x >> 6) * 8 + ((s) - (s0))) * (slots) + (k)] = \
          __builtin_amdgcn_s_memtime();                                                                            \
  } while (0)

}  // namespace
}  // namespace ringdp::kern
