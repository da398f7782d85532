// Shared pieces of the fused attention kernels (head dim 64): the strided operand views, the LDS swizzles and
// the column-sum epilogue.  Used by vit.hip (Tp <= 256: all of K and V of a head in LDS) and by
// vit_attn_long.hip (any length: key-blocked).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

constexpr int ATT_D = 64;
// Strided view of one attention operand: element (b, h, t, d) at base + b*sb + h*sh + t*st + d - either
// head-major [B*H][Tp][64] (sb = Tp*64, sh = 0 with H = 1 per "batch" bh) or the token rows of the qkv
// projection [B*T][3*H*64] (sb = T*st, sh = 64, st = 3*H*64), which the kernels then read directly
// (no split/merge passes).  Rows t >= T read as zero.
struct AttnIn {
  const bf16* base;
  int64_t sb, sh, st;
  __device__ __forceinline__ const bf16* row(int bh, int H, int t) const {
    return base + (int64_t)(bh / H) * sb + (int64_t)(bh % H) * sh + (int64_t)t * st;
  }
  __device__ __forceinline__ bf16x8 load8(int bh, int H, int t, int T, int d) const {
    return t < T ? *reinterpret_cast<const bf16x8*>(row(bh, H, t) + d) : zero_bf16x8();
  }
};
struct AttnOut {
  bf16* base;
  int64_t sb, sh, st;
  int rows;  // rows t < rows are written (T for token rows, Tp for head-major)
  __device__ __forceinline__ bf16* row(int bh, int H, int t) const {
    return base + (int64_t)(bh / H) * sb + (int64_t)(bh % H) * sh + (int64_t)t * st;
  }
};
__device__ __forceinline__ int att_ksw(int r, int d) { return r * ATT_D + ((((d >> 3) ^ (r & 7))) << 3) + (d & 7); }
__device__ __forceinline__ int att_vsw(int r, int d) {
  return r * ATT_D + ((((d >> 4) ^ ((r >> 1) & 3))) << 4) + (d & 15);
}

// Column sums of a kernel's 64-wide output block (a bias gradient's partial): lane (g, i) holds sums for columns
// 16 dt + 4g + e; reduced over the 16 lanes of each g, then over the 4 waves through `scratch` (>= 1 KiB of the
// kernel's LDS, free once its main loop is done - the caller has passed a barrier), and stored as 64 floats.
__device__ __forceinline__ void attn_colsum_store(float (&cs)[4][4], float* scratch, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = cs[dt][e];
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      t += __shfl_xor(t, 8, 64);
      cs[dt][e] = t;
    }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) scratch[wave * 64 + 16 * dt + 4 * g + e] = cs[dt][e];
  }
  __syncthreads();
  if (threadIdx.x < 64)
    out[threadIdx.x] = (scratch[threadIdx.x] + scratch[64 + threadIdx.x]) + (scratch[128 + threadIdx.x] + scratch[192 + threadIdx.x]);
}

// head-major [BH][Tp][64] views (H = 1: bh is the batch index) and token-row views of a [B*T][width]
// matrix at column offset col0
inline AttnIn head_major(const void* base, int Tp) {
  return AttnIn{static_cast<const bf16*>(base), (int64_t)Tp * ATT_D, 0, ATT_D};
}
inline AttnOut head_major_out(void* base, int Tp) { return AttnOut{static_cast<bf16*>(base), (int64_t)Tp * ATT_D, 0, ATT_D, Tp}; }
inline AttnIn token_rows(const void* base, int T, int64_t width, int64_t col0) {
  return AttnIn{static_cast<const bf16*>(base) + col0, (int64_t)T * width, ATT_D, width};
}
inline AttnOut token_rows_out(void* base, int T, int64_t width, int64_t col0) {
  return AttnOut{static_cast<bf16*>(base) + col0, (int64_t)T * width, ATT_D, width, T};
}

}  // namespace kern
}  // namespace ringdp
