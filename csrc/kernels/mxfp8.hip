// MXFP8 quantiser (OCP microscaling): e4m3 elements with one E8M0 scale per block of 32, computed from the
// data in the pass that quantises it - no amax history, no roll, no state between calls.
//
//   x[R][C] (bf16, or fp32 rounded to bf16 on load), C % 32 == 0, one read, either or both of
//     row-wise     q [R][Cp] e4m3, s [R][Cp/32] E8M0   blocks of 32 along a row of x
//     column-wise  qt[C][Rp] e4m3, st[C][Rp/32] E8M0   blocks of 32 along a column of x, stored transposed
//   Cp / Rp = C / R rounded up to 128: padding elements are 0 and all-padding blocks have scale byte 127, so
//   the GEMM (gemm_mxfp8_256.hip) only ever sees whole 128-byte k-steps.
//
// Scale rule, per block with amax a > 0: e = the smallest integer with a * 2^-e <= 448, clamped to
// [-127, 127]; scale byte e + 127; elements cvt_e4m3(x * 2^-e), round to nearest even.  448 = 1.75 * 2^8, so
// with a = m * 2^p (1 <= m < 2) e = p - 8 when m <= 1.75 and p - 7 otherwise: integer arithmetic on the
// float's exponent and mantissa fields.  x * 2^-e is exact (v_ldexp_f32), so nothing saturates except under
// the clamp.  An all-zero block gets byte 127; byte 255 (NaN) is never written.
//
// Work split: a 256-thread workgroup owns a 128 x 128 tile.  A lane loads 16 consecutive values of a row
// (32 B of bf16), so a row block is two lanes: in-lane max, one cross-lane step, and the row-wise bytes leave
// straight from registers as one 16-B store per lane (8 lanes = one 128-B line); the four scale bytes of a
// row's 128 columns are gathered into one dword store.  For the column-wise output the tile is also written
// to LDS as bf16 [128][128] (32 KiB, 16-B writes); after one barrier lane l of a wave reads column 64 h + l
// down the rows (64 lanes = 32 consecutive dwords: no bank conflict, no padding) - a whole 32-row block per
// lane, so its amax needs no cross-lane step and the transposed bytes leave as two 16-B stores; a lane owns
// two vertically adjacent blocks and writes their scales as one 16-bit store.
#include "device_common.h"
#include "kernels.h"
#include "mx_device.h"

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

constexpr int kT = 128;  // tile edge

__device__ __forceinline__ void load16(const bf16* p, bf16x8& a, bf16x8& b) {
  a = *reinterpret_cast<const bf16x8*>(p);
  b = *reinterpret_cast<const bf16x8*>(p + 8);
}
__device__ __forceinline__ void load16(const float* p, bf16x8& a, bf16x8& b) {  // fp32 masters: their bf16 rounding
  const float4* f = reinterpret_cast<const float4*>(p);
  const float4 v0 = f[0], v1 = f[1], v2 = f[2], v3 = f[3];
  a = bf16x8{(bf16)v0.x, (bf16)v0.y, (bf16)v0.z, (bf16)v0.w, (bf16)v1.x, (bf16)v1.y, (bf16)v1.z, (bf16)v1.w};
  b = bf16x8{(bf16)v2.x, (bf16)v2.y, (bf16)v2.z, (bf16)v2.w, (bf16)v3.x, (bf16)v3.y, (bf16)v3.z, (bf16)v3.w};
}

// One 128 x 128 tile (br, bc); q / qt null: that orientation is not wanted (uniform over the launch or entry).
template <typename X>
__device__ __forceinline__ void mx_tile(const X* __restrict__ x, int64_t R, int64_t C, uint8_t* __restrict__ q,
                                        uint8_t* __restrict__ s, uint8_t* __restrict__ qt,
                                        uint8_t* __restrict__ st, int br, int bc) {
  __shared__ __attribute__((aligned(16))) bf16 tile[kT * kT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t Cp = (C + kT - 1) / kT * kT, Rp = (R + kT - 1) / kT * kT;
  const int cl = (tid & 7) * 16;
  const int64_t gc = (int64_t)bc * kT + cl;
  bf16x8 v[4][2];
#pragma unroll
  for (int p = 0; p < 4; ++p) {  // all loads first
    const int64_t gr = (int64_t)br * kT + p * 32 + (tid >> 3);
    v[p][0] = zero_bf16x8();
    v[p][1] = zero_bf16x8();
    if (gr < R && gc < C) load16(x + gr * C + gc, v[p][0], v[p][1]);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int rl = p * 32 + (tid >> 3);
    const int64_t gr = (int64_t)br * kT + rl;
    if (qt) {
      *reinterpret_cast<bf16x8*>(tile + rl * kT + cl) = v[p][0];
      *reinterpret_cast<bf16x8*>(tile + rl * kT + cl + 8) = v[p][1];
    }
    if (q) {
      float f[16];
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        f[j] = (float)v[p][j >> 3][j & 7];
        a = fmaxf(a, fabsf(f[j]));
      }
      a = fmaxf(a, __shfl_xor(a, 1, 64));  // the other half of this 32-value row block
      const int e = mx_exp(a);
      const uint4 w = make_uint4(mx_pack4(f[0], f[1], f[2], f[3], e), mx_pack4(f[4], f[5], f[6], f[7], e),
                                 mx_pack4(f[8], f[9], f[10], f[11], e), mx_pack4(f[12], f[13], f[14], f[15], e));
      // the row's four scale bytes (lanes 0 / 2 / 4 / 6 of its 8) into one dword on the first lane
      const unsigned sb = (unsigned)(e + 127);
      const int l0 = lane & ~7;
      const unsigned s4 = sb | (__shfl(sb, l0 + 2, 64) << 8) | (__shfl(sb, l0 + 4, 64) << 16) |
                          (__shfl(sb, l0 + 6, 64) << 24);
      if (gr < R) {
        *reinterpret_cast<uint4*>(q + gr * Cp + gc) = w;
        if ((tid & 7) == 0) *reinterpret_cast<unsigned*>(s + gr * (Cp / 32) + bc * 4) = s4;
      }
    }
  }
  if (!qt) return;
  __syncthreads();
  const int c = (wave & 1) * 64 + lane, rb0 = (wave >> 1) * 2;
  const int64_t gc2 = (int64_t)bc * kT + c;
  if (gc2 >= C) return;
  unsigned sc2 = 0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int r0 = (rb0 + b) * 32;
    float f[32];
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      f[i] = (float)tile[(r0 + i) * kT + c];
      a = fmaxf(a, fabsf(f[i]));
    }
    const int e = mx_exp(a);
    unsigned w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = mx_pack4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3], e);
    uint8_t* dst = qt + gc2 * Rp + (int64_t)br * kT + r0;
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4*>(dst + 16) = make_uint4(w[4], w[5], w[6], w[7]);
    sc2 |= (unsigned)(e + 127) << (8 * b);
  }
  *reinterpret_cast<unsigned short*>(st + gc2 * (Rp / 32) + br * 4 + rb0) = (unsigned short)sc2;
}

template <typename X>
__global__ __launch_bounds__(256) void mx_quant_kernel(const X* __restrict__ x, int64_t R, int64_t C,
                                                       uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                                                       uint8_t* __restrict__ qt, uint8_t* __restrict__ st,
                                                       int tiles_c) {
  const int br = blockIdx.x / tiles_c, bc = blockIdx.x - br * tiles_c;
  mx_tile(x, R, C, q, s, qt, st, br, bc);
}

// many fp32 matrices (a model's weights), both orientations, in one launch: entry i covers blocks
// [tile0, next entry's tile0)
__global__ __launch_bounds__(256) void mx_quant_multi_kernel(MxQuantTable tab) {
  __shared__ MxQuantEntry se[kMxQuantMax];
#pragma unroll
  for (int i = 0; i < kMxQuantMax; ++i)
    if (threadIdx.x == i && i < tab.n) se[i] = tab.e[i];
  __syncthreads();
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= se[i + 1].tile0) ++i;
  const MxQuantEntry& e = se[i];
  const int tiles_c = (int)((e.cols + kT - 1) / kT);
  const int l = (int)blockIdx.x - e.tile0, br = l / tiles_c, bc = l - br * tiles_c;
  mx_tile(e.src, e.rows, e.cols, e.q, e.s, e.qt, e.st, br, bc);
}

}  // namespace

int64_t mx_pad(int64_t n) { return (n + kT - 1) / kT * kT; }
int64_t mx_quant_tiles(int64_t rows, int64_t cols) { return (mx_pad(rows) / kT) * (mx_pad(cols) / kT); }

void mx_quantize(const void* x, bool x_f32, int64_t rows, int64_t cols, uint8_t* q, uint8_t* s, uint8_t* qt,
                 uint8_t* st, hipStream_t stream) {
  const int tiles_c = (int)(mx_pad(cols) / kT);
  const int blocks = (int)mx_quant_tiles(rows, cols);
  if (blocks <= 0) return;
  if (x_f32)
    mx_quant_kernel<float><<<blocks, 256, 0, stream>>>(static_cast<const float*>(x), rows, cols, q, s, qt, st, tiles_c);
  else
    mx_quant_kernel<bf16><<<blocks, 256, 0, stream>>>(static_cast<const bf16*>(x), rows, cols, q, s, qt, st, tiles_c);
}

void mx_quantize_multi(const MxQuantTable& t, hipStream_t stream) {
  if (t.n > 0 && t.total_tiles > 0) mx_quant_multi_kernel<<<t.total_tiles, 256, 0, stream>>>(t);
}

}  // namespace kern
}  // namespace ringdp
