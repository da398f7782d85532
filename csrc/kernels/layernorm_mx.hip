// LayerNorm forward that writes its output as MXFP8 (e4m3 elements, one E8M0 scale per block of 32, see
// mxfp8.hip) for the next MXFP8 linear instead of bf16: the normalised rows never reach memory and mx_quantize
// does not read them back.
//
//   x [rows][D] bf16, w / b fp32, D % 32 == 0, 32 <= D <= 2048, any rows >= 1
//     stats [rows][2]                                   mean, rstd
//     row-wise     q [rows][Cp] e4m3, s [rows][Cp/32]   blocks of 32 along a row
//     column-wise  qt[D][Rp]    e4m3, st[D][Rp/32]      blocks of 32 along a column, stored transposed (optional)
//   Cp / Rp = D / rows rounded up to 128.  Every byte, padding included (zero elements, scale byte 127), is the
//   byte mx_quantize writes for layernorm_fwd's bf16 output, and stats is layernorm_fwd's bit for bit.
//
// For that the statistics keep layernorm_fwd_kernel's per-lane element assignment (8-element vectors at
// lane + 64 i), its summation order and wave_sum, and the arithmetic is spelled out in the form vit.hip's ISA
// has - the squares of the variance rounded before they are added, (v - mean) * rstd rounded and then one fma
// with w and b - under `fp contract(off)`, so that this unit's flags (no packed fp32 ops, unlike vit.hip)
// cannot make the compiler contract it differently.
//
// Work split: a 512-thread workgroup owns a band of 32 rows (one column block high) and all D columns; its 8
// waves take the rows round-robin, one wave per row, the next row's load in flight while this one is reduced.
//   row-wise     A lane holds 8 consecutive normalised values, so a 32-block is 4 adjacent lanes of one vector
//                index: in-lane max, two cross-lane steps, mx_exp, two mx_pack4 and one 8-B store straight from
//                registers; the scale bytes of 16 lanes (128 columns) are gathered into one dword store.  The
//                lanes past D (up to Cp) hold zeros and write the column padding the same way.
//   column-wise  Each row's bf16 values also go to an LDS image [32][D] (16-B writes).  After one barrier a
//                thread owns a column and reads it down the 32 rows (64 lanes = 32 consecutive dwords: no bank
//                conflict) - a whole block per lane, so its amax needs no cross-lane step - and writes the
//                transposed bytes as two 16-B stores and the scale as a byte.  One block's 32 values are live
//                at a time (the fence at the end of the column loop keeps the compiler from hoisting the next
//                block's LDS reads over the stores).
// The image is not padded: the row writes are consecutive 16-B pieces of one wave and the column reads are
// consecutive 2-B pieces, conflict-free at any row pitch, and at D = 768 the unpadded 48 KiB lets three
// workgroups share a CU's 160 KiB.  A band's 32-B pieces of qt share their 128-B lines with the three
// neighbouring bands, so band ids are remapped (xcd_remap) to keep neighbours on one XCD, whose L2 merges them.
// Bands wholly beyond `rows` (up to Rp) load nothing and write only zero qt bytes and 127 scale bytes.  With
// qt null there is no LDS image, no barrier and no padding band.
// No atomics, no fences, no state between calls: every output byte has one writer.
#include "device_common.h"
#include "kernels.h"
#include "mx_device.h"

#pragma clang fp contract(off)

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

constexpr int kBand = 32;                    // rows of a workgroup: one column block
constexpr int kLnMxThreads = 512;            // 8 waves x 4 rows
constexpr int kLnMxWaves = kLnMxThreads / 64;

template <int VPL>
__device__ __forceinline__ void ln_mx_load(const bf16* __restrict__ x, int64_t row, int64_t rows, int D, int lane,
                                           bf16x8 (&t)[VPL]) {
  const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + row * D);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + 64 * i;
    t[i] = zero_bf16x8();
    if (row < rows && vi < D / 8) t[i] = xr[vi];
  }
}

// 8-element vectors per lane; column-wise output wanted.  VPL <= 2 (D <= 1024, an image of at most 64 KiB): 6 waves
// per SIMD, i.e. registers for the three workgroups per CU that the image at D = 768 leaves room for
template <int VPL, bool COL>
__global__ __launch_bounds__(kLnMxThreads, VPL <= 2 ? 6 : 2) void layernorm_fwd_mx_kernel(
    const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int64_t rows, int D,
    float eps, float* __restrict__ stats, uint8_t* __restrict__ q, uint8_t* __restrict__ s, uint8_t* __restrict__ qt,
    uint8_t* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) bf16 ln_mx_img[];  // [kBand][D], COL only
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int band = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int64_t r0 = (int64_t)band * kBand;
  const int nv = D / 8, Cp = (D + 127) / 128 * 128;
  const int64_t Rp = (rows + 127) / 128 * 128;

  if (r0 >= rows) {  // a band of row padding (COL launches only)
    if (COL) {
      for (int c = threadIdx.x; c < D; c += kLnMxThreads) {
        uint4* dst = reinterpret_cast<uint4*>(qt + c * Rp + r0);
        dst[0] = make_uint4(0u, 0u, 0u, 0u);
        dst[1] = make_uint4(0u, 0u, 0u, 0u);
        st[c * (Rp / 32) + band] = 127;
      }
    }
    return;
  }

  bf16x8 t[VPL];
  ln_mx_load<VPL>(x, r0 + wave, rows, D, lane, t);
  for (int rl = wave; rl < kBand; rl += kLnMxWaves) {
    const int64_t row = r0 + rl;
    bf16x8 tn[VPL];  // this wave's next row (none after its last: `rows` loads nothing)
    ln_mx_load<VPL>(x, rl + kLnMxWaves < kBand ? row + kLnMxWaves : rows, rows, D, lane, tn);
    if (row < rows) {
      float v[VPL][8];
      float sm = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        if (lane + 64 * i < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            v[i][j] = (float)t[i][j];
            sm += v[i][j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
        }
      }
      const float mean = wave_sum(sm) / (float)D;
      float qq = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < nv)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = v[i][j] - mean;
            const float d2 = d * d;  // rounded, then added: layernorm_fwd_kernel's ISA
            qq += d2;
          }
      const float rstd = rsqrtf(wave_sum(qq) / (float)D + eps);
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        // (opaque per row: otherwise the lane's w / b / q / s addresses are hoisted out of the row loop as
        // 64-bit pairs, and VPL 2 spills four of them at 80 VGPRs)
        int vi = lane + 64 * i;
        asm volatile("" : "+v"(vi));
        bf16x8 o = zero_bf16x8();  // lanes past D: the column padding of q
        if (vi < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int c = vi * 8 + j;
            const float n = (v[i][j] - mean) * rstd;
            o[j] = (bf16)__builtin_fmaf(n, w[c], b[c]);  // layernorm_fwd_kernel's value
          }
          if (COL) *reinterpret_cast<bf16x8*>(ln_mx_img + rl * D + vi * 8) = o;
        }
        float f[8];
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f[j] = (float)o[j];
          a = fmaxf(a, fabsf(f[j]));
        }
        a = fmaxf(a, __shfl_xor(a, 1, 64));  // the other three lanes of this 32-value block
        a = fmaxf(a, __shfl_xor(a, 2, 64));
        const int e = mx_exp(a);
        const unsigned lo = mx_pack4(f[0], f[1], f[2], f[3], e), hi = mx_pack4(f[4], f[5], f[6], f[7], e);
        // the four scale bytes of 128 columns (lanes 0 / 4 / 8 / 12 of 16) into one dword on the first lane
        const unsigned sb = (unsigned)(e + 127);
        const int l0 = lane & ~15;
        const unsigned s4 = sb | (__shfl(sb, l0 + 4, 64) << 8) | (__shfl(sb, l0 + 8, 64) << 16) |
                            (__shfl(sb, l0 + 12, 64) << 24);
        if (vi * 8 < Cp) {
          *reinterpret_cast<uint2*>(q + row * Cp + vi * 8) = make_uint2(lo, hi);
          if ((lane & 15) == 0) *reinterpret_cast<unsigned*>(s + row * (Cp / 32) + vi / 4) = s4;
        }
        asm volatile("" ::: "memory");  // one vector's w / b live at a time (VPL 2 fits 80 VGPRs without scratch)
      }
      if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
      }
    } else if (COL) {  // row padding inside the last band: zeros for the column walk
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int vi = lane + 64 * i;
        if (vi < nv) *reinterpret_cast<bf16x8*>(ln_mx_img + rl * D + vi * 8) = zero_bf16x8();
      }
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) t[i] = tn[i];
  }
  if (!COL) return;
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += kLnMxThreads) {
    float f[32];
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      f[i] = (float)ln_mx_img[i * D + c];
      a = fmaxf(a, fabsf(f[i]));
    }
    const int e = mx_exp(a);
    unsigned p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = mx_pack4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3], e);
    uint4* dst = reinterpret_cast<uint4*>(qt + c * Rp + r0);
    dst[0] = make_uint4(p[0], p[1], p[2], p[3]);
    dst[1] = make_uint4(p[4], p[5], p[6], p[7]);
    st[c * (Rp / 32) + band] = (uint8_t)(e + 127);
    asm volatile("" ::: "memory");  // one block's values live at a time
  }
}

template <int VPL>
void ln_mx_launch(const bf16* x, const float* w, const float* b, int64_t rows, int D, float eps, float* stats,
                  uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, hipStream_t stream) {
  if (qt) {
    const int bands = (int)(mx_pad(rows) / kBand);
    const size_t lds = (size_t)kBand * D * sizeof(bf16);
    layernorm_fwd_mx_kernel<VPL, true><<<bands, kLnMxThreads, lds, stream>>>(x, w, b, rows, D, eps, stats, q, s, qt, st);
  } else {
    const int bands = (int)((rows + kBand - 1) / kBand);
    layernorm_fwd_mx_kernel<VPL, false><<<bands, kLnMxThreads, 0, stream>>>(x, w, b, rows, D, eps, stats, q, s, nullptr,
                                                                            nullptr);
  }
}

}  // namespace

void layernorm_fwd_mx(const void* x, const float* w, const float* b, int64_t rows, int D, float eps, float* stats,
                      uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, hipStream_t stream) {
  if (rows <= 0) return;
  const bf16* xb = static_cast<const bf16*>(x);
  const int nv = D / 8;
  if (nv <= 64)
    ln_mx_launch<1>(xb, w, b, rows, D, eps, stats, q, s, qt, st, stream);
  else if (nv <= 128)
    ln_mx_launch<2>(xb, w, b, rows, D, eps, stats, q, s, qt, st, stream);
  else
    ln_mx_launch<4>(xb, w, b, rows, D, eps, stats, q, s, qt, st, stream);
}

}  // namespace kern
}  // namespace ringdp
