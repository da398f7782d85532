// LayerNorm backward that also writes its dx as MXFP8 (e4m3 elements, one E8M0 scale per block of 32, see
// mxfp8.hip) and as per-band column sums: dx is the output gradient of the MXFP8 linear in front of the LayerNorm
// (attention proj / fc2), which then needs neither mx_quantize nor colsum_f32 - two passes over dx - for its data,
// weight and bias gradients.
//
//   dy, x, dres (nullable) [rows][D] bf16, stats [rows][2], w fp32, D % 32 == 0, 32 <= D <= 2048, any rows >= 1
//     dx [rows][D] bf16                                 layernorm_bwd's dx bit for bit
//     row-wise     q [rows][Cp] e4m3, s [rows][Cp/32]   blocks of 32 along a row
//     column-wise  qt[D][Rp]    e4m3, st[D][Rp/32]      blocks of 32 along a column, stored transposed (optional)
//     cs_part [ceil(rows / 32)][D] fp32                 each band's column sums of the stored dx (with qt only)
//     part [ceil(rows / 32)][2][D] fp32                 each band's dw / db partials, for reduce_parts
//   Cp / Rp = D / rows rounded up to 128.  Every MXFP8 byte, padding included (zero elements, scale byte 127), is
//   the byte mx_quantize writes for that dx.
//
// For the bit-equal dx the row pass keeps layernorm_bwd_kernel's per-lane element assignment (8-element vectors at
// lane + 64 i), its accumulation order for s1 / s2 and wave_sum, and the arithmetic is spelled out in the form
// vit.hip's ISA has - xhat = (x - mean) * rstd and gw = g * w as rounded products, gw * xhat rounded before it is
// added to s2, then t = gw - m1, u = fma(-m2, xhat, t), dx = fma(rstd, u, dres) - under `fp contract(off)`, so
// that this unit's flags (no packed fp32 ops, unlike vit.hip) cannot make the compiler contract it differently.
//
// Work split: a 512-thread workgroup owns a band of 32 rows (one column block high) and all D columns; its 8
// waves take the rows round-robin, one wave per row, the next row's x / dy / dres in flight while this one is
// reduced.
//   row phase     m1 / m2 by wave_sum, then the lane's 8 dx values of a vector are rounded to bf16 once and go three
//                 ways from registers: the 16-B dx store, the LDS image [32][D] (column-wise only), and the row-wise
//                 MXFP8 - a 32-block is 4 adjacent lanes: in-lane max, two cross-lane steps, mx_exp, two mx_pack4,
//                 one 8-B store; the scale bytes of 16 lanes (128 columns) are gathered into one dword store.  Lanes
//                 past D (up to Cp) hold zeros and write q's column padding the same way.  dw / db of the lane's
//                 columns accumulate in registers over the wave's 4 rows.
//   column phase  After one barrier a thread owns a column and reads it down the 32 rows (a whole block per lane:
//                 no cross-lane step), writes the transposed bytes as two 16-B stores and the scale as a byte, and
//                 adds the same 32 values top-down into cs_part[band][c]: the column sums cost no pass of their
//                 own and no registers in the row phase.
//   dw / db       After the column walk and a barrier the image's 64 D bytes are reused as [8 waves][2][D] floats;
//                 a thread sums its column over the waves in a fixed order into part[band].  Without qt there is
//                 no image and the same dynamic LDS is the reduction's stage only.
// The image is not padded (see layernorm_mx.hip); band ids go through xcd_remap for the same qt line-sharing
// reason.  Rows of the last band beyond `rows` put zeros into the image; bands wholly beyond `rows` (up to Rp)
// load nothing and write only zero qt bytes and 127 scale bytes; part and cs_part have the live bands only.
// No atomics, no fences, no state between calls: every output byte has one writer.
#include "device_common.h"
#include "kernels.h"
#include "mx_device.h"

#pragma clang fp contract(off)

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

constexpr int kBand = 32;                      // rows of a workgroup: one column block
constexpr int kLnbThreads = 512;               // 8 waves x 4 rows
constexpr int kLnbWaves = kLnbThreads / 64;

// one row's operands as loaded: 3 x 16 B per vector
template <int VPL>
struct LnbRow {
  bf16x8 x[VPL], g[VPL], r[VPL];
};

template <int VPL>
__device__ __forceinline__ void lnb_load(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                         const bf16* __restrict__ dres, int64_t row, int64_t rows, int D, int lane,
                                         LnbRow<VPL>& t) {
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + 64 * i;
    t.x[i] = t.g[i] = t.r[i] = zero_bf16x8();
    if (row < rows && vi < D / 8) {
      t.x[i] = reinterpret_cast<const bf16x8*>(x + row * D)[vi];
      t.g[i] = reinterpret_cast<const bf16x8*>(dy + row * D)[vi];
      if (dres) t.r[i] = reinterpret_cast<const bf16x8*>(dres + row * D)[vi];
    }
  }
}

// VPL <= 2 (D <= 1024): 4 waves per SIMD, i.e. two workgroups per CU (128 VGPRs: two rows' packed operands and the
// dw / db accumulators are live at once); VPL 4: one workgroup, which is all its 128-KiB image leaves room for
template <int VPL, bool COL>
__global__ __launch_bounds__(kLnbThreads, VPL <= 2 ? 4 : 2) void layernorm_bwd_mx_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x, const float* __restrict__ stats,
    const float* __restrict__ w, const bf16* __restrict__ dres, int64_t rows, int D, bf16* __restrict__ dx,
    uint8_t* __restrict__ q, uint8_t* __restrict__ s, uint8_t* __restrict__ qt, uint8_t* __restrict__ st,
    float* __restrict__ cs_part, float* __restrict__ part) {
  // COL: the bf16 image [kBand][D]; then, and without COL only, the dw / db stage [kLnbWaves][2][D] floats
  extern __shared__ __attribute__((aligned(16))) unsigned char lnb_lds[];
  bf16* img = reinterpret_cast<bf16*>(lnb_lds);
  float* stage = reinterpret_cast<float*>(lnb_lds);
  // (the wave id as a scalar: the row and every row base address are then wave-uniform, and a lane's loads and
  // stores take a scalar base plus a 32-bit lane offset instead of a 64-bit address pair each)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int band = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int64_t r0 = (int64_t)band * kBand;
  // (LDS indices - img[i * D + c], stage[k * 2 * D + c] - stay below 32 * D <= 65536 and are plain ints; every
  // global index has an int64 factor)
  const int nv = D / 8, Cp = (D + 127) / 128 * 128;
  const int64_t Rp = (rows + 127) / 128 * 128;

  if (r0 >= rows) {  // a band of row padding (COL launches only)
    if (COL) {
      for (int c = threadIdx.x; c < D; c += kLnbThreads) {
        uint4* dst = reinterpret_cast<uint4*>(qt + c * Rp + r0);
        dst[0] = make_uint4(0u, 0u, 0u, 0u);
        dst[1] = make_uint4(0u, 0u, 0u, 0u);
        st[c * (Rp / 32) + band] = 127;
      }
    }
    return;
  }

  float dw[VPL][8], db[VPL][8];
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[i][j] = db[i][j] = 0.f;

  LnbRow<VPL> t;
  lnb_load<VPL>(x, dy, dres, r0 + wave, rows, D, lane, t);
#pragma unroll 1
  for (int rl = wave; rl < kBand; rl += kLnbWaves) {
    const int64_t row = r0 + rl;
    LnbRow<VPL> tn;  // this wave's next row (none after its last: `rows` loads nothing)
    lnb_load<VPL>(x, dy, dres, rl + kLnbWaves < kBand ? row + kLnbWaves : rows, rows, D, lane, tn);
    if (row < rows) {
      const float mean = stats[2 * row], rstd = stats[2 * row + 1];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        int vi = lane + 64 * i;
        asm volatile("" : "+v"(vi));  // (w is read per row, not kept in registers over the row loop)
        if (vi < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = ((float)t.x[i][j] - mean) * rstd;
            const float g = (float)t.g[i][j];
            const float gw = g * w[vi * 8 + j];
            s1 += gw;
            const float p = gw * xh;  // rounded, then added: layernorm_bwd_kernel's ISA
            s2 += p;
            dw[i][j] = __builtin_fmaf(g, xh, dw[i][j]);
            db[i][j] += g;
          }
        }
      }
      const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        // xhat and gw are made again from the packed operands (the same rounded products) instead of being kept
        // over the reduction: 8 registers per vector instead of 16.  Opaque, so that the compiler does not keep
        // them after all, nor hoist the lane's w / q / s addresses out of the row loop
        int vi = lane + 64 * i;
        asm volatile("" : "+v"(vi), "+v"(t.x[i]), "+v"(t.g[i]));
        bf16x8 o = zero_bf16x8();  // lanes past D: the column padding of q
        if (vi < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = ((float)t.x[i][j] - mean) * rstd;
            const float gw = (float)t.g[i][j] * w[vi * 8 + j];
            const float d = gw - m1;
            const float u = __builtin_fmaf(-m2, xh, d);
            o[j] = (bf16)__builtin_fmaf(rstd, u, (float)t.r[i][j]);  // layernorm_bwd_kernel's value
          }
          reinterpret_cast<bf16x8*>(dx + row * D)[vi] = o;
          if (COL) *reinterpret_cast<bf16x8*>(img + rl * D + vi * 8) = o;
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
        asm volatile("" ::: "memory");  // one vector's w live at a time
      }
    } else if (COL) {  // row padding inside the last band: zeros for the column walk
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int vi = lane + 64 * i;
        if (vi < nv) *reinterpret_cast<bf16x8*>(img + rl * D + vi * 8) = zero_bf16x8();
      }
    }
    t = tn;
  }

  if (COL) {
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += kLnbThreads) {
      float f[32];
      float a = 0.f, cs = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        f[i] = (float)img[i * D + c];
        a = fmaxf(a, fabsf(f[i]));
        cs += f[i];  // top-down, the band's rows in order
      }
      const int e = mx_exp(a);
      unsigned p[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k] = mx_pack4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3], e);
      uint4* dst = reinterpret_cast<uint4*>(qt + c * Rp + r0);
      dst[0] = make_uint4(p[0], p[1], p[2], p[3]);
      dst[1] = make_uint4(p[4], p[5], p[6], p[7]);
      st[c * (Rp / 32) + band] = (uint8_t)(e + 127);
      cs_part[(int64_t)band * D + c] = cs;
      asm volatile("" ::: "memory");  // one block's values live at a time
    }
    __syncthreads();  // the image is read: its bytes become the stage
  }

  // the 8 waves' dw / db of every column, summed in a fixed order
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int vi = lane + 64 * i;
    if (vi < nv) {
      f32x4* pw = reinterpret_cast<f32x4*>(stage + (wave * 2) * D + vi * 8);
      f32x4* pb = reinterpret_cast<f32x4*>(stage + (wave * 2 + 1) * D + vi * 8);
      pw[0] = f32x4{dw[i][0], dw[i][1], dw[i][2], dw[i][3]};
      pw[1] = f32x4{dw[i][4], dw[i][5], dw[i][6], dw[i][7]};
      pb[0] = f32x4{db[i][0], db[i][1], db[i][2], db[i][3]};
      pb[1] = f32x4{db[i][4], db[i][5], db[i][6], db[i][7]};
    }
  }
  __syncthreads();
  float* dst = part + (int64_t)band * 2 * D;
  for (int c = threadIdx.x; c < 2 * D; c += kLnbThreads) {  // c = which * D + column
    float v[kLnbWaves];
#pragma unroll
    for (int k = 0; k < kLnbWaves; ++k) v[k] = stage[k * 2 * D + c];
    dst[c] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  }
}

template <int VPL>
void lnb_launch(const bf16* dy, const bf16* x, const float* stats, const float* w, const bf16* dres, int64_t rows,
                int D, bf16* dx, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, float* cs_part, float* part,
                hipStream_t stream) {
  const size_t lds = (size_t)kBand * D * sizeof(bf16);  // = kLnbWaves * 2 * D floats
  if (qt) {
    const int bands = (int)(mx_pad(rows) / kBand);
    layernorm_bwd_mx_kernel<VPL, true><<<bands, kLnbThreads, lds, stream>>>(dy, x, stats, w, dres, rows, D, dx, q, s, qt,
                                                                           st, cs_part, part);
  } else {
    const int bands = layernorm_bwd_mx_bands(rows);
    layernorm_bwd_mx_kernel<VPL, false><<<bands, kLnbThreads, lds, stream>>>(dy, x, stats, w, dres, rows, D, dx, q, s,
                                                                            nullptr, nullptr, nullptr, part);
  }
}

}  // namespace

int layernorm_bwd_mx_bands(int64_t rows) { return (int)((rows + kBand - 1) / kBand); }

int64_t layernorm_bwd_mx_scratch_floats(int64_t rows, int D) {
  const int nb = layernorm_bwd_mx_bands(rows);
  return (int64_t)nb * 2 * D + reduce_parts_scratch_floats(nb, D);
}

void layernorm_bwd_mx(const void* dy, const void* x, const float* stats, const float* w, const void* dres,
                      int64_t rows, int D, void* dx, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, float* cs_part,
                      float* scratch, float* dw, float* db, hipStream_t stream) {
  if (rows <= 0) return;
  const bf16 *gb = static_cast<const bf16*>(dy), *xb = static_cast<const bf16*>(x);
  const bf16* rb = static_cast<const bf16*>(dres);
  bf16* dxb = static_cast<bf16*>(dx);
  const int nv = D / 8;
  if (nv <= 64)
    lnb_launch<1>(gb, xb, stats, w, rb, rows, D, dxb, q, s, qt, st, cs_part, scratch, stream);
  else if (nv <= 128)
    lnb_launch<2>(gb, xb, stats, w, rb, rows, D, dxb, q, s, qt, st, cs_part, scratch, stream);
  else
    lnb_launch<4>(gb, xb, stats, w, rb, rows, D, dxb, q, s, qt, st, cs_part, scratch, stream);
  // part [bands][2][D] -> dw = sum part[.][0], db = sum part[.][1] (two fixed-order levels, any number of bands)
  const int nb = layernorm_bwd_mx_bands(rows);
  reduce_parts(scratch, nb, D, scratch + (int64_t)nb * 2 * D, dw, db, stream);
}

}  // namespace kern
}  // namespace ringdp
