// MXFP8 scale rule and element packing shared by the quantiser (mxfp8.hip) and the GEMM epilogue that writes
// MXFP8 (gemm256_store_mx, gemm256_epilogue.h): both must give the same bytes for the same bf16 values.
#pragma once

#include "device_common.h"

namespace ringdp {
namespace kern {

// unbiased block exponent of a block with amax a >= 0: the smallest e with a * 2^-e <= 448, clamped to
// [-127, 127], 0 for an all-zero block (see the header of mxfp8.hip)
__device__ __forceinline__ int mx_exp(float a) {
  const unsigned u = __float_as_uint(a);
  const int e = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return u == 0 ? 0 : max(-127, min(127, e));
}

// four values scaled by 2^-e (exact) as four e4m3 bytes, round to nearest even
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, int e) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(a, -e), ldexpf(b, -e), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(c, -e), ldexpf(d, -e), w, true);
  return (unsigned)w;
}

}  // namespace kern
}  // namespace ringdp
