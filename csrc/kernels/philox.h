// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator
// behind ringdp's dropout masks.  Host and device: the mask a kernel applies can be reproduced anywhere from
// (seed, step, site, group) alone.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RINGDP_HD __host__ __device__ __forceinline__
#else
#define RINGDP_HD inline
#endif

namespace ringdp {
namespace philox {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;
constexpr uint32_t kWeyl0 = 0x9E3779B9u, kWeyl1 = 0xBB67AE85u;

struct U4 {
  uint32_t w[4];
};

RINGDP_HD U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kMul0 * c0, p1 = (uint64_t)kMul1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kWeyl0;
    k1 += kWeyl1;
  }
  return U4{{c0, c1, c2, c3}};
}

// thr = round(p * 65536) clamped to [0, 65535]; keep iff a 16-bit draw >= thr, so the realised keep probability is
// (65536 - thr) / 65536 and this is its exact inverse (rounded to fp32 once)
inline float keep_scale(uint32_t thr) { return (float)(65536.0 / (double)(65536u - thr)); }

}  // namespace philox
}  // namespace ringdp
