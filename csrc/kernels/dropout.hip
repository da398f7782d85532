// Dropout and stochastic depth (drop-path) for bf16 token rows on gfx950, hipGraph-safe.
//
//  * rng_tick_kernel  one thread per forward: state.step += 1, snapshot <- {seed, step}
//  * dropout_kernel   y = m * x  or  y = res + m * x  with m = m_row * m_elem regenerated from
//                     Philox4x32-10(key = seed, counter = (group, step lo, step hi, site)); no mask is stored, the
//                     backward runs the same kernel on dy with the same snapshot and site
//
// The generator state lives in device memory and advances inside the captured graph (as the Adam step counter
// does, optim.hip), so every replay draws new masks.  Every site of one forward and of its backward reads the
// forward's snapshot, never the live state, so fwd, fwd, bwd, bwd stays correct.  No atomics, arrival counters or
// fences: the tick and its readers are ordered by kernel boundaries on one stream.
//
// Memory-bound streams: one 16-byte load per operand and one Philox call (about 60 integer ops) per 8 elements,
// 2048 workgroups of four 64-wide waves at most (8 per CU) and a grid-stride loop over the rest, no LDS.  The
// snapshot pointer is wave-uniform.  With both factors on, the row decision is a second Philox call per vector although
// it is the same for a whole sample (thousands of vectors): twice the integer work of element mode on the
// dropout + drop-path sites, not timed by tools/dropout_bench.py (element mode only); the step times with and without
// stochastic depth are in profiles/r11/dropout/README.md.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"
#include "philox.h"

namespace ringdp {
namespace kern {

using namespace dev;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = 2048;

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__global__ void rng_tick_kernel(uint64_t* __restrict__ state, uint64_t* __restrict__ snapshot) {
  const uint64_t seed = state[0], step = state[1] + 1;
  state[1] = step;
  snapshot[0] = seed;
  snapshot[1] = step;
}

struct DropArgs {
  uint32_t site_e, thr_e, site_r, thr_r;
  float scale_e, scale_r;
  uint32_t row_vecs;  // 16-byte vectors per row-mode sample
};

// kElem / kRow: which factors of m are on; kAdd: y = res + m * x (a dropped vector / element yields res bit for bit)
template <bool kElem, bool kRow, bool kAdd>
__global__ __launch_bounds__(kThreads) void dropout_kernel(const bf16* __restrict__ x, const bf16* __restrict__ res,
                                                           const uint64_t* __restrict__ snapshot, DropArgs a,
                                                           int64_t nvec, bf16* __restrict__ y) {
  const uint64_t seed = snapshot[0], step = snapshot[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += stride) {
    const uint32_t g = (uint32_t)v;  // nvec < 2^32 (checked by the caller)
    float m_row = 1.f;
    if (kRow) {
      const philox::U4 r = philox::philox4x32_10(g / a.row_vecs, s0, s1, a.site_r, k0, k1);
      m_row = (r.w[0] & 0xffffu) >= a.thr_r ? a.scale_r : 0.f;
    }
    u16x8 o;
    if (kRow && m_row == 0.f) {  // a dropped sample: x is not read
      if (kAdd) {
        o = reinterpret_cast<const u16x8*>(res)[v];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0;
      }
      reinterpret_cast<u16x8*>(y)[v] = o;
      continue;
    }
    const bf16x8 xv = reinterpret_cast<const bf16x8*>(x)[v];
    u16x8 rbits = {};
    if (kAdd) rbits = reinterpret_cast<const u16x8*>(res)[v];
    const bf16x8 rv = __builtin_bit_cast(bf16x8, rbits);
    philox::U4 e = {};
    if (kElem) e = philox::philox4x32_10(g, s0, s1, a.site_e, k0, k1);
    const float m = kElem ? m_row * a.scale_e : m_row;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = !kElem || ((e.w[j >> 1] >> (16 * (j & 1))) & 0xffffu) >= a.thr_e;
      if (kAdd) {
        const bf16 s = (bf16)__builtin_fmaf(m, (float)xv[j], (float)rv[j]);  // one fp32 rounding, then bf16
        o[j] = keep ? __builtin_bit_cast(unsigned short, s) : rbits[j];
      } else {
        const bf16 s = (bf16)(m * (float)xv[j]);
        o[j] = keep ? __builtin_bit_cast(unsigned short, s) : (unsigned short)0;
      }
    }
    reinterpret_cast<u16x8*>(y)[v] = o;
  }
}

template <bool kElem, bool kRow>
void launch(const void* x, const void* res, const uint64_t* snapshot, const DropArgs& a, int64_t nvec, void* y,
            hipStream_t s) {
  int64_t blocks = (nvec + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const bf16* xp = static_cast<const bf16*>(x);
  const bf16* rp = static_cast<const bf16*>(res);
  bf16* yp = static_cast<bf16*>(y);
  if (res != nullptr)
    dropout_kernel<kElem, kRow, true><<<(unsigned)blocks, kThreads, 0, s>>>(xp, rp, snapshot, a, nvec, yp);
  else
    dropout_kernel<kElem, kRow, false><<<(unsigned)blocks, kThreads, 0, s>>>(xp, rp, snapshot, a, nvec, yp);
}

}  // namespace

void rng_tick(uint64_t* state, uint64_t* snapshot, hipStream_t s) {
  rng_tick_kernel<<<1, 1, 0, s>>>(state, snapshot);
}

void dropout_bf16(const void* x, const void* res, const uint64_t* snapshot, uint32_t site_e, uint32_t thr_e,
                  uint32_t site_r, uint32_t thr_r, int64_t row_elems, int64_t n, void* y, hipStream_t s) {
  const int64_t nvec = n / 8;
  if (nvec <= 0 || (thr_e == 0 && thr_r == 0)) return;  // callers take the identity path themselves
  DropArgs a{};
  a.site_e = site_e;
  a.thr_e = thr_e;
  a.site_r = site_r;
  a.thr_r = thr_r;
  a.scale_e = philox::keep_scale(thr_e);
  a.scale_r = philox::keep_scale(thr_r);
  a.row_vecs = (uint32_t)(thr_r ? row_elems / 8 : 1);
  if (thr_e && thr_r)
    launch<true, true>(x, res, snapshot, a, nvec, y, s);
  else if (thr_e)
    launch<true, false>(x, res, snapshot, a, nvec, y, s);
  else
    launch<false, true>(x, res, snapshot, a, nvec, y, s);
}

}  // namespace kern
}  // namespace ringdp
