// Device-side learning-rate schedules and the model EMA for gfx950.
//
//  * lr_sched_kernel    one workgroup per scheduler step: thread g reads the step counter t, evaluates the factor
//                       f(t) in fp64 and writes (float)(base_lr[g] * f) to group g's lr tensor; after a barrier one
//                       thread stores the new counter
//  * ema_tick_kernel    one thread per update: num_updates += 1, w = 1 - decay_n (fp64, rounded once) -> record
//  * ema_update_*       e = fmaf(w, p - e, e) streamed as float4, multi-tensor over the optimizer's pointer table
//                       or one flat range
//
// As in optim.hip every value that changes from step to step lives in device memory, so a captured hipGraph step
// replays correctly.  No atomics, spin waits or fences: the kernels are ordered by their boundaries on one stream,
// and every element is written by exactly one thread, so results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace ringdp {
namespace kern {

namespace {

constexpr int kThreads = 256;
constexpr int kSchedThreads = 64;  // >= kAdamMaxGroups: one wave

__device__ __forceinline__ bool is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The factor of ringdp/optim/lr_scheduler.py at counter value t (the module docstring is the contract).
__device__ __forceinline__ double sched_factor(const LrSchedSpec& S, int64_t t) {
  const int64_t s = t / S.period;
  const int64_t W = S.warmup_steps;
  if (s < W) {
    const double a = S.warmup_start_factor;
    return a + (1.0 - a) * (double)s / (double)W;
  }
  const int64_t N = S.total_steps - W;
  int64_t u = s - W;
  u = u < 0 ? 0 : (u > N ? N : u);
  const double m = S.min_factor;
  switch (S.kind) {
    case kSchedCosine:
      return m + (1.0 - m) * (1.0 + cos(M_PI * (double)u / (double)N)) / 2.0;
    case kSchedPoly:
      return m + (1.0 - m) * pow(1.0 - (double)u / (double)N, S.power);
    case kSchedMultiStep: {
      int k = 0;
      for (int i = 0; i < S.nmilestones; ++i) k += S.milestones[i] <= s ? 1 : 0;
      return pow(S.gamma, (double)k);
    }
    default:
      return 1.0;
  }
}

__global__ __launch_bounds__(kSchedThreads) void lr_sched_kernel(LrSchedArgs a) {
  const int64_t t = *a.counter + (a.advance ? 1 : 0);
  const int g = threadIdx.x;
  if (g < a.ngroups) *a.group[g].lr_ptr = (float)(a.group[g].base_lr * sched_factor(a.spec, t));
  __syncthreads();  // every read of the counter precedes its store
  if (threadIdx.x == 0 && a.advance) *a.counter = t;
}

__global__ void ema_tick_kernel(int64_t* __restrict__ num_updates, float* __restrict__ w, double decay, int warmup) {
  const int64_t n = *num_updates + 1;
  *num_updates = n;
  double d = decay;
  if (warmup) {
    const double dw = (1.0 + (double)n) / (10.0 + (double)n);  // timm's warmup rule
    d = dw < d ? dw : d;
  }
  *w = (float)(1.0 - d);
}

// The element contract: d = p - e (rounded to fp32), e = fma(w, d, e).
__device__ __forceinline__ float ema_elem(float e, float p, float w) {
  const float d = p - e;
  return fmaf(w, d, e);
}

__device__ __forceinline__ void ema_vec4(float* __restrict__ e, const float* __restrict__ p, int64_t i, float w) {
  float4 ev = reinterpret_cast<float4*>(e)[i];
  const float4 pv = reinterpret_cast<const float4*>(p)[i];
  ev.x = ema_elem(ev.x, pv.x, w);
  ev.y = ema_elem(ev.y, pv.y, w);
  ev.z = ema_elem(ev.z, pv.z, w);
  ev.w = ema_elem(ev.w, pv.w, w);
  reinterpret_cast<float4*>(e)[i] = ev;
}

// Multi-tensor form over the optimizer's table layout ({tensor, start} chunks of kAdamChunk elements): p = shadow,
// g = source.  kVec: the host asserted that every base is 16-byte aligned; otherwise each chunk checks its own two
// pointers and takes the scalar loop when one is misaligned.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void ema_update_kernel(const AdamTensor* __restrict__ table,
                                                              const int64_t* __restrict__ chunks,
                                                              const float* __restrict__ wp) {
  const float w = *wp;
  const int64_t ti = chunks[2 * (int64_t)blockIdx.x];
  const int64_t start = chunks[2 * (int64_t)blockIdx.x + 1];
  const AdamTensor T = table[ti];
  const int64_t end = start + kAdamChunk < T.n ? start + kAdamChunk : T.n;
  float* e = T.p + start;
  const float* p = T.g + start;
  const int64_t n = end - start;
  if (kVec || (is_aligned16(e) && is_aligned16(p))) {
    const int64_t n4 = n >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += kThreads) ema_vec4(e, p, i, w);
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += kThreads) e[i] = ema_elem(e[i], p[i], w);
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kThreads) e[i] = ema_elem(e[i], p[i], w);
  }
}

// Flat form: one range, grid-stride.
__global__ __launch_bounds__(kThreads) void ema_update_flat_kernel(float* __restrict__ e, const float* __restrict__ p,
                                                                   int64_t n, const float* __restrict__ wp) {
  const float w = *wp;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += stride) ema_vec4(e, p, i, w);
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) e[i] = ema_elem(e[i], p[i], w);
}

}  // namespace

void lr_sched(const LrSchedArgs& a, hipStream_t s) { lr_sched_kernel<<<1, kSchedThreads, 0, s>>>(a); }

void ema_tick(int64_t* num_updates, float* w, double decay, bool warmup, hipStream_t s) {
  ema_tick_kernel<<<1, 1, 0, s>>>(num_updates, w, decay, warmup ? 1 : 0);
}

void ema_update_multi(const AdamTensor* table, const int64_t* chunks, int64_t nchunks, const float* w,
                      bool all_aligned, hipStream_t s) {
  if (nchunks <= 0) return;
  const unsigned grid = (unsigned)nchunks;
  if (all_aligned)
    ema_update_kernel<true><<<grid, kThreads, 0, s>>>(table, chunks, w);
  else
    ema_update_kernel<false><<<grid, kThreads, 0, s>>>(table, chunks, w);
}

void ema_update_flat(float* e, const float* p, int64_t n, const float* w, hipStream_t s) {
  if (n <= 0) return;
  int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;  // memory-bound: about 8 workgroups per CU, grid-stride the rest
  ema_update_flat_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(e, p, n, w);
}

}  // namespace kern
}  // namespace ringdp
