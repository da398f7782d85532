// Adam / AdamW with fused global-norm gradient clipping for gfx950.
//
//  * grad_sumsq_kernel   one workgroup per {tensor, start} chunk of 65536 elements: sum of g^2 -> partials[chunk]
//  * adam_prepare_kernel one workgroup per step(): partials -> total_norm / clip_coef (fp64, fixed order), step
//                        counters += 1, bias corrections, the per-group records the update kernels read
//  * adam_update_*       p / g / m / v streamed as float4; math in adam_device.h (torch's single-tensor Adam)
//  * grad_scale_multi    g *= clip_coef in place (ringdp.nn.utils.clip_grad_norm_)
//
// Every value that changes from step to step (step count, lr, clip coefficient) lives in device memory, so a
// captured hipGraph step replays correctly.  No atomics, arrival counters, spin waits or fences: the kernels are
// ordered by their boundaries on one stream, and every reduction has a fixed element-to-thread mapping and a fixed
// tree, so results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include "adam_device.h"
#include "kernels.h"

namespace ringdp {
namespace kern {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Chunk {
  int64_t tensor, start, end;
};

__device__ __forceinline__ Chunk load_chunk(const AdamTensor* __restrict__ table, const int64_t* __restrict__ chunks,
                                            AdamTensor& T) {
  Chunk c;
  c.tensor = chunks[2 * (int64_t)blockIdx.x];
  c.start = chunks[2 * (int64_t)blockIdx.x + 1];
  T = table[c.tensor];
  c.end = c.start + kAdamChunk < T.n ? c.start + kAdamChunk : T.n;
  return c;
}

// Sum over the workgroup in a fixed tree: xor-shuffles inside each wave, then the 4 wave sums in order.
template <typename T>
__device__ __forceinline__ T block_sum(T x, T* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = x;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const AdamTensor* __restrict__ table,
                                                              const int64_t* __restrict__ chunks,
                                                              float* __restrict__ partials) {
  __shared__ float lds[4];
  AdamTensor T;
  const Chunk c = load_chunk(table, chunks, T);
  const float* g = T.g + c.start;
  const int64_t n = c.end - c.start;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (is_aligned16(g)) {
    const int64_t n4 = n >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += kThreads) {
      const float4 x = reinterpret_cast<const float4*>(g)[i];
      a0 = fmaf(x.x, x.x, a0);
      a1 = fmaf(x.y, x.y, a1);
      a2 = fmaf(x.z, x.z, a2);
      a3 = fmaf(x.w, x.w, a3);
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += kThreads) a0 = fmaf(g[i], g[i], a0);
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kThreads) a0 = fmaf(g[i], g[i], a0);
  }
  const float s = block_sum((a0 + a1) + (a2 + a3), lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void adam_prepare_kernel(AdamPrepArgs a) {
  __shared__ double lds[4];
  float clip = 1.f;
  if (a.partials != nullptr) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.npartials; i += kThreads) acc += (double)a.partials[i];
    const double sum = block_sum(acc, lds);
    const float total = (float)sqrt(sum);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); a NaN norm stays NaN
    const float coef = a.max_norm / (total + 1e-6f);
    clip = coef > 1.f ? 1.f : coef;
    if (threadIdx.x == 0) {
      a.rec[0] = total;
      a.rec[1] = clip;
    }
  }
  const int gi = threadIdx.x;
  if (gi < a.ngroups) {
    const AdamGroupPrep& G = a.group[gi];
    const float t = *G.step + 1.f;
    *G.step = t;
    const float lr = G.lr_ptr ? *G.lr_ptr : G.lr;
    const double bc1 = 1.0 - pow(G.beta1, (double)t);
    const double bc2 = 1.0 - pow(G.beta2, (double)t);
    float* r = a.rec + kAdamRecHead + kAdamRecGroup * gi;
    r[0] = lr;
    r[1] = (float)((double)lr / bc1);
    r[2] = (float)(1.0 / sqrt(bc2));
    r[3] = clip;
  }
}

template <bool kDecoupled>
__device__ __forceinline__ void adam_vec4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int64_t i, const AdamDev& d) {
  float4 pv = reinterpret_cast<float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 mv = reinterpret_cast<float4*>(m)[i];
  float4 vv = reinterpret_cast<float4*>(v)[i];
  adam_elem<kDecoupled>(pv.x, gv.x, mv.x, vv.x, d);
  adam_elem<kDecoupled>(pv.y, gv.y, mv.y, vv.y, d);
  adam_elem<kDecoupled>(pv.z, gv.z, mv.z, vv.z, d);
  adam_elem<kDecoupled>(pv.w, gv.w, mv.w, vv.w, d);
  reinterpret_cast<float4*>(p)[i] = pv;
  reinterpret_cast<float4*>(m)[i] = mv;
  reinterpret_cast<float4*>(v)[i] = vv;
}

template <bool kDecoupled>
__device__ __forceinline__ void adam_scalar(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t i, const AdamDev& d) {
  float pv = p[i], mv = m[i], vv = v[i];
  adam_elem<kDecoupled>(pv, g[i], mv, vv, d);
  p[i] = pv;
  m[i] = mv;
  v[i] = vv;
}

// Multi-tensor form.  kVec: the host asserted that every base is 16-byte aligned; otherwise each chunk checks its
// own four pointers and takes the scalar loop when one is misaligned.
template <bool kDecoupled, bool kVec>
__global__ __launch_bounds__(kThreads) void adam_update_kernel(const AdamTensor* __restrict__ table,
                                                               const int64_t* __restrict__ chunks, AdamArgs a) {
  const AdamDev d = load_adam(a);
  AdamTensor T;
  const Chunk c = load_chunk(table, chunks, T);
  float* p = T.p + c.start;
  const float* g = T.g + c.start;
  float* m = T.m + c.start;
  float* v = T.v + c.start;
  const int64_t n = c.end - c.start;
  if (kVec || (is_aligned16(p) && is_aligned16(g) && is_aligned16(m) && is_aligned16(v))) {
    const int64_t n4 = n >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += kThreads) adam_vec4<kDecoupled>(p, g, m, v, i, d);
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += kThreads) adam_scalar<kDecoupled>(p, g, m, v, i, d);
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kThreads) adam_scalar<kDecoupled>(p, g, m, v, i, d);
  }
}

// Flat form: one range, grid-stride.
template <bool kDecoupled>
__global__ __launch_bounds__(kThreads) void adam_update_flat_kernel(float* __restrict__ p,
                                                                    const float* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v,
                                                                    int64_t n, AdamArgs a) {
  const AdamDev d = load_adam(a);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += stride) adam_vec4<kDecoupled>(p, g, m, v, i, d);
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) adam_scalar<kDecoupled>(p, g, m, v, i, d);
}

__global__ __launch_bounds__(kThreads) void grad_scale_multi_kernel(const AdamTensor* __restrict__ table,
                                                                    const int64_t* __restrict__ chunks,
                                                                    const float* __restrict__ rec) {
  const float coef = rec[1];
  AdamTensor T;
  const Chunk c = load_chunk(table, chunks, T);
  float* g = T.g + c.start;
  const int64_t n = c.end - c.start;
  if (is_aligned16(g)) {
    const int64_t n4 = n >> 2;
    for (int64_t i = threadIdx.x; i < n4; i += kThreads) {
      float4 x = reinterpret_cast<float4*>(g)[i];
      x.x *= coef;
      x.y *= coef;
      x.z *= coef;
      x.w *= coef;
      reinterpret_cast<float4*>(g)[i] = x;
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += kThreads) g[i] *= coef;
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kThreads) g[i] *= coef;
  }
}

}  // namespace

void grad_sumsq(const AdamTensor* table, const int64_t* chunks, int64_t nchunks, float* partials, hipStream_t s) {
  if (nchunks <= 0) return;
  grad_sumsq_kernel<<<(unsigned)nchunks, kThreads, 0, s>>>(table, chunks, partials);
}

void adam_prepare(const AdamPrepArgs& a, hipStream_t s) { adam_prepare_kernel<<<1, kThreads, 0, s>>>(a); }

void adam_update_multi(const AdamTensor* table, const int64_t* chunks, int64_t nchunks, const AdamArgs& a,
                       bool decoupled, bool all_aligned, hipStream_t s) {
  if (nchunks <= 0) return;
  const unsigned grid = (unsigned)nchunks;
  if (decoupled) {
    if (all_aligned)
      adam_update_kernel<true, true><<<grid, kThreads, 0, s>>>(table, chunks, a);
    else
      adam_update_kernel<true, false><<<grid, kThreads, 0, s>>>(table, chunks, a);
  } else {
    if (all_aligned)
      adam_update_kernel<false, true><<<grid, kThreads, 0, s>>>(table, chunks, a);
    else
      adam_update_kernel<false, false><<<grid, kThreads, 0, s>>>(table, chunks, a);
  }
}

void adam_update_flat(float* p, const float* g, float* m, float* v, int64_t n, const AdamArgs& a, bool decoupled,
                      hipStream_t s) {
  if (n <= 0) return;
  int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;  // memory-bound: about 8 workgroups per CU, grid-stride the rest
  if (decoupled)
    adam_update_flat_kernel<true><<<(unsigned)blocks, kThreads, 0, s>>>(p, g, m, v, n, a);
  else
    adam_update_flat_kernel<false><<<(unsigned)blocks, kThreads, 0, s>>>(p, g, m, v, n, a);
}

void grad_scale_multi(const AdamTensor* table, const int64_t* chunks, int64_t nchunks, const float* rec,
                      hipStream_t s) {
  if (nchunks <= 0) return;
  grad_scale_multi_kernel<<<(unsigned)nchunks, kThreads, 0, s>>>(table, chunks, rec);
}

}  // namespace kern
}  // namespace ringdp
