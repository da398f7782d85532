// bf16 ConvNet (design: convnet_fwd.hip): the fixed-order slab reduction that ends every layer's backward, and the
// host helpers that convnet_host.h declares.
#include <cstdlib>

#include "convnet_device.h"
#include "convnet_host.h"

namespace ringdp {
namespace kern {

namespace {

// ================================================================== fixed-order slab reductions
constexpr int kMaxRedSegs = 8;
struct ReduceSegs {
  ReduceSeg seg[kMaxRedSegs];
  int count;
};

// Each workgroup owns 64 x vec outputs of one segment (vec = 4: one 16-B load per slice per lane) and sums
// its slices with 8 waves (coalesced rows, 4 loads in flight per wave), combined in a fixed order.  Several
// waves per output group because the conv1 / fc1 segments have few outputs and hundreds of slices; 4
// outputs per lane and 8 (was 16) waves cut the B=100 merged reduction's wave count 8x.
constexpr int kRedWaves = 8;
__device__ __forceinline__ void red_store(const ReduceSeg& sg, int64_t i, float v) {
  if (sg.mode == 0) {
    sg.out[i] = v;
  } else if (sg.mode == 2) {
    const int t = (int)(i & 255), nj = (int)(i >> 8), n = nj >> 3, j = nj & 7;
    sg.out[n * 2048 + ((t & 15) * 8 + j) * 16 + (t >> 4)] = v;
  } else {
    const int n = (int)(i / sg.cout), co = (int)(i % sg.cout);
    sg.out[((int64_t)co * sg.cin + n % sg.cin) * 9 + n / sg.cin] = v;
  }
}

__global__ __launch_bounds__(64 * kRedWaves) void slab_reduce_kernel(ReduceSegs segs) {
  __shared__ f32x4 part[kRedWaves][64];
  int blk = blockIdx.x, sidx = 0;
  while (sidx < segs.count - 1 && blk >= segs.seg[sidx].blocks) {
    blk -= segs.seg[sidx].blocks;
    ++sidx;
  }
  const ReduceSeg& sg = segs.seg[sidx];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = sg.vec;
  const int64_t i0 = ((int64_t)blk * 64 + lane) * V;
  f32x4 a0 = zero_f32x4(), a1 = zero_f32x4(), a2 = zero_f32x4(), a3 = zero_f32x4();
  if (i0 < sg.n) {
    const float* pp = sg.slabs + sg.off + i0;
    int s = wave;
    if (V == 4) {
      for (; s + 3 * kRedWaves < sg.nslices; s += 4 * kRedWaves) {
        a0 += *reinterpret_cast<const f32x4*>(pp + (int64_t)s * sg.stride);
        a1 += *reinterpret_cast<const f32x4*>(pp + (int64_t)(s + kRedWaves) * sg.stride);
        a2 += *reinterpret_cast<const f32x4*>(pp + (int64_t)(s + 2 * kRedWaves) * sg.stride);
        a3 += *reinterpret_cast<const f32x4*>(pp + (int64_t)(s + 3 * kRedWaves) * sg.stride);
      }
      for (; s < sg.nslices; s += kRedWaves) a0 += *reinterpret_cast<const f32x4*>(pp + (int64_t)s * sg.stride);
    } else {
      for (; s + 3 * kRedWaves < sg.nslices; s += 4 * kRedWaves) {
        a0[0] += pp[(int64_t)s * sg.stride];
        a1[0] += pp[(int64_t)(s + kRedWaves) * sg.stride];
        a2[0] += pp[(int64_t)(s + 2 * kRedWaves) * sg.stride];
        a3[0] += pp[(int64_t)(s + 3 * kRedWaves) * sg.stride];
      }
      for (; s < sg.nslices; s += kRedWaves) a0[0] += pp[(int64_t)s * sg.stride];
    }
  }
  part[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (wave != 0 || i0 >= sg.n) return;
  f32x4 v = zero_f32x4();
#pragma unroll
  for (int w = 0; w < kRedWaves; ++w) v += part[w][lane];
  for (int k = 0; k < V; ++k) red_store(sg, i0 + k, v[k]);
}

}  // namespace

ReduceSeg seg(const float* slabs, int64_t stride, int64_t off, int64_t n, int nslices, float* out, int mode,
              int cin, int cout) {
  const int vec = ((off | stride | n) & 3) == 0 ? 4 : 1;
  return ReduceSeg{slabs, stride, off, n, nslices, out, mode, cin, cout, (int)((n + 64 * vec - 1) / (64 * vec)), vec};
}

void launch_reduce(const std::vector<ReduceSeg>& v, hipStream_t s) {
  if (v.empty()) return;
  if (v.size() > (size_t)kMaxRedSegs) {  // more than one launch holds: split
    launch_reduce(std::vector<ReduceSeg>(v.begin(), v.begin() + kMaxRedSegs), s);
    launch_reduce(std::vector<ReduceSeg>(v.begin() + kMaxRedSegs, v.end()), s);
    return;
  }
  ReduceSegs segs{};
  int total = 0;
  segs.count = (int)v.size();
  for (size_t k = 0; k < v.size(); ++k) {
    segs.seg[k] = v[k];
    total += v[k].blocks;
  }
  slab_reduce_kernel<<<total, 64 * kRedWaves, 0, s>>>(segs);
}

int num_cus() {
  static int cus = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
    }
    return n;
  }();
  return cus;
}

int env_int(const char* name, int dflt, bool (*ok)(int)) {
  const char* v = std::getenv(name);
  const int n = v ? std::atoi(v) : dflt;
  return !ok || ok(n) ? n : dflt;
}

double env_real(const char* name, double dflt, bool (*ok)(double)) {
  const char* v = std::getenv(name);
  const double f = v ? std::atof(v) : dflt;
  return ok(f) ? f : dflt;
}

int fc_in_c3_max_batch() {
  static const int v = env_int("RINGDP_CN_FC_IN_C3_MAX", 2048);
  return v;
}

void cn_launch_reduce(const ReduceList& segs, hipStream_t s) { launch_reduce(segs, s); }

}  // namespace kern
}  // namespace ringdp
