// fp32 ConvNet weight (+ bias) gradients: split-K implicit GEMMs and the dedicated conv2 / conv3 kernels into
// per-slice slabs, and the fixed-order slab reductions (design: conv_f32_gemm.h).
#include "conv_f32_gemm.h"

namespace ringdp::kern {
namespace {

// Fixed-order sums of the split-K slabs [slices][Kout][Nw + has_bias]: stage 1 sums groups of
// kSlabGroup consecutive slices into part[group] (grid.y = groups), stage 2 sums the groups into
// dw [Kout][Nw] and db [Kout].  Two stages keep each thread's serial chain short.
__global__ __launch_bounds__(256) void slab_group_kernel(const float* __restrict__ slab, int slices, int total,
                                                         float* __restrict__ part) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= total) return;
  const int z0 = static_cast<int>(blockIdx.y) * kSlabGroup, z1 = min(z0 + kSlabGroup, slices);
  float acc = 0.f;
  for (int z = z0; z < z1; ++z) acc += slab[static_cast<int64_t>(z) * total + i];
  part[static_cast<int64_t>(blockIdx.y) * total + i] = acc;
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, int slices, int Kout,
                                                           int Nw, int ncol, float* __restrict__ dw,
                                                           float* __restrict__ db) {
  const int total = Kout * ncol;
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < total;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    float acc = slab[i];
    for (int z = 1; z < slices; ++z) acc += slab[static_cast<int64_t>(z) * total + i];
    const int m = i / ncol, n = i - m * ncol;
    if (n < Nw) dw[m * Nw + n] = acc;
    else db[m] = acc;
  }
}

// f32_slab_reduce of up to kF32RedMax segments in one launch: element e of a segment is the sum of its slices in
// the two-stage order of slab_group_kernel + wgrad_reduce_kernel (groups of kSlabGroup slices summed from 0.f,
// then the group sums in order; one group: the slices in order) - the same bits, done by one thread.
struct F32RedArgs {
  F32RedSeg seg[kF32RedMax];
  int bstart[kF32RedMax];  // first workgroup of each segment
  int n;
};
// Two kinds of workgroup, chosen per segment on the host: a segment of at most kSlabGroup slices (one group) gets
// 256 elements per workgroup, one thread each summing the slices in order (unconditional loads, all in flight);
// a segment with more slices gets 32 elements x 8 group lanes: lane q sums groups q, q + 8, .. into LDS and lane 0
// adds the group sums in order.  Both are the two-stage arithmetic of slab_group_kernel + wgrad_reduce_kernel.
// (One 32-element workgroup kind for every segment was 3553 workgroups at B=100 and ~20 us of dispatch; the
// serial one-thread form before it spent 20 us in conv1's 400-slice chain.)
constexpr int kRedLanes = 8, kRedElems = 256 / kRedLanes, kRedMaxGroups = 64;

__device__ __forceinline__ float red_group(const F32RedSeg& sg, int total, int e, int z0) {
  // unconditional loads (index clamped into the group) from a global-address-space pointer: a guarded load is a
  // branch the compiler will not hoist past, and the slab pointer read back from LDS would be a flat access
  const int nz = min(kSlabGroup, sg.slices - z0);
  const __attribute__((address_space(1))) float* src =
      (const __attribute__((address_space(1))) float*)(sg.slab + static_cast<int64_t>(z0) * total + e);
  float v[kSlabGroup];
#pragma unroll
  for (int z = 0; z < kSlabGroup; ++z) v[z] = src[static_cast<int64_t>(min(z, nz - 1)) * total];
  float p = 0.f;
#pragma unroll
  for (int z = 0; z < kSlabGroup; ++z)
    if (z < nz) p += v[z];
  return p;
}

__device__ __forceinline__ void red_store_f32(const F32RedSeg& sg, int e, float t) {
  const int m = e / sg.ncol, n = e - m * sg.ncol;
  if (n < sg.Nw) sg.dw[m * sg.Nw + n] = t;
  else sg.db[m] = t;
}

__global__ __launch_bounds__(256) void f32_reduce_multi_kernel(F32RedArgs a) {
  __shared__ float part[kRedMaxGroups][kRedElems];
  // the segment of this workgroup: compile-time indices into the by-value argument (a run-time index would copy
  // it to scratch per thread)
  int k = 0;
#pragma unroll
  for (int i = 1; i < kF32RedMax; ++i)
    if (i < a.n && (int)blockIdx.x >= a.bstart[i]) k = i;
  F32RedSeg sg = a.seg[0];
  int b0 = a.bstart[0];
#pragma unroll
  for (int i = 1; i < kF32RedMax; ++i)
    if (i == k) {
      sg = a.seg[i];
      b0 = a.bstart[i];
    }
  const int total = sg.Kout * sg.ncol, blk = (int)blockIdx.x - b0;
  const int ngroups = (sg.slices + kSlabGroup - 1) / kSlabGroup;
  if (ngroups == 1) {  // 256 elements, one thread each
    const int e = blk * 256 + (int)threadIdx.x;
    if (e < total) red_store_f32(sg, e, red_group(sg, total, e, 0));
    return;
  }
  const int el = threadIdx.x % kRedElems, q = threadIdx.x / kRedElems;
  const int e = blk * kRedElems + el;
  const bool live = e < total;
  const bool staged = ngroups <= kRedMaxGroups;
  for (int g = q; live && staged && g < ngroups; g += kRedLanes) part[g][el] = red_group(sg, total, e, g * kSlabGroup);
  __syncthreads();
  if (q != 0 || !live) return;
  float t;
  if (staged) {
    t = part[0][el];
    for (int g = 1; g < ngroups; ++g) t += part[g][el];
  } else {  // more slices than the LDS stage holds: every group in order by this thread
    t = red_group(sg, total, e, 0);
    for (int g = 1; g < ngroups; ++g) t += red_group(sg, total, e, g * kSlabGroup);
  }
  red_store_f32(sg, e, t);
}

// RINGDP_F32_WGRAD_MIN_K: shallowest k slice of a weight gradient.  512 (was 1024): B=100 step 318 -> 296 us
// (256: 297, 128: 306); B=65536 unchanged (profiles/r05/fp32/).  320 on the round-6 step (every slab reduced by
// one launch, so more slices cost little): 216 -> 209 us (192: 217, 256: 211, 384: 212, 1024: 241;
// profiles/r06/fp32/b100_wgrad_depth_sweep.txt).
int wgrad_min_depth() {
  static const int d = [] {
    const char* e = std::getenv("RINGDP_F32_WGRAD_MIN_K");
    return e && *e ? std::max(BK, std::atoi(e)) : 320;
  }();
  return d;
}

int wgrad_slices(int M, int N, int64_t K) {
  // enough slices to put >= ~2048 workgroups on the 256 CUs, each slice >= wgrad_min_depth() deep
  const Layout l = pick_layout(M, N, 1 << 20);  // the big-tile layout (the launch may still pick 32x32)
  const int bm = layout_bm(l), bn = layout_bn(l);
  const int64_t tiles = static_cast<int64_t>((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  int64_t s = (2048 + tiles - 1) / tiles;
  // K below one minimum-depth slice on a grid of < 64 tiles (fc1 at B=100: 16 tiles, K = 100): 2-k-tile slices
  const int depth = (K < wgrad_min_depth() && tiles < 64) ? 2 * BK : wgrad_min_depth();
  const int64_t cap = (K + depth - 1) / depth;
  if (s > cap) s = cap;
  return static_cast<int>(s < 1 ? 1 : (s > 1024 ? 1024 : s));
}

int64_t wgrad_chunk(const ConvF32Geom& g) {
  return batch_chunk(g.B, {static_cast<int64_t>(g.C) * g.H * g.W, static_cast<int64_t>(g.Kout) * g.OH * g.OW});
}

// The weight-gradient B operand of images [b0, b0 + nb) by input kind - raw uint8 pixels, a padded fp32 input or
// a valid one - handed to `launch` (a generic lambda around launch_gemm).
template <class F>
void with_wgrad_b(const ConvF32Geom& g, const float* x, const unsigned char* xu8, float mean, float inv_std,
                  int64_t b0, int nb, F&& launch) {
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W;
  const int Nw = g.C * g.R * g.R, xbytes = static_cast<int>(nb * xin);
  const FastDiv ohw = make_fdiv(g.OH * g.OW), ow = make_fdiv(g.OW);
  if (xu8) launch(WgradB<true, true>{{xu8 + b0 * xin, xbytes, mean, inv_std}, g.C, g.H, g.W, g.R, g.pad, g.OW, Nw, ohw, ow});
  else if (g.pad) launch(WgradB<false, true>{{x + b0 * xin, xbytes * 4, 0.f, 1.f}, g.C, g.H, g.W, g.R, g.pad, g.OW, Nw, ohw, ow});
  else launch(WgradB<false, false>{{x + b0 * xin, xbytes * 4, 0.f, 1.f}, g.C, g.H, g.W, g.R, g.pad, g.OW, Nw, ohw, ow});
}

}  // namespace

constexpr int W3_SLICES = 128;                    // conv3's image slices (slab rows): 512 workgroups, 2 per CU
constexpr int W2_SLICES = 256;                    // conv2's (2 channel tiles): 512 workgroups

// ---------------------------------------------------------------- conv3 weight gradient
// dW3[co][ci][t] = sum over images b and the 8x8 positions p of dz3[b][co][p] * a2[b][ci][p + t] (+ the bias
// gradient db3[co] = sum dz3): a dedicated kernel instead of the implicit GEMM's per-element gathers.  Workgroup
// (ct, slice) owns input channels [16 ct, +16) and images [B slice / S, B (slice + 1) / S); wave w owns output
// channels [32 w, +32) x 16 channels x 9 taps (18 MFMA tiles).  Per image both operands come from LDS with
// compile-time offsets: dz3 in its natural [co][p] order with a row stride of 2 mod 32 banks (the A fragment,
// 16 co x 4 positions, is a conflict-free b32 read; the transposed layout it replaces made every staging
// store a 16-way bank conflict) and the 16-channel a2 tile (the tap shift is an immediate).  The bias sums
// ride in the staging (ct = 0 workgroups, VALU).  The next image's operands are loaded into registers during
// the k loop.  Each workgroup writes its slice's partial dW into slab[slice][co][ci 9 + t] (+ the bias
// column), reduced by the same fixed-order f32_slab_reduce as the GEMM path: deterministic.
constexpr int W3_DS = 66;   // floats per co row of the dz3 tile (64 positions + 2; 66 = 2 mod 32)
constexpr int W3_AS = 101;  // floats per channel row of the a2 tile (odd)

__global__ __launch_bounds__(256, 2) void conv3_wgrad_f32_kernel(const float* __restrict__ dz,
                                                                  const float* __restrict__ a2,
                                                                  float* __restrict__ slab, int B) {
  // single-buffered (40.3 KB): two workgroups per CU, so one stages while the other multiplies
  __shared__ __attribute__((aligned(16))) float DZ[128 * W3_DS];  // 33.8 KB
  __shared__ __attribute__((aligned(16))) float AX[16 * W3_AS];   // 6.5 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int ct = blockIdx.x & 3, slice = blockIdx.x >> 2;
  const int b0 = static_cast<int>((int64_t)B * slice / W3_SLICES), b1 = static_cast<int>((int64_t)B * (slice + 1) / W3_SLICES);
  const bool bias = ct == 0;
  // staging: dz3 = 2048 float4 (co = e >> 4, positions 4 (e & 15) ..), 8 per thread; the a2 tile = 400 float4
  // (channel 4 e / 100, never crossing a row), 1-2 per thread
  float4 rz[8], ra[2];
  auto load = [&](int b) {
    const float4* z4 = reinterpret_cast<const float4*>(dz + (int64_t)b * 8192);
#pragma unroll
    for (int u = 0; u < 8; ++u) rz[u] = z4[tid + 256 * u];
    const float4* a4 = reinterpret_cast<const float4*>(a2 + (int64_t)b * 6400 + ct * 1600);
    ra[0] = a4[tid];
    ra[1] = a4[tid < 144 ? 256 + tid : tid];
  };
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // bias partials of co (tid >> 4) + 16 u
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = tid + 256 * u, co = e >> 4, p = (e & 15) * 4;
      float2* d = reinterpret_cast<float2*>(DZ + co * W3_DS + p);  // 8-B aligned (W3_DS even)
      d[0] = make_float2(rz[u].x, rz[u].y);
      d[1] = make_float2(rz[u].z, rz[u].w);
      if (bias) bsum[u] += (rz[u].x + rz[u].y) + (rz[u].z + rz[u].w);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + 256 * u;
      if (u == 0 || tid < 144) {
        const int c = (4 * e) / 100, q = 4 * e - 100 * c;
        AX[c * W3_AS + q + 0] = ra[u].x;
        AX[c * W3_AS + q + 1] = ra[u].y;
        AX[c * W3_AS + q + 2] = ra[u].z;
        AX[c * W3_AS + q + 3] = ra[u].w;
      }
    }
  };
  f32x4 acc[2][9];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = dev::zero_f32x4();
  const int abase = (32 * wave + lr) * W3_DS + lk;  // A: output channel 32 w + 16 j + lr, position 4 ks + lk
  const int xbase = lr * W3_AS + lk;                // B: channel lr, position (ks >> 1, 4 (ks & 1) + lk) + tap
  if (b0 < b1) load(b0);
  for (int b = b0; b < b1; ++b) {
    stash();
    __syncthreads();
    if (b + 1 < b1) load(b + 1);  // in flight during the k loop
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      float a[2], w[9];
#pragma unroll
      for (int j = 0; j < 2; ++j) a[j] = DZ[abase + 4 * ks + 16 * j * W3_DS];
#pragma unroll
      for (int t = 0; t < 9; ++t) w[t] = AX[xbase + ((ks >> 1) + t / 3) * 10 + 4 * (ks & 1) + t % 3];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[t], acc[j][t], 0, 0, 0);
    }
    __syncthreads();  // the tile is read out before the next image's stash
  }
  // partial dW of this slice: lane holds D[co = 32 w + 16 j + 4 lk + r][ci = 16 ct + lr] per tap
  constexpr int NCOL = 64 * 9 + 1;
  float* out = slab + (int64_t)slice * 128 * NCOL;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = 32 * wave + 16 * j + 4 * lk + r;
#pragma unroll
      for (int t = 0; t < 9; ++t) out[co * NCOL + (16 * ct + lr) * 9 + t] = acc[j][t][r];
    }
  if (bias) {  // the 16 threads sharing co (tid >> 4) + 16 u hold the 4-position partials of all 64 positions
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float v = bsum[u];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      if ((tid & 15) == 0) out[((tid >> 4) + 16 * u) * NCOL + 576] = v;
    }
  }
}

// conv2's weight gradient (64 <- 32 channels, 13x13 -> 11x11) the same way: workgroup (ct of 2, slice) owns
// input channels [16 ct, +16), wave w output channels [16 w, +16) x 16 x 9 taps.  The 121 positions are 31
// k-steps of 4 (positions 121..123 of the dz2 tile are zero); a position's 13x13 offset is a per-lane table
// (the 11-wide rows do not split on k-step boundaries).  dz2 stays in its natural [co][p] order with a row
// stride of 2 mod 32 banks, so the A fragment (16 co x 4 positions) is a conflict-free read and the staging
// writes run along rows.  256 slices (512 workgroups, 2 per CU) and the next image's loads in flight during
// the k loop: with 256 workgroups and no prefetch the staging was exposed (4.49 ms vs the GEMM's 4.19).
constexpr int W2_S = 130;   // floats per output-channel row of the dz2 tile (121 + 9; 130 = 2 mod 32)
constexpr int W2_AS = 171;  // floats per channel row of the a1 tile (odd)

__global__ __launch_bounds__(256, 2) void conv2_wgrad_f32_kernel(const float* __restrict__ dz,
                                                                  const float* __restrict__ a1,
                                                                  float* __restrict__ slab, int B) {
  __shared__ __attribute__((aligned(16))) float DZ[64 * W2_S];   // 33.3 KB
  __shared__ __attribute__((aligned(16))) float AX[16 * W2_AS];  // 10.9 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int ct = blockIdx.x & 1, slice = blockIdx.x >> 1;
  const int b0 = static_cast<int>((int64_t)B * slice / W2_SLICES), b1 = static_cast<int>((int64_t)B * (slice + 1) / W2_SLICES);
  const bool bias = ct == 0;
  // padding positions 121..123 of every row: zero once (never written by the staging)
  for (int e = tid; e < 64 * 3; e += 256) DZ[(e / 3) * W2_S + 121 + e % 3] = 0.f;
  int xoff[31];  // per k-step: the 13x13 offset of this lane's position 4 ks + lk (clamped past 120)
#pragma unroll
  for (int ks = 0; ks < 31; ++ks) {
    const int p = min(4 * ks + lk, 120);
    xoff[ks] = (p / 11) * 13 + p % 11;
  }
  f32x4 acc[9], accb = dev::zero_f32x4();  // accb: the bias sums (ct = 0), one MFMA against ones per k-step
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = dev::zero_f32x4();
  // staging registers: dz2 image = 7744 floats = 1936 float4 (8 per thread), a1 tile 16 x 169 = 676 float4 (3)
  float4 rz[8], ra[3];
  auto load = [&](int b) {
    const float4* z4 = reinterpret_cast<const float4*>(dz + (int64_t)b * 7744);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (tid + 256 * u < 1936) rz[u] = z4[tid + 256 * u];
    const float4* a4 = reinterpret_cast<const float4*>(a1 + (int64_t)b * 5408 + ct * 2704);
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (tid + 256 * u < 676) ra[u] = a4[tid + 256 * u];
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = tid + 256 * u;
      if (e < 1936) {
        const float vv[4] = {rz[u].x, rz[u].y, rz[u].z, rz[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * e + j, co = f / 121, p = f - 121 * co;
          DZ[co * W2_S + p] = vv[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e = tid + 256 * u;
      if (e < 676) {
        const float vv[4] = {ra[u].x, ra[u].y, ra[u].z, ra[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * e + j, c = f / 169, q = f - 169 * c;
          AX[c * W2_AS + q] = vv[j];
        }
      }
    }
  };
  const int abase = (16 * wave + lr) * W2_S + lk;  // A: output channel 16 w + lr, position 4 ks + lk
  const int xbase = lr * W2_AS;                    // B: channel lr, position offset xoff[ks] + tap
  if (b0 < b1) load(b0);
  for (int b = b0; b < b1; ++b) {
    stash();
    __syncthreads();
    if (b + 1 < b1) load(b + 1);  // in flight during the k loop
    // one straight k-loop per workgroup kind (a uniform branch outside it, not one per k-step)
    auto kloop = [&](auto with_bias) {
#pragma unroll
      for (int ks = 0; ks < 31; ++ks) {
        const float a = DZ[abase + 4 * ks];
        float w[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = AX[xbase + xoff[ks] + (t / 3) * 13 + t % 3];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[t], acc[t], 0, 0, 0);
        if constexpr (decltype(with_bias)::value) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.f, accb, 0, 0, 0);
      }
    };
    if (bias)
      kloop(std::true_type{});
    else
      kloop(std::false_type{});
    __syncthreads();
  }
  constexpr int NCOL = 32 * 9 + 1;
  float* out = slab + (int64_t)slice * 64 * NCOL;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = 16 * wave + 4 * lk + r;
#pragma unroll
    for (int t = 0; t < 9; ++t) out[co * NCOL + (16 * ct + lr) * 9 + t] = acc[t][r];
  }
  if (bias && lr == 0) {  // every column of accb holds the row sums
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(16 * wave + 4 * lk + r) * NCOL + 288] = accb[r];
  }
}

static bool conv3_wgrad_f32_ok(const ConvF32Geom& g) {
  return is_convnet_conv3(g) && g.B >= 8 * W3_SLICES && g.B * 8192 < (int64_t{1} << 31);
}
static bool conv2_wgrad_f32_ok(const ConvF32Geom& g) {
  return is_convnet_conv2(g) && g.B >= 4 * W2_SLICES && g.B * 7744 < (int64_t{1} << 31);
}

int conv_f32_wgrad_slices(const ConvF32Geom& g) {
  if (conv3_wgrad_f32_ok(g)) return W3_SLICES + (W3_SLICES + kSlabGroup - 1) / kSlabGroup;
  if (conv2_wgrad_f32_ok(g)) return W2_SLICES + (W2_SLICES + kSlabGroup - 1) / kSlabGroup;
  const int64_t chunk = wgrad_chunk(g);
  const int64_t nchunks = (g.B + chunk - 1) / chunk;
  const int slices = static_cast<int>(nchunks) *
                     wgrad_slices(g.Kout, g.C * g.R * g.R, chunk * static_cast<int64_t>(g.OH) * g.OW);
  return slices + (slices + kSlabGroup - 1) / kSlabGroup;  // + room for the stage-1 group sums
}

void conv_f32_wgrad(const ConvF32Geom& g, const float* dz, const float* x, const unsigned char* xu8, float mean,
                    float inv_std, float* slab, int slices, float* dw, float* db, hipStream_t s, F32RedList* defer) {
  auto reduce = [&](int n, int Kout, int Nw, int ncol) {
    if (defer)
      defer->push_back(F32RedSeg{slab, n, Kout, Nw, ncol, dw, db});
    else
      f32_slab_reduce(slab, n, Kout, Nw, ncol, dw, db, s);
  };
  const int Nw = g.C * g.R * g.R;
  const int ncol = Nw + (db ? 1 : 0);
  if (!xu8 && db && conv3_wgrad_f32_ok(g)) {  // the ConvNet's conv3 / conv2 at large batches: dedicated kernels
    hipLaunchKernelGGL(conv3_wgrad_f32_kernel, dim3(4 * W3_SLICES), dim3(256), 0, s, dz, x, slab,
                       static_cast<int>(g.B));
    reduce(W3_SLICES, g.Kout, Nw, ncol);
    return;
  }
  if (!xu8 && db && conv2_wgrad_f32_ok(g)) {
    hipLaunchKernelGGL(conv2_wgrad_f32_kernel, dim3(2 * W2_SLICES), dim3(256), 0, s, dz, x, slab,
                       static_cast<int>(g.B));
    reduce(W2_SLICES, g.Kout, Nw, ncol);
    return;
  }
  const int64_t zin = static_cast<int64_t>(g.Kout) * g.OH * g.OW;
  const int64_t chunk = wgrad_chunk(g);
  const int ohw = g.OH * g.OW;
  int used = 0;
  for (int64_t b0 = 0; b0 < g.B; b0 += chunk) {
    const int nb = static_cast<int>(std::min(chunk, g.B - b0));
    const int K = nb * ohw;
    const int sl = wgrad_slices(g.Kout, Nw, static_cast<int64_t>(chunk) * ohw);
    int per = (K + sl - 1) / sl;
    per = (per + BK - 1) / BK * BK;
    const int used_sl = (K + per - 1) / per;
    // GEMM columns = the Nw weights; the bias column (ncol - 1) comes from the dz row sums
    WgradA la{{dz + b0 * zin, static_cast<int>(nb * zin * 4), 0.f, 1.f}, g.Kout, ohw, make_fdiv(ohw)};
    SlabOut epi{slab + static_cast<int64_t>(used) * g.Kout * ncol, ncol, g.Kout};
    const int bias_col = db ? Nw : -1;
    with_wgrad_b(g, x, xu8, mean, inv_std, b0, nb,
                 [&](const auto& lb) { launch_gemm(g.Kout, Nw, K, per, used_sl, bias_col, la, lb, epi, s); });
    used += used_sl;
  }
  // the slab holds conv_f32_wgrad_slices(g) = (slices of all chunks) + their group count >= used + groups
  (void)slices;
  reduce(used, g.Kout, Nw, ncol);
}

int f32_slab_capacity(int slices) { return slices + (slices + kSlabGroup - 1) / kSlabGroup; }

void f32_slab_reduce(float* slab, int slices, int Kout, int Nw, int ncol, float* dw, float* db, hipStream_t s) {
  const int total = Kout * ncol;
  const float* src = slab;
  int nsum = slices;
  if (slices > kSlabGroup) {
    float* part = slab + static_cast<int64_t>(slices) * total;
    nsum = (slices + kSlabGroup - 1) / kSlabGroup;
    hipLaunchKernelGGL(slab_group_kernel, dim3((total + 255) / 256, nsum), dim3(256), 0, s, slab, slices, total,
                       part);
    src = part;
  }
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_1d(total)), dim3(256), 0, s, src, nsum, Kout, Nw, ncol, dw, db);
}

void f32_slab_reduce_multi(const F32RedList& segs, hipStream_t s) {
  if (segs.empty()) return;
  if ((int)segs.size() > kF32RedMax) {
    for (const auto& g : segs)
      f32_slab_reduce(const_cast<float*>(g.slab), g.slices, g.Kout, g.Nw, g.ncol, g.dw, g.db, s);
    return;
  }
  F32RedArgs a{};
  a.n = static_cast<int>(segs.size());
  int blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    a.seg[i] = segs[i];
    a.bstart[i] = blocks;
    const int total = segs[i].Kout * segs[i].ncol;
    const int per = segs[i].slices <= kSlabGroup ? 256 : kRedElems;  // the kernel's two workgroup kinds
    blocks += (total + per - 1) / per;
  }
  for (int i = a.n; i < kF32RedMax; ++i) a.bstart[i] = blocks;
  const int grid = blocks;
  hipLaunchKernelGGL(f32_reduce_multi_kernel, dim3(grid), dim3(256), 0, s, a);
}

}  // namespace ringdp::kern
