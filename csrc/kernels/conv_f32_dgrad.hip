// fp32 ConvNet data gradients: the implicit-GEMM launchers (one slice, or split K + a fixed-order plane sum, also
// fused with pool2's backward) and the dedicated scatter-form conv2 / conv3 kernels (design: conv_f32_gemm.h).
#include "conv_f32_gemm.h"

namespace ringdp::kern {
namespace {

// dx = sum over the split-K planes of NCHWSlabOut, in plane order (deterministic); n4 = plane / 4
__global__ __launch_bounds__(256) void slab_sum_kernel(const float4* __restrict__ slab, int slices, int n4,
                                                       float4* __restrict__ out) {
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < n4;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    float4 acc = slab[i];
    for (int z = 1; z < slices; ++z) {
      const float4 v = slab[static_cast<int64_t>(z) * n4 + i];
      acc.x += v.x;
      acc.y += v.y;
      acc.z += v.z;
      acc.w += v.w;
    }
    out[i] = acc;
  }
}

}  // namespace

// Small batches (the reference's 100 images): the data-gradient GEMM has few workgroups, each with one long k
// loop that is latency-bound (B=100 conv3: 626 workgroups of 32x32 x 72 k-tiles, 63 us).  Split K into slices
// of ~8 k-tiles (at most 8 slices): the grid then takes the big-tile layouts again (fewer gathers per MFMA)
// and the slices' partial dx planes are summed in order by slab_sum_kernel.  B=100 step, forced counts
// (profiles/r05/fp32/): 1 slice 353 us, 2: 353, 3: 342, 4: 329, 6: 313, 8: 312, 12: 317.  At least 6 slices on the
// round-6 step (conv2's 18 k-tiles had 3): 209 -> 207 us (forced 4: 220, 10: 207;
// profiles/r06/fp32/b100_slices_sweep.txt).  Big batches (>= 8 32x32 tiles per CU) and chunked batches keep one
// slice.  RINGDP_F32_DGRAD_SLICES=n forces n (1: off).
int conv_f32_dgrad_slices(const ConvF32Geom& g) {
  const int K = g.Kout * g.R * g.R;
  const int64_t zin = static_cast<int64_t>(g.Kout) * g.OH * g.OW, xout = static_cast<int64_t>(g.C) * g.H * g.W;
  if (batch_chunk(g.B, {zin, xout}) < g.B) return 1;
  const int64_t M = g.B * g.H * g.W, plane = M * g.C;
  if (plane % 4 != 0) return 1;
  const int64_t tiles32 = ((M + 31) / 32) * ((g.C + 31) / 32);
  int s = tiles32 >= 8 * f32_num_cus() ? 1 : std::min(8, std::max(6, (K + 8 * BK - 1) / (8 * BK)));
  if (const char* e = std::getenv("RINGDP_F32_DGRAD_SLICES")) {
    const int v = std::atoi(e);
    if (v > 0) s = v;
  }
  s = std::max(1, std::min(s, std::min(16, (K + BK - 1) / BK)));
  if (static_cast<int64_t>(s) * plane >= (int64_t{1} << 29)) return 1;
  return s;
}

// ---------------------------------------------------------------- conv3 data gradient, scatter form
// The ConvNet's conv3 (64 -> 128 channels, 3x3 valid, 10x10 -> 8x8) data gradient as one GEMM per kernel tap
// over the LIVE positions only: P_t[p][ci] = sum_co dz[co][p] * w[co][ci][t] (p over the 8x8 dz positions),
// scattered into dx[ci][p + (kh, kw)].  The implicit-GEMM path correlates the zero-padded 12x12 dz against
// the 10x10 output, and 36 % of its MACs multiply padding (profiles/r05/fp32/).
// One 256-thread workgroup per CU, persistent over images; wave w owns the 16 input channels
// [16 w, 16 w + 16) for all 9 taps and all 64 positions, so every A fragment (4 co x 16 positions) read from
// LDS feeds 9 MFMAs and no two waves write the same dx element.  The weights stay in L2: a lane streams its
// 9 tap values per k-step (3 x 16 B, repacked once per call into [wave][k-step][lane][12]) two k-steps ahead.
// col2im: tap by tap (fixed order: deterministic) into a wave-private fp32 LDS image, then stored
// coalesced - the wave's 16 x 100 outputs are one contiguous NCHW run.  The next image's dz (32 KB) is loaded
// into registers while this one multiplies and stashed to the other LDS buffer behind the same barrier (loads
// are counted in order, so the first weight wait also waits for that HBM round trip; issued after the k-loop
// instead, the stash waited for it: 5.9 -> 6.6 ms at B=65536).
// Exact fp32 MFMA (v_mfma_f32_16x16x4_f32): results differ from the GEMM path only by summation order.
constexpr int D3_AS = 80;   // floats per co row of the staged dz image (64 + 16: the 2 k rows of a b32 read
                            // land 16 banks apart)
constexpr int D3_XS = 101;  // floats per channel row of a wave's dx image (odd: the 16 channel rows of a
                            // b32 RMW hit 16 distinct banks)
constexpr int D3_WP = 4 * 32 * 9 * 64;  // repacked weights (floats): [wave][k-step][tap][lane]

__global__ __launch_bounds__(256) void d3_repack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D3_WP) return;
  const int lane = i & 63, t = (i >> 6) % 9, ks = (i / 576) & 31, ct = i / 18432;
  const int co = ks * 4 + (lane >> 4), ci = ct * 16 + (lane & 15);
  wp[i] = w[(co * 64 + ci) * 9 + t];
}

__global__ __launch_bounds__(256, 2) void conv3_dgrad_f32_kernel(const float* __restrict__ dz,
                                                                  const float* __restrict__ wp,
                                                                  float* __restrict__ dx, int B) {
  __shared__ __attribute__((aligned(16))) float A[1][128 * D3_AS];   // 40 KB (two workgroups per CU)
  __shared__ __attribute__((aligned(16))) float X[4][16 * D3_XS];   // 25.9 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const float* wl = wp + wave * 32 * 576 + lane;  // + (k-step * 9 + tap) * 64
  float* xw = X[wave];
  // an image's dz into the staging buffer: this thread's 8 float4 (2048 float4: co = e / 16, column 4 (e % 16)),
  // all loads issued before the first store
  auto copy_img = [&](int b, float* buf) {
    const float4* src = reinterpret_cast<const float4*>(dz + (int64_t)b * 8192) + tid;
    // named registers, not an array: the array form was left on the scratch stack
    const float4 r0 = src[0], r1 = src[256], r2 = src[512], r3 = src[768], r4 = src[1024], r5 = src[1280],
                 r6 = src[1536], r7 = src[1792];
    float* d = buf + (tid >> 4) * D3_AS + (tid & 15) * 4;  // + 16 co rows per 256 float4
    *reinterpret_cast<float4*>(d + 0 * 16 * D3_AS) = r0;
    *reinterpret_cast<float4*>(d + 1 * 16 * D3_AS) = r1;
    *reinterpret_cast<float4*>(d + 2 * 16 * D3_AS) = r2;
    *reinterpret_cast<float4*>(d + 3 * 16 * D3_AS) = r3;
    *reinterpret_cast<float4*>(d + 4 * 16 * D3_AS) = r4;
    *reinterpret_cast<float4*>(d + 5 * 16 * D3_AS) = r5;
    *reinterpret_cast<float4*>(d + 6 * 16 * D3_AS) = r6;
    *reinterpret_cast<float4*>(d + 7 * 16 * D3_AS) = r7;
  };
  int b = blockIdx.x;
  if (b < B) copy_img(b, A[0]);
  __syncthreads();
  for (; b < B; b += gridDim.x) {
    const int nb = b + gridDim.x;
    const float* a_img = A[0];
    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] = dev::zero_f32x4();
    // weights: two register sets, each reloaded right after its MFMAs were issued, for the k-step two ahead
    // (one coalesced 256-B dword load per tap, straight into the registers the MFMAs read).  The reloads are
    // unconditional (the last two read past this wave's k-steps: the next wave's, or the buffer's pad) and
    // pinned behind their k-step's MFMAs (sched_barrier), so each wait covers only the set about to be used
    // and every load has a whole k-step (36 MFMAs, ~1150 cycles) to arrive.
    float wa[9], wb[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      wa[t] = wl[t * 64];
      wb[t] = wl[(9 + t) * 64];
    }
    auto kstep = [&](int ks, const float (&wt)[9]) {
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = a_img[(ks * 4 + lk) * D3_AS + 16 * i + lr];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)  // rows: positions 16 i + (lane & 15); columns: channels
          acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wt[t], acc[t][i], 0, 0, 0);
    };
#pragma unroll 1
    for (int ks = 0; ks < 32; ks += 2) {
      kstep(ks, wa);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) wa[t] = wl[((ks + 2) * 9 + t) * 64];
      __builtin_amdgcn_sched_barrier(0);
      kstep(ks + 1, wb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) wb[t] = wl[((ks + 3) * 9 + t) * 64];
      __builtin_amdgcn_sched_barrier(0);
    }
    // col2im into the wave's dx image: lane holds P_t[p = 16 i + 4 lk + r][ci = lr].  Lanes share
    // destinations across taps (the x = 4, 5 columns of lanes with lk even and odd), which the compiler's
    // per-thread alias analysis cannot see: a memory clobber between the phases keeps the wave's LDS
    // operations in program order (one wave's LDS operations then complete in order).
    for (int e = lane; e < 16 * D3_XS; e += 64) xw[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      asm volatile("" ::: "memory");
      const int kh = t / 3, kw = t % 3;
      float v[16];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 16 * i + 4 * lk + r;
          v[4 * i + r] = xw[lr * D3_XS + ((p >> 3) + kh) * 10 + (p & 7) + kw];
        }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 16 * i + 4 * lk + r;
          xw[lr * D3_XS + ((p >> 3) + kh) * 10 + (p & 7) + kw] = v[4 * i + r] + acc[t][i][r];
        }
    }
    asm volatile("" ::: "memory");
    // the wave's 16 channels x 100 positions: one contiguous run of dx
    float* out = dx + (int64_t)b * 6400 + wave * 1600;
    for (int e = lane; e < 1600; e += 64) {
      const int c = e / 100;
      out[e] = xw[c * D3_XS + (e - 100 * c)];
    }
    asm volatile("" ::: "memory");
    __syncthreads();  // every wave's k loop has read this image
    // the next image's dz straight through registers into the single buffer: the round trip is exposed to
    // this workgroup only; the CU's other workgroup keeps the matrix cores busy meanwhile
    if (nb < B) copy_img(nb, A[0]);
    __syncthreads();
  }
}

// conv2 (32 -> 64 channels, 3x3 valid, 13x13 -> 11x11): its data gradient in the same scatter form.  dz2 has
// 121 positions (8 tiles of 16, the last 7 rows padding: never scattered); wave w owns input channels
// [16 (w & 1), +16) for positions [64 (w >> 1), +64), so the two waves of a channel tile write overlapping
// output rows: each scatters into its own LDS image and the pair is summed in a fixed order on the way out.
constexpr int D2_XS = 171;                  // floats per channel row of a wave's 13x13 image (odd)
constexpr int D2_WP = 2 * 16 * 9 * 64;      // repacked weights: [ci tile][k-step][tap][lane]

__global__ __launch_bounds__(256) void d2_repack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D2_WP) return;
  const int lane = i & 63, t = (i >> 6) % 9, ks = (i / 576) & 15, ct = i / 9216;
  const int co = ks * 4 + (lane >> 4), ci = ct * 16 + (lane & 15);
  wp[i] = w[(co * 32 + ci) * 9 + t];
}

__global__ __launch_bounds__(256, 2) void conv2_dgrad_f32_kernel(const float* __restrict__ dz,
                                                                  const float* __restrict__ wp,
                                                                  float* __restrict__ dx, int B) {
  __shared__ __attribute__((aligned(16))) float A[1][64 * 121 + 128];  // 31 KB (+ readable padding rows)
  __shared__ __attribute__((aligned(16))) float X[4][16 * D2_XS + 32];  // 44.3 KB (+ a dump row per wave)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4, ct = wave & 1, half = wave >> 1;
  const float* wl = wp + ct * 16 * 576 + lane;  // + (k-step * 9 + tap) * 64
  float* xw = X[wave];
  // per (tile i, row r) of this lane: the image offset (channel row included) of its dz position
  // p = 64 half + 16 i + 4 lk + r; past the 121 real positions the wave's dump row (branch-free col2im)
  int dst[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 64 * half + 16 * i + 4 * lk + r;
      dst[4 * i + r] = p < 121 ? lr * D2_XS + (p / 11) * 13 + p % 11 : 16 * D2_XS;
    }
  // an image of dz is 7744 contiguous floats = 1936 float4: threads take 7 or 8 of them (the loads are
  // unconditional, clamped to the image, so they all issue before the first store)
  auto copy_img = [&](int b, float* buf) {
    const float4* src = reinterpret_cast<const float4*>(dz + (int64_t)b * 7744) + tid;
    float4* d = reinterpret_cast<float4*>(buf) + tid;
    // named registers (an array was left on the scratch stack); the last one exists for tid < 144
    const float4 r0 = src[0], r1 = src[256], r2 = src[512], r3 = src[768], r4 = src[1024], r5 = src[1280],
                 r6 = src[1536], r7 = src[tid < 144 ? 1792 : 0];
    d[0] = r0;
    d[256] = r1;
    d[512] = r2;
    d[768] = r3;
    d[1024] = r4;
    d[1280] = r5;
    d[1536] = r6;
    if (tid < 144) d[1792] = r7;
  };
  int b = blockIdx.x;
  if (b < B) copy_img(b, A[0]);
  __syncthreads();
  for (; b < B; b += gridDim.x) {
    const int nb = b + gridDim.x;
    const float* a_img = A[0] + 64 * half;
    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] = dev::zero_f32x4();
    float wa[9], wb[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      wa[t] = wl[t * 64];
      wb[t] = wl[(9 + t) * 64];
    }
    // rows of dz: co = 4 ks + lk at 121 floats; positions 16 i + lr of this half (rows 121.. of the last
    // tile read padding / the next channel: their products are never scattered)
    auto kstep = [&](int ks, const float (&wt)[9]) {
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = a_img[(ks * 4 + lk) * 121 + 16 * i + lr];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wt[t], acc[t][i], 0, 0, 0);
    };
#pragma unroll 1
    for (int ks = 0; ks < 16; ks += 2) {  // as conv3_dgrad_f32_kernel: pinned, unconditional weight reloads
      kstep(ks, wa);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) wa[t] = wl[((ks + 2) * 9 + t) * 64];
      __builtin_amdgcn_sched_barrier(0);
      kstep(ks + 1, wb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) wb[t] = wl[((ks + 3) * 9 + t) * 64];
      __builtin_amdgcn_sched_barrier(0);
    }
    // col2im into this wave's image (cross-lane shared destinations: keep program order, see conv3)
    for (int e = lane; e < 16 * D2_XS; e += 64) xw[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      asm volatile("" ::: "memory");
      const int off = (t / 3) * 13 + t % 3;
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = xw[dst[q] + off];
#pragma unroll
      for (int q = 0; q < 16; ++q) xw[dst[q] + off] = v[q] + acc[t][q >> 2][q & 3];
    }
    __syncthreads();  // both halves of every channel tile scattered
    {
      // channel tile ct, elements [1352 half, +1352) of its 16 x 169 run: half 0's image + half 1's, in order
      const float* x0 = X[ct];
      const float* x1 = X[ct + 2];
      float* out = dx + (int64_t)b * 5408 + ct * 2704;
      for (int e = 1352 * half + lane; e < 1352 * (half + 1); e += 64) {
        const int c = e / 169, q = e - 169 * c;
        out[e] = x0[c * D2_XS + q] + x1[c * D2_XS + q];
      }
    }
    if (nb < B) copy_img(nb, A[0]);  // every k loop finished before the barrier above (see conv3)
    __syncthreads();  // images read out, next dz staged
  }
}

bool conv_dgrad_f32_scatter_ok(const ConvF32Geom& g) {
  // the persistent one-image-per-workgroup form needs images for every CU; small batches keep split K
  return (is_convnet_conv3(g) || is_convnet_conv2(g)) && g.B >= 2 * f32_num_cus() && g.B * 8192 < (int64_t{1} << 31);
}

void conv_dgrad_f32_scatter(const ConvF32Geom& g, const float* dz, const float* w, float* dx, float* wp,
                            hipStream_t s) {
  // two persistent workgroups per CU (single-buffered dz): one's col2im runs beside the other's MFMAs
  const int grid = static_cast<int>(std::min<int64_t>(g.B, 2 * f32_num_cus()));
  if (is_convnet_conv3(g)) {
    hipLaunchKernelGGL(d3_repack_kernel, dim3((D3_WP + 255) / 256), dim3(256), 0, s, w, wp);
    hipLaunchKernelGGL(conv3_dgrad_f32_kernel, dim3(grid), dim3(256), 0, s, dz, wp, dx, static_cast<int>(g.B));
  } else {
    hipLaunchKernelGGL(d2_repack_kernel, dim3((D2_WP + 255) / 256), dim3(256), 0, s, w, wp);
    hipLaunchKernelGGL(conv2_dgrad_f32_kernel, dim3(grid), dim3(256), 0, s, dz, wp, dx, static_cast<int>(g.B));
  }
}

int conv_dgrad_f32_scratch() { return D3_WP + 2 * 576; }  // the larger repack + the prefetch pad

// The split-K data-gradient GEMM (conv_f32_dgrad_slices(g) > 1: one chunk, plane % 4 == 0): slice z of K stores its
// partial dx into plane z of slab.  Returns the number of planes written.
static int dgrad_split_k(const ConvF32Geom& g, const float* dz, const float* w, float* slab, int slices,
                         hipStream_t s) {
  const int K = g.Kout * g.R * g.R;
  const int64_t zin = static_cast<int64_t>(g.Kout) * g.OH * g.OW;
  const int M = static_cast<int>(g.B * g.H * g.W);
  const int plane = M * g.C;
  int per = (K + slices - 1) / slices;
  per = (per + BK - 1) / BK * BK;
  const int used = (K + per - 1) / per;
  DgradA la{{dz, static_cast<int>(g.B * zin * 4), 0.f, 1.f}, g.Kout, g.W, g.R, g.OH, g.OW, g.pad, K, M,
            make_fdiv(g.H * g.W), make_fdiv(g.W)};
  DgradB lb{{w, K * g.C * 4, 0.f, 1.f}, g.C, g.R * g.R, K, make_fdiv(g.R * g.R)};
  NCHWSlabOut epi{slab, g.C, M, plane, make_fdiv(g.H * g.W)};
  launch_gemm(M, g.C, K, per, used, -1, la, lb, epi, s);
  return used;
}

void conv_f32_dgrad(const ConvF32Geom& g, const float* dz, const float* w, float* dx, float* slab, int slices,
                    hipStream_t s) {
  const int K = g.Kout * g.R * g.R;
  const int64_t zin = static_cast<int64_t>(g.Kout) * g.OH * g.OW, xout = static_cast<int64_t>(g.C) * g.H * g.W;
  if (slab && slices > 1) {
    const int used = dgrad_split_k(g, dz, w, slab, slices, s);
    const int n4 = static_cast<int>(g.B * xout / 4);
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_1d(n4)), dim3(256), 0, s, reinterpret_cast<const float4*>(slab),
                       used, n4, reinterpret_cast<float4*>(dx));
    return;
  }
  const int64_t chunk = batch_chunk(g.B, {zin, xout});
  for (int64_t b0 = 0; b0 < g.B; b0 += chunk) {
    const int nb = static_cast<int>(std::min(chunk, g.B - b0));
    const int M = nb * g.H * g.W;
    DgradA la{{dz + b0 * zin, static_cast<int>(nb * zin * 4), 0.f, 1.f}, g.Kout, g.W, g.R, g.OH, g.OW, g.pad, K,
              M, make_fdiv(g.H * g.W), make_fdiv(g.W)};
    DgradB lb{{w, K * g.C * 4, 0.f, 1.f}, g.C, g.R * g.R, K, make_fdiv(g.R * g.R)};
    NCHWOut epi{dx + b0 * xout, nullptr, g.C, M, make_fdiv(g.H * g.W)};
    launch_gemm(M, g.C, K, K, 1, -1, la, lb, epi, s);
  }
}

bool conv_f32_dgrad_pool2s1_ok(const ConvF32Geom& g) {
  const int64_t BC = g.B * g.C;
  return conv_f32_dgrad_slices(g) > 1 && !conv_dgrad_f32_scatter_ok(g) && g.H == 10 && g.W == 10 && BC % kP2Tile == 0;
}

void conv_f32_dgrad_pool2s1_bwd(const ConvF32Geom& g, const float* dz, const float* w, float* slab, int slices,
                                const unsigned char* code, float* dzp, hipStream_t s) {
  // conv_f32_dgrad's split-K GEMM into slab (its planes are the pool's da), then the tiled 2x2/s1 pool backward
  // summing the planes as it stages them: one launch fewer than dgrad + slab_sum + pool backward
  const int used = dgrad_split_k(g, dz, w, slab, slices, s);
  pool2s1_bwd_tile(slab, code, dzp, static_cast<int>(g.B * g.C / kP2Tile), g.H, g.W, used, g.B * g.C * g.H * g.W, s);
}

}  // namespace ringdp::kern
