// fp32 ConvNet forward: the implicit-GEMM conv (+ fused pool) launchers, the dedicated conv2 / conv3 + pool
// kernels, fc1 at small batches and the split-K pooled forward (design: conv_f32_gemm.h).
#include "conv_f32_gemm.h"

namespace ringdp::kern {
namespace {

// ReLU + 2x2 max-pool (stride st) over the split-K planes of a plain NCHW conv output: each window value is
// the in-order sum of its slices plus the bias (bias before the max, as PoolOut / PoolS1Out), the first maximum
// in window order wins, code 255 where the result is 0.  One thread per pooled output.
// SC: the slice count at compile time (all 4 x SC loads of a window issued together), 0: run-time slices
template <int SC>
__global__ __launch_bounds__(256) void pool_slab_fwd_kernel(const float* __restrict__ slab, int slices_rt, int plane,
                                                            const float* __restrict__ bias, int C, int OH, int OW,
                                                            int st, int PH, int PW, int total, float* __restrict__ a,
                                                            unsigned char* __restrict__ code) {
  const int o = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (o >= total) return;
  const int px = o % PW;
  int t = o / PW;
  const int py = t % PH;
  t /= PH;
  const int n = t % C;
  const int base = t * OH * OW + py * st * OW + px * st;  // t = b * C + n
  const float bn = bias ? bias[n] : 0.f;
  const int slices = SC > 0 ? SC : slices_rt;
  float best = 0.f;
  int bt = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = base + (u >> 1) * OW + (u & 1);
    float v = slab[i];
#pragma unroll
    for (int z = 1; z < (SC > 0 ? SC : 1); ++z) v += slab[static_cast<int64_t>(z) * plane + i];
    if (SC == 0)
      for (int z = 1; z < slices; ++z) v += slab[static_cast<int64_t>(z) * plane + i];
    v += bn;
    if (u == 0 || v > best) {
      best = v;
      bt = u;
    }
  }
  const bool live = best > 0.f;
  a[o] = live ? best : 0.f;
  code[o] = live ? static_cast<unsigned char>(bt) : 255;
}

// Linear layer with few outputs (the ConvNet's fc1: N = 10, K = 2048) at small batches: the GEMM core's
// single 128-row tile ran K serially in one workgroup (163 us at B=100).  One wave per input row: lane l
// accumulates k = l, l+64, ... for every output, then a fixed butterfly sums the lanes (deterministic).
template <int N>
__global__ __launch_bounds__(256) void linear_skinny_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ z,
                                                              int M, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (int64_t)row * K;
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float v = xr[k];
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = fmaf(v, w[(int64_t)n * K + k], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    float v = acc[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[n] = v;
  }
  if (lane < N) {
    float v = 0.f;
#pragma unroll
    for (int n = 0; n < N; ++n) v = lane == n ? acc[n] : v;
    z[(int64_t)row * N + lane] = v + (bias ? bias[lane] : 0.f);
  }
}

// The same with one 256-thread workgroup per row and 16-B loads (K % 4 == 0, 16-B aligned rows): each
// thread's chain is K / 1024 float4 steps instead of K / 64 scalar ones (B=100 fc1: 14.8 us -> see
// profiles/r05/fp32/); per-wave sums, then the 4 waves in order (deterministic).
template <int N>
__global__ __launch_bounds__(256) void linear_row_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ z,
                                                             int K) {
  __shared__ float red[4][N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x;
  const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)row * K);
  const int K4 = K >> 2;
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.f;
  for (int k = tid; k < K4; k += 256) {
    const float4 v = xr[k];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const float4 q = reinterpret_cast<const float4*>(w + (int64_t)n * K)[k];
      acc[n] = fmaf(v.x, q.x, fmaf(v.y, q.y, fmaf(v.z, q.z, fmaf(v.w, q.w, acc[n]))));
    }
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    float v = acc[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][n] = v;
  }
  __syncthreads();
  if (tid < N) z[(int64_t)row * N + tid] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + (bias ? bias[tid] : 0.f);
}

// The forward A operand of images [b0, b0 + nb), M rows, by input kind - raw uint8 pixels (never with MODE 2), a
// padded fp32 input or a valid one - handed to `launch` (a generic lambda around the GEMM launch).  MODE, `ow`: FwdA.
template <int MODE, class F>
void with_fwd_a(const ConvF32Geom& g, const float* x, const unsigned char* xu8, float mean, float inv_std, int64_t b0,
                int nb, int M, FastDiv ow, F&& launch) {
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W;
  const int K = g.C * g.R * g.R, xbytes = static_cast<int>(nb * xin);
  const FastDiv ohw = make_fdiv(g.OH * g.OW);
  if constexpr (MODE != 2)
    if (xu8)
      return launch(FwdA<true, true, MODE>{{xu8 + b0 * xin, xbytes, mean, inv_std}, g.C, g.H, g.W, g.R, g.pad, g.OW, K, M, ohw, ow});
  if (g.pad) launch(FwdA<false, true, MODE>{{x + b0 * xin, xbytes * 4, 0.f, 1.f}, g.C, g.H, g.W, g.R, g.pad, g.OW, K, M, ohw, ow});
  else launch(FwdA<false, false, MODE>{{x + b0 * xin, xbytes * 4, 0.f, 1.f}, g.C, g.H, g.W, g.R, g.pad, g.OW, K, M, ohw, ow});
}

}  // namespace

void conv_f32_fwd(const ConvF32Geom& g, const float* x, const unsigned char* xu8, float mean, float inv_std,
                  const float* w, const float* bias, float* z, hipStream_t s) {
  const int K = g.C * g.R * g.R;
  if (!xu8 && g.R == 1 && g.H == 1 && g.W == 1 && g.Kout == 10 && g.B <= 8192) {  // fc1 at small batches
    if (K % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0)
      linear_row_f32_kernel<10><<<static_cast<unsigned>(g.B), 256, 0, s>>>(x, w, bias, z, K);
    else
      linear_skinny_f32_kernel<10><<<static_cast<unsigned>((g.B + 3) / 4), 256, 0, s>>>(x, w, bias, z,
                                                                                       static_cast<int>(g.B), K);
    return;
  }
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W, zout = static_cast<int64_t>(g.Kout) * g.OH * g.OW;
  const int64_t chunk = batch_chunk(g.B, {xin, zout});
  for (int64_t b0 = 0; b0 < g.B; b0 += chunk) {
    const int nb = static_cast<int>(std::min(chunk, g.B - b0));
    const int M = nb * g.OH * g.OW;
    WeightB lb{{w, K * g.Kout * 4, 0.f, 1.f}, K, g.Kout};
    NCHWOut epi{z + b0 * zout, bias, g.Kout, M, make_fdiv(g.OH * g.OW)};
    with_fwd_a<0>(g, x, xu8, mean, inv_std, b0, nb, M, make_fdiv(g.OW),
                  [&](const auto& la) { launch_gemm(M, g.Kout, K, K, 1, -1, la, lb, epi, s); });
  }
}

// ---------------------------------------------------------------- conv3 + ReLU + pool3 forward (fp32)
// The ConvNet's conv3 (64 -> 128 channels, 3x3 valid, 10x10 -> 8x8) with bias, ReLU and the 2x2/s2 max-pool
// (-> 4x4, + the argmax code of pool_relu / PoolOut) as one persistent 512-thread workgroup per CU.  Its
// 128 x 576 weights (295 KB) do not fit in LDS but do fit in the 8 waves' registers: wave w owns output
// channels [16 w, +16) and holds their whole K (144 k-steps of 4, tap-major: k = 64 tap + ci) as B operands,
// 144 VGPRs per lane, loaded once per launch.  Per image the waves share one LDS copy of the input (64
// channels x 10 x 10, row stride 112 floats = 16 banks apart, so the two channel rows of a b32 read never
// collide) and each runs 4 m-tiles x 144 k-steps with 4 independent accumulators.  The m-tile rows are
// window-major (row r of tile t: window 4 (r / 4) + t, tap r % 4), so a lane's 4 accumulator registers of
// tile t are the 4 pixels of window 4 lk + t: the pool is a register reduction and a lane's 4 tiles give 4
// consecutive pooled outputs of one channel (one float4 + one dword of codes per lane and image).
// The next image's input is loaded into registers during the k loop and stored to the other LDS buffer.
namespace {
constexpr int C3P_S = 112;  // floats per input channel row in LDS (100 + 12; 112 = 16 mod 32)

__global__ __launch_bounds__(512, 1) void conv3_pool_f32_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ bias,
                                                                float* __restrict__ a,
                                                                unsigned char* __restrict__ code, int B) {
  __shared__ __attribute__((aligned(16))) float XI[2][64 * C3P_S];  // 2 x 28 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int co = 16 * wave + lr;
  // B[k = 4 ks + lk][n = lr] = w[co][ci = 4 (ks & 15) + lk][tap = ks >> 4]
  float wr[144];
  {
    const float* wc = w + co * 576;
#pragma unroll
    for (int ks = 0; ks < 144; ++ks) wr[ks] = wc[(4 * (ks & 15) + lk) * 9 + (ks >> 4)];
  }
  const float bv = bias[co];
  // A: row lr of m-tile t = pixel (2 (lr >> 2) + ((lr >> 1) & 1), 2 t + (lr & 1)) of channel 4 (ks & 15) + lk
  int abase[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) abase[t] = lk * C3P_S + (2 * (lr >> 2) + ((lr >> 1) & 1)) * 10 + 2 * t + (lr & 1);
  auto koff = [](int ks) { const int tap = ks >> 4; return 4 * (ks & 15) * C3P_S + (tap / 3) * 10 + tap % 3; };
  // staging: an image is 1600 float4 (channel e / 25, column 4 (e % 25)); threads take 3 or 4 (named
  // registers: an array of them was left on the scratch stack)
  float4 st0, st1, st2, st3;
  auto load = [&](int b) {
    const float4* src = reinterpret_cast<const float4*>(x + (int64_t)b * 6400) + tid;
    st0 = src[0];
    st1 = src[512];
    st2 = src[1024];
    st3 = src[tid < 64 ? 1536 : 0];
  };
  auto put = [&](float* buf, int e, const float4& v) {
    const int c = e / 25, q = 4 * (e - 25 * c);
    *reinterpret_cast<float4*>(buf + c * C3P_S + q) = v;
  };
  auto stash = [&](float* buf) {
    put(buf, tid, st0);
    put(buf, tid + 512, st1);
    put(buf, tid + 1024, st2);
    if (tid < 64) put(buf, tid + 1536, st3);
  };
  int b = blockIdx.x;
  if (b < B) {
    load(b);
    stash(XI[0]);
  }
  __syncthreads();
  int cur = 0;
  for (; b < B; b += gridDim.x) {
    const int nb = b + gridDim.x;
    if (nb < B) load(nb);  // lands during the k loop
    const float* X = XI[cur];
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{bv, bv, bv, bv};
    // k-step-major: the next k-step's 4 A reads issued ahead of this one's 4 MFMAs
    float av[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) av[t] = X[abase[t] + koff(0)];
#pragma unroll
    for (int ks = 0; ks < 144; ++ks) {
      float an[4];
      if (ks + 1 < 144) {
#pragma unroll
        for (int t = 0; t < 4; ++t) an[t] = X[abase[t] + koff(ks + 1)];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], wr[ks], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < 144) {
#pragma unroll
        for (int t = 0; t < 4; ++t) av[t] = an[t];
      }
    }
    // lane: D[row 4 lk + r][co] of tile t = window 4 lk + t, tap r (row-major in the window)
    float o[4];
    uint32_t cw = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 v = acc[t];
      const float best = fmaxf(fmaxf(fmaxf(v[0], v[1]), v[2]), v[3]);
      const uint32_t arg = v[0] == best ? 0u : v[1] == best ? 1u : v[2] == best ? 2u : 3u;  // first maximum
      const bool live = best > 0.f;
      o[t] = live ? best : 0.f;
      cw |= (live ? arg : 255u) << (8 * t);
    }
    reinterpret_cast<float4*>(a + (int64_t)b * 2048 + co * 16)[lk] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<uint32_t*>(code + (int64_t)b * 2048 + co * 16)[lk] = cw;
    if (nb < B) stash(XI[cur ^ 1]);
    __syncthreads();  // the next image staged; this one's reads done before it is overwritten next round
    cur ^= 1;
  }
}
}  // namespace

// smallest batch that takes the dedicated conv2 / conv3 forward kernels (one image per workgroup at a time)
// instead of split K + pool_slab_fwd: 4 images per CU
static int f32_fwd_dedicated_min_b() { return 4 * f32_num_cus(); }

static bool conv3_pool_f32_ok(const ConvF32Geom& g) {
  return is_convnet_conv3(g) && g.B >= f32_fwd_dedicated_min_b() && g.B * 6400 < (int64_t{1} << 31);
}

void conv_f32_fwd_pool(const ConvF32Geom& g, const float* x, const unsigned char* xu8, float mean, float inv_std,
                       const float* w, const float* bias, float* a, unsigned char* code, hipStream_t s) {
  const int K = g.C * g.R * g.R;
  if (bias && !xu8 && conv3_pool_f32_ok(g)) {  // the ConvNet's conv3 at large batches: the dedicated kernel
    const int grid = static_cast<int>(std::min<int64_t>(g.B, f32_num_cus()));
    hipLaunchKernelGGL(conv3_pool_f32_kernel, dim3(grid), dim3(512), 0, s, x, w, bias, a, code, static_cast<int>(g.B));
    return;
  }
  const int phw = (g.OH / 2) * (g.OW / 2);
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W, aout = static_cast<int64_t>(g.Kout) * phw;
  const int64_t chunk = batch_chunk(g.B, {xin, static_cast<int64_t>(g.Kout) * g.OH * g.OW});
  for (int64_t b0 = 0; b0 < g.B; b0 += chunk) {
    const int nb = static_cast<int>(std::min(chunk, g.B - b0));
    const int M = nb * g.OH * g.OW;
    WeightB lb{{w, K * g.Kout * 4, 0.f, 1.f}, K, g.Kout};
    PoolOut epi{a + b0 * aout, code + b0 * aout, bias, g.Kout, M, phw, make_fdiv(g.OH * g.OW)};
    with_fwd_a<1>(g, x, xu8, mean, inv_std, b0, nb, M, make_fdiv(g.OW / 2),
                  [&](const auto& la) { launch_gemm(M, g.Kout, K, K, 1, -1, la, lb, epi, s); });
  }
}

// ---------------------------------------------------------------- conv2 + ReLU + pool2 forward (fp32)
// The ConvNet's conv2 (32 -> 64 channels, 3x3 valid, 13x13 -> 11x11) with bias, ReLU and the overlapping 2x2/s1
// max-pool (+ its argmax code, pool2s1_fwd_kernel semantics) as one persistent kernel, two 256-thread
// workgroups per CU.  Wave w owns output channels [16 w, +16) with its 16 x 288 weights resident in registers
// (72 per lane); K runs tap-major (k = 32 tap + ci), so an A fragment - 16 positions x 4 input channels of one
// tap - is one b32 read of the LDS image at a per-lane base + a compile-time offset (no index math in the
// loop).  The 121 positions are 8 tiles of 16 (the last 7 rows read the image's tail and are never stored).
// Epilogue: conv + bias to an LDS tile, then pool + ReLU + code, 4 outputs (float4 / 4 code bytes) per thread.
namespace {
constexpr int C2F_ZS = 121 + 3;  // floats per channel row of the conv output tile

__global__ __launch_bounds__(256, 2) void conv2_pool_f32_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ bias,
                                                                 float* __restrict__ a,
                                                                 unsigned char* __restrict__ code, int B) {
  __shared__ __attribute__((aligned(16))) float XI[5408 + 128];     // 22.1 KB: the input image (+ tail)
  __shared__ __attribute__((aligned(16))) float Z[64 * C2F_ZS];     // 31.7 KB: conv + bias
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  // weights: lane holds B[k = 4 ks + lk][co = 16 wave + lr] = w[co][ci = (4 ks + lk) & 31][tap = ks >> 3]
  float wr[72];
  {
    const float* wc = w + (16 * wave + lr) * 288;
#pragma unroll
    for (int ks = 0; ks < 72; ++ks) wr[ks] = wc[((4 * ks + lk) & 31) * 9 + (ks >> 3)];
  }
  const float bv = bias[16 * wave + lr];
  // A base per position tile: lane row p = 16 i + lr -> (oy, ox); + the input channel lk
  int pbase[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = min(16 * i + lr, 120);  // rows past 120: a real pixel, product never stored
    pbase[i] = lk * 169 + (p / 11) * 13 + p % 11;
  }
  // staging: the image is 5408 floats = 1352 float4, 5 or 6 per thread, loaded into named registers one image
  // ahead (in flight during the k loop) and stored after the pool phase
  float4 s0, s1, s2, s3, s4, s5;
  auto load = [&](int b) {
    const float4* src = reinterpret_cast<const float4*>(x + (int64_t)b * 5408) + tid;
    s0 = src[0];
    s1 = src[256];
    s2 = src[512];
    s3 = src[768];
    s4 = src[1024];
    s5 = src[tid < 72 ? 1280 : 0];
  };
  auto stash = [&]() {
    float4* d = reinterpret_cast<float4*>(XI) + tid;
    d[0] = s0;
    d[256] = s1;
    d[512] = s2;
    d[768] = s3;
    d[1024] = s4;
    if (tid < 72) d[1280] = s5;
  };
  if (blockIdx.x < B) {
    load(blockIdx.x);
    stash();
  }
  __syncthreads();
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int nb = b + gridDim.x;
    if (nb < B) load(nb);
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = dev::zero_f32x4();
    // k-step-major with the next k-step's 8 A reads issued ahead of this one's 8 MFMAs (independent
    // accumulators back to back; left to itself the scheduler ran one position tile's 72 dependent MFMAs
    // in a row: 4.27 ms at B=65536)
    auto koff = [](int ks) { const int tap = ks >> 3; return 4 * (ks & 7) * 169 + (tap / 3) * 13 + tap % 3; };
    float av[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) av[i] = XI[pbase[i] + koff(0)];
#pragma unroll
    for (int ks = 0; ks < 72; ++ks) {
      float an[8];
      if (ks + 1 < 72) {
#pragma unroll
        for (int i = 0; i < 8; ++i) an[i] = XI[pbase[i] + koff(ks + 1)];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], wr[ks], acc[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < 72) {
#pragma unroll
        for (int i = 0; i < 8; ++i) av[i] = an[i];
      }
    }
    // lane holds D[p = 16 i + 4 lk + r][co = 16 wave + lr]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * i + 4 * lk + r;
        if (p < 121) Z[(16 * wave + lr) * C2F_ZS + p] = acc[i][r] + bv;
      }
    __syncthreads();
    // pool: quads of 4 consecutive outputs of one channel (100 per channel: never crossing a channel)
    float4* ao = reinterpret_cast<float4*>(a + (int64_t)b * 6400);
    uint32_t* co = reinterpret_cast<uint32_t*>(code + (int64_t)b * 6400);
    for (int qd = tid; qd < 1600; qd += 256) {
      const int ch = qd / 25, q0 = 4 * (qd - 25 * ch);
      float o[4];
      uint32_t cw = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = q0 + j, py = q / 10, px = q - 10 * py;
        const float* t = Z + ch * C2F_ZS + py * 11 + px;
        const float v0 = t[0], v1 = t[1], v2 = t[11], v3 = t[12];
        float best = v0;
        uint32_t arg = 0;
        if (v1 > best) { best = v1; arg = 1; }
        if (v2 > best) { best = v2; arg = 2; }
        if (v3 > best) { best = v3; arg = 3; }
        const bool live = best > 0.f;
        o[j] = live ? best : 0.f;
        cw |= (live ? arg : 255u) << (8 * j);
      }
      ao[qd] = make_float4(o[0], o[1], o[2], o[3]);
      co[qd] = cw;
    }
    if (nb < B) stash();  // XI was last read by the k loop, before the barrier above
    __syncthreads();  // Z free, the next image staged
  }
}
}  // namespace

static bool conv2_pool_f32_ok(const ConvF32Geom& g) {
  return is_convnet_conv2(g) && g.B >= f32_fwd_dedicated_min_b() && g.B * 6400 < (int64_t{1} << 31);
}

void conv_f32_fwd_pool_s1(const ConvF32Geom& g, const float* x, const float* w, const float* bias, float* a,
                          unsigned char* code, hipStream_t s) {
  if (bias && conv2_pool_f32_ok(g)) {  // the ConvNet's conv2 at large batches: the dedicated kernel
    const int grid = static_cast<int>(std::min<int64_t>(g.B, 2 * f32_num_cus()));
    hipLaunchKernelGGL(conv2_pool_f32_kernel, dim3(grid), dim3(256), 0, s, x, w, bias, a, code, static_cast<int>(g.B));
    return;
  }
  const int K = g.C * g.R * g.R;
  const int PH = g.OH - 1, PW = g.OW - 1, phw = PH * PW;
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W, aout = static_cast<int64_t>(g.Kout) * phw;
  const int64_t chunk = batch_chunk(g.B, {xin, int64_t{128} * g.Kout});
  for (int64_t b0 = 0; b0 < g.B; b0 += chunk) {
    const int nb = static_cast<int>(std::min(chunk, g.B - b0));
    const int M = nb * 128;
    WeightB lb{{w, K * g.Kout * 4, 0.f, 1.f}, K, g.Kout};
    PoolS1Out epi{a + b0 * aout, code + b0 * aout, bias, g.Kout, g.OW, PW, phw, make_fdiv(phw), make_fdiv(PW)};
    with_fwd_a<2>(g, x, nullptr, 0.f, 1.f, b0, nb, M, make_fdiv(g.OW),
                  [&](const auto& la) { launch_layout<4, 1, 2, 4>(M, g.Kout, K, K, 1, -1, la, lb, epi, s); });
  }
}

// Small batches, valid convs with a fused pool (the ConvNet's conv2 / conv3 at B=100: 100 one-image tiles x 18
// k-tiles, 800 32x32 tiles x 36 k-tiles, ~30 us each): the same k split as the data gradient
// (conv_f32_dgrad.hip), into planes of the plain conv output, then pool_slab_fwd_kernel sums, adds the bias and
// pools.  RINGDP_F32_FWD_SLICES=n forces n (1: the one-launch fused kernels).
int conv_f32_fwd_slices(const ConvF32Geom& g) {
  if (g.pad != 0 || conv2_pool_f32_ok(g) || conv3_pool_f32_ok(g)) return 1;
  const int K = g.C * g.R * g.R;
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W, zout = static_cast<int64_t>(g.Kout) * g.OH * g.OW;
  if (batch_chunk(g.B, {xin, zout}) < g.B) return 1;
  const int64_t M = g.B * g.OH * g.OW, plane = M * g.Kout;
  const int64_t tiles32 = ((M + 31) / 32) * ((g.Kout + 31) / 32);
  int s = tiles32 >= 8 * f32_num_cus() ? 1 : std::min(8, (K + 8 * BK - 1) / (8 * BK));
  if (const char* e = std::getenv("RINGDP_F32_FWD_SLICES")) {
    const int v = std::atoi(e);
    if (v > 0) s = v;
  }
  s = std::max(1, std::min(s, std::min(16, (K + BK - 1) / BK)));
  if (static_cast<int64_t>(s) * plane >= (int64_t{1} << 29)) return 1;
  return s;
}

void conv_f32_fwd_pool_split(const ConvF32Geom& g, const float* x, const float* w, const float* bias, float* slab,
                             int slices, int st, float* a, unsigned char* code, hipStream_t s) {
  const int K = g.C * g.R * g.R;
  const int M = static_cast<int>(g.B * g.OH * g.OW);
  const int plane = M * g.Kout;
  int per = (K + slices - 1) / slices;
  per = (per + BK - 1) / BK * BK;
  const int used = (K + per - 1) / per;
  const int64_t xin = static_cast<int64_t>(g.C) * g.H * g.W;
  WeightB lb{{w, K * g.Kout * 4, 0.f, 1.f}, K, g.Kout};
  FwdA<false, false> la{{x, static_cast<int>(g.B * xin * 4), 0.f, 1.f}, g.C, g.H, g.W, g.R, g.pad, g.OW, K, M,
                        make_fdiv(g.OH * g.OW), make_fdiv(g.OW)};
  NCHWSlabOut epi{slab, g.Kout, M, plane, make_fdiv(g.OH * g.OW)};
  launch_gemm(M, g.Kout, K, per, used, -1, la, lb, epi, s);
  const int PH = st == 2 ? g.OH / 2 : g.OH - 1, PW = st == 2 ? g.OW / 2 : g.OW - 1;
  const int total = static_cast<int>(g.B) * g.Kout * PH * PW;
  const dim3 grid((total + 255) / 256);
#define RINGDP_POOL_SLAB(SCV)                                                                                         \
  hipLaunchKernelGGL(pool_slab_fwd_kernel<SCV>, grid, dim3(256), 0, s, slab, used, plane, bias, g.Kout, g.OH, g.OW, st, \
                     PH, PW, total, a, code)
  switch (used) {
    case 2: RINGDP_POOL_SLAB(2); break;
    case 3: RINGDP_POOL_SLAB(3); break;
    case 4: RINGDP_POOL_SLAB(4); break;
    case 5: RINGDP_POOL_SLAB(5); break;
    case 6: RINGDP_POOL_SLAB(6); break;
    case 8: RINGDP_POOL_SLAB(8); break;
    default: RINGDP_POOL_SLAB(0); break;
  }
#undef RINGDP_POOL_SLAB
}

}  // namespace ringdp::kern
