// Depthwise K x K convolution on NHWC bf16 activations for gfx950 (the first layer of a ConvNeXt block): stride 1,
// dilation 1, "same" padding K / 2, K in {3, 5, 7}, C % 8 == 0.  Activations bf16 [N, H, W, C], arithmetic fp32, weights
// the fp32 master in torch layout [C, 1, K, K] (never rounded to bf16), optional fp32 bias [C].
//
//  * dwconv_fwd_kernel     y[n, oy, ox, c] = b[c] + sum_{ky, kx} x[n, oy + ky - K/2, ox + kx - K/2, c] * w[c, ky, kx],
//                          rounded to bf16 once.  With flip it reads w[c, K-1-ky, K-1-kx]: the data gradient
//                          dx = conv(dy, flipped w) is the same body, the flag only changes the weight stage.
//  * dwconv_wgrad_kernel   per workgroup one partial [K*K + 1][32] of
//                          dw[c, ky, kx] = sum_{n, oy, ox} dy[n, oy, ox, c] * x[n, oy + ky - K/2, ox + kx - K/2, c] and
//                          db[c] = sum dy
//  * dwconv_wgrad_reduce_kernel  sums the partials in a fixed order into dw (torch layout) and db.
//
// Why VALU and not MFMA (reasoned, not measured): a depthwise conv has no reduction over channels.  Per channel it is a
// banded-Toeplitz product; padded to a 16x16x32 MFMA about 22 % of the MACs would be useful, and the per-channel B
// operand would have to be gathered from channel-innermost data with 2-byte strided LDS reads.  The VALU form below
// does 28 FMAs per 8-byte LDS read at K = 7; measured timings are in profiles/r22/dwconv/README.md.
//
// Forward, per workgroup of 256 threads = one image, a slab of CB channels, a tile of R output rows x TW columns,
// with TW * CB / 4 == 256 and (TW, CB, R) one of (32, 32, 14), (16, 64, 14), (8, 128, 7) picked on the host by W and C
// so that the lanes stay busy on 14 x 14 and 7 x 7 maps, where the whole image is one tile:
//   1. stage the (R + K - 1) x (TW + K - 1) x CB input halo into LDS as bf16 with 16-byte loads; positions outside
//      the image or past C are written as zeros, so the padding lives in LDS and not in branches.  The slab's weights
//      go to LDS as fp32 [K * K][CB] (flipped for the data gradient).
//   2. a thread owns 4 adjacent channels and one output column; lanes run over channel quads first, then columns, so
//      a wave's 8-byte read of one halo position covers 512 contiguous bytes (conflict-free) and the 16-byte weight
//      reads are broadcasts.  kx is the outer loop: the thread loads the K * 4 weights of that kernel column, walks
//      down the R + K - 1 input rows of column ox + kx, reads each 4-channel input once and feeds the up to K output
//      rows it contributes to.  R * 4 fp32 accumulators stay live.
//   3. masked 8-byte stores (tails in C, H and W).
//
// Weight gradient, per workgroup = a slab of 32 channels and a run of consecutive (image, row tile, column tile)
// items of that slab (at least kMinItems, so the partial count stays small):
//   1. per item stage the same x halo plus the R x TW dy tile (zeros outside the image / past C).
//   2. a thread is (channel quad, kx, part) and keeps K * 4 accumulators, one 4-vector per ky.  Part p takes the
//      output columns p, p + PARTS, ...; for a column it walks down the R + K - 1 rows of x column ox + kx with the
//      last K dy vectors in registers: each x vector read from LDS feeds K * 4 FMAs.  The threads left over sum dy
//      for db.
//   3. after the last item the parts are summed through LDS in a fixed order and the workgroup writes its partial.
// No atomics anywhere: dw and db are bitwise reproducible run to run.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"

namespace ringdp {
namespace kern {

using namespace dev;

namespace {

constexpr int kThreads = 256;
constexpr int kWgCB = 32;      // channels of a weight-gradient slab
constexpr int kMinItems = 4;   // tiles a weight-gradient workgroup takes at least
constexpr int kRedLanes = 8;   // partial sums per output element in the reduce kernel

__device__ __forceinline__ f32x4 cvt4(const bf16* p) {  // 4 bf16 (8-byte aligned, LDS) -> fp32
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
               __uint_as_float(v.y & 0xffff0000u)};
}

struct DwTile {
  int N, H, W, C;
  int rtiles, wtiles, ctiles;
};

// The (HR x HC x CB) halo of the tile at (oy0, ox0) of image n, channels [c0, c0 + CB), zero outside the image and
// past C.  pad = K / 2 for x; the dy tile is the same call with pad = 0 and the tile's own extent.
template <int HR, int HC, int CB>
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ src, bf16* lds, const DwTile& a, int n, int gy0,
                                           int gx0, int c0, int tid) {
  constexpr int CH = CB / 8;
#pragma unroll 4
  for (int i = tid; i < HR * HC * CH; i += kThreads) {
    const int ch = i % CH, pos = i / CH, ic = pos % HC, ir = pos / HC;
    const int gy = gy0 + ir, gx = gx0 + ic, c = c0 + ch * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W && c < a.C)
      v = *reinterpret_cast<const uint4*>(src + (((int64_t)n * a.H + gy) * a.W + gx) * a.C + c);
    *reinterpret_cast<uint4*>(lds + pos * CB + ch * 8) = v;
  }
}

template <int K, int TW, int CB, int R>
__global__ __launch_bounds__(kThreads) void dwconv_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, bf16* __restrict__ y,
                                                              DwTile a, int flip) {
  constexpr int P = K / 2, HR = R + K - 1, HC = TW + K - 1, Q = CB / 4, KK = K * K;
  static_assert(TW * Q == kThreads, "a thread per (channel quad, output column)");
  __shared__ __attribute__((aligned(16))) bf16 halo[HR * HC * CB];
  __shared__ __attribute__((aligned(16))) float wl[KK * CB];

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int wt = b % a.wtiles;
  b /= a.wtiles;
  const int rt = b % a.rtiles;
  b /= a.rtiles;
  const int ct = b % a.ctiles, n = b / a.ctiles;
  const int oy0 = rt * R, ox0 = wt * TW, c0 = ct * CB;

  stage_tile<HR, HC, CB>(x, halo, a, n, oy0 - P, ox0 - P, c0, tid);
  for (int i = tid; i < KK * CB; i += kThreads) {
    const int cl = i % CB, t = i / CB;
    wl[i] = c0 + cl < a.C ? w[(int64_t)(c0 + cl) * KK + (flip ? KK - 1 - t : t)] : 0.f;
  }
  __syncthreads();

  const int q = tid % Q, col = tid / Q, c = c0 + q * 4, ox = ox0 + col;
  const bool live = c < a.C && ox < a.W;
  f32x4 acc[R];
  const f32x4 bv = (bias != nullptr && live) ? *reinterpret_cast<const f32x4*>(bias + c) : zero_f32x4();
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = bv;
  const bf16* hp = halo + col * CB + q * 4;
  const float* wp = wl + q * 4;
#pragma unroll 1
  for (int kx = 0; kx < K; ++kx) {
    f32x4 wv[K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) wv[ky] = *reinterpret_cast<const f32x4*>(wp + (ky * K + kx) * CB);
#pragma unroll
    for (int ir = 0; ir < HR; ++ir) {
      const f32x4 xv = cvt4(hp + (ir * HC + kx) * CB);
#pragma unroll
      for (int ky = 0; ky < K; ++ky)
        if (ir - ky >= 0 && ir - ky < R) acc[ir - ky] += xv * wv[ky];
    }
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oy = oy0 + r;
    if (oy < a.H) {
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)acc[r][j];
      *reinterpret_cast<bf16x4*>(y + (((int64_t)n * a.H + oy) * a.W + ox) * a.C + c) = o;
    }
  }
}

template <int K, int TW, int R>
struct WgradCfg {
  static constexpr int CB = kWgCB, Q = CB / 4, KK = K * K, HR = R + K - 1, HC = TW + K - 1;
  static constexpr int PARTS = kThreads / (Q * K) < TW ? kThreads / (Q * K) : TW;
  static constexpr int NCONV = Q * K * PARTS;       // threads that accumulate dw
  static constexpr int NSP = (kThreads - NCONV) / Q;  // threads per channel quad that accumulate db
  static constexpr int kStage = (HR * HC + R * TW) * CB * 2;   // bytes: x halo + dy tile
  static constexpr int kRed = (PARTS * KK + NSP) * CB * 4;     // bytes: the parts' sums, aliased onto the stage
  static constexpr int kLds = kStage > kRed ? kStage : kRed;
  static_assert(NSP >= 1, "no thread left for the bias gradient");
};

template <int K, int TW, int R>
__global__ __launch_bounds__(kThreads) void dwconv_wgrad_kernel(const bf16* __restrict__ x,
                                                                const bf16* __restrict__ dy,
                                                                float* __restrict__ partial, DwTile a, int items,
                                                                int per_wg, int groups) {
  using Cfg = WgradCfg<K, TW, R>;
  constexpr int P = K / 2, HR = Cfg::HR, HC = Cfg::HC, CB = Cfg::CB, Q = Cfg::Q, KK = Cfg::KK;
  constexpr int PARTS = Cfg::PARTS, NCONV = Cfg::NCONV, NSP = Cfg::NSP;
  __shared__ __attribute__((aligned(16))) uint8_t smem[Cfg::kLds];
  bf16* halo = reinterpret_cast<bf16*>(smem);
  bf16* dyt = halo + HR * HC * CB;

  const int tid = threadIdx.x;
  const int ct = blockIdx.x / groups, g = blockIdx.x - ct * groups, c0 = ct * CB;
  const int it0 = g * per_wg, it1 = min(items, it0 + per_wg);
  const int q = tid % Q, kx = (tid / Q) % K, part = tid / (Q * K);
  const int sq = (tid - NCONV) % Q, sub = (tid - NCONV) / Q;  // the bias-gradient role of tid >= NCONV

  f32x4 acc[K];
#pragma unroll
  for (int ky = 0; ky < K; ++ky) acc[ky] = zero_f32x4();
  f32x4 dbacc = zero_f32x4();

  for (int item = it0; item < it1; ++item) {
    int t = item;
    const int wt = t % a.wtiles;
    t /= a.wtiles;
    const int rt = t % a.rtiles, n = t / a.rtiles;
    const int oy0 = rt * R, ox0 = wt * TW;
    if (item != it0) __syncthreads();  // the previous item's reads are done
    stage_tile<HR, HC, CB>(x, halo, a, n, oy0 - P, ox0 - P, c0, tid);
    stage_tile<R, TW, CB>(dy, dyt, a, n, oy0, ox0, c0, tid);
    __syncthreads();
    if (tid < NCONV) {
#pragma unroll 1
      for (int oc = part; oc < TW; oc += PARTS) {
        const bf16* xp = halo + (oc + kx) * CB + q * 4;
        const bf16* dp = dyt + oc * CB + q * 4;
        f32x4 dv[R];
#pragma unroll
        for (int ir = 0; ir < HR; ++ir) {
          if (ir < R) dv[ir] = cvt4(dp + ir * TW * CB);
          const f32x4 xv = cvt4(xp + ir * HC * CB);
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
            if (ir - ky >= 0 && ir - ky < R) acc[ky] += dv[ir - ky] * xv;
        }
      }
    } else if (sub < NSP) {
#pragma unroll 4
      for (int pos = sub; pos < R * TW; pos += NSP) dbacc += cvt4(dyt + pos * CB + sq * 4);
    }
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [PARTS][KK][CB], then [NSP][CB]
  if (tid < NCONV) {
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
      *reinterpret_cast<f32x4*>(red + (part * KK + ky * K + kx) * CB + q * 4) = acc[ky];
  } else if (sub < NSP) {
    *reinterpret_cast<f32x4*>(red + (PARTS * KK + sub) * CB + sq * 4) = dbacc;
  }
  __syncthreads();
  float* out = partial + (int64_t)blockIdx.x * (KK + 1) * CB;
  for (int i = tid; i < (KK + 1) * CB; i += kThreads) {
    const int cl = i % CB, t = i / CB;
    float s = 0.f;
    if (t < KK) {
#pragma unroll
      for (int p = 0; p < PARTS; ++p) s += red[(p * KK + t) * CB + cl];
    } else {
#pragma unroll
      for (int p = 0; p < NSP; ++p) s += red[(PARTS * KK + p) * CB + cl];
    }
    out[i] = s;
  }
}

// One workgroup per (slab, tap): thread (cl, j) sums the partials g = j, j + 8, ... in order, then lane group 0 adds the
// 8 sums in order.  tap == KK is the bias gradient.
__global__ __launch_bounds__(kThreads) void dwconv_wgrad_reduce_kernel(const float* __restrict__ partial,
                                                                       float* __restrict__ dw, float* __restrict__ db,
                                                                       int C, int KK, int groups) {
  __shared__ float sm[kRedLanes][kWgCB];
  const int tid = threadIdx.x, cl = tid % kWgCB, j = tid / kWgCB;
  const int ct = blockIdx.x / (KK + 1), t = blockIdx.x - ct * (KK + 1);
  const float* p = partial + ((int64_t)ct * groups * (KK + 1) + t) * kWgCB + cl;
  float s = 0.f;
  for (int g = j; g < groups; g += kRedLanes) s += p[(int64_t)g * (KK + 1) * kWgCB];
  sm[j][cl] = s;
  __syncthreads();
  const int c = ct * kWgCB + cl;
  if (j != 0 || c >= C) return;
#pragma unroll
  for (int k = 1; k < kRedLanes; ++k) s += sm[k][cl];
  if (t < KK)
    dw[(int64_t)c * KK + t] = s;
  else if (db != nullptr)
    db[c] = s;
}

DwTile make_tile(int N, int H, int W, int C, int R, int TW, int CB) {
  DwTile a{};
  a.N = N;
  a.H = H;
  a.W = W;
  a.C = C;
  a.rtiles = (H + R - 1) / R;
  a.wtiles = (W + TW - 1) / TW;
  a.ctiles = (C + CB - 1) / CB;
  return a;
}

template <int K, int TW, int CB, int R>
void launch_fwd(const bf16* x, const float* w, const float* bias, bf16* y, int N, int H, int W, int C, bool flip,
                hipStream_t s) {
  const DwTile a = make_tile(N, H, W, C, R, TW, CB);
  const unsigned grid = (unsigned)((int64_t)N * a.ctiles * a.rtiles * a.wtiles);
  dwconv_fwd_kernel<K, TW, CB, R><<<grid, kThreads, 0, s>>>(x, w, bias, y, a, flip ? 1 : 0);
}

template <int K>
void fwd_k(const bf16* x, const float* w, const float* bias, bf16* y, int N, int H, int W, int C, bool flip,
           hipStream_t s) {
  if (W > 16 || C <= 32)
    launch_fwd<K, 32, 32, 14>(x, w, bias, y, N, H, W, C, flip, s);
  else if (W > 8 || C <= 64)
    launch_fwd<K, 16, 64, 14>(x, w, bias, y, N, H, W, C, flip, s);
  else
    launch_fwd<K, 8, 128, 7>(x, w, bias, y, N, H, W, C, flip, s);
}

int wgrad_tw(int W) { return W > 16 ? 32 : (W > 8 ? 16 : 8); }
int wgrad_r(int W) { return W > 8 ? 14 : 7; }

// (items of a slab, items per workgroup, workgroups per slab)
void wgrad_split(const DwTile& a, int num_cus, int& items, int& per_wg, int& groups) {
  items = a.N * a.rtiles * a.wtiles;
  const int want = (2 * num_cus + a.ctiles - 1) / a.ctiles;  // two resident workgroups per CU over all slabs
  per_wg = (items + want - 1) / want;
  per_wg = per_wg < kMinItems ? kMinItems : per_wg;
  groups = (items + per_wg - 1) / per_wg;
}

template <int K, int TW, int R>
void launch_wgrad(const bf16* x, const bf16* dy, float* partial, int N, int H, int W, int C, int num_cus,
                  hipStream_t s) {
  const DwTile a = make_tile(N, H, W, C, R, TW, kWgCB);
  int items, per_wg, groups;
  wgrad_split(a, num_cus, items, per_wg, groups);
  dwconv_wgrad_kernel<K, TW, R><<<(unsigned)(a.ctiles * groups), kThreads, 0, s>>>(x, dy, partial, a, items, per_wg,
                                                                                 groups);
}

template <int K>
void wgrad_k(const bf16* x, const bf16* dy, float* partial, int N, int H, int W, int C, int num_cus, hipStream_t s) {
  if (W > 16)
    launch_wgrad<K, 32, 14>(x, dy, partial, N, H, W, C, num_cus, s);
  else if (W > 8)
    launch_wgrad<K, 16, 14>(x, dy, partial, N, H, W, C, num_cus, s);
  else
    launch_wgrad<K, 8, 7>(x, dy, partial, N, H, W, C, num_cus, s);
}

}  // namespace

bool dwconv_ok(int K) { return K == 3 || K == 5 || K == 7; }

void dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C, int K, bool flip,
                hipStream_t s) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return;
  const bf16* xb = static_cast<const bf16*>(x);
  bf16* yb = static_cast<bf16*>(y);
  if (K == 3)
    fwd_k<3>(xb, w, bias, yb, N, H, W, C, flip, s);
  else if (K == 5)
    fwd_k<5>(xb, w, bias, yb, N, H, W, C, flip, s);
  else
    fwd_k<7>(xb, w, bias, yb, N, H, W, C, flip, s);
}

int64_t dwconv_wgrad_partial_floats(int N, int H, int W, int C, int K, int num_cus) {
  const DwTile a = make_tile(N, H, W, C, wgrad_r(W), wgrad_tw(W), kWgCB);
  int items, per_wg, groups;
  wgrad_split(a, num_cus, items, per_wg, groups);
  return (int64_t)a.ctiles * groups * (K * K + 1) * kWgCB;
}

void dwconv_wgrad(const void* x, const void* dy, float* partial, float* dw, float* db, int N, int H, int W, int C,
                  int K, int num_cus, hipStream_t s) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return;
  const bf16* xb = static_cast<const bf16*>(x);
  const bf16* dyb = static_cast<const bf16*>(dy);
  if (K == 3)
    wgrad_k<3>(xb, dyb, partial, N, H, W, C, num_cus, s);
  else if (K == 5)
    wgrad_k<5>(xb, dyb, partial, N, H, W, C, num_cus, s);
  else
    wgrad_k<7>(xb, dyb, partial, N, H, W, C, num_cus, s);
  const DwTile a = make_tile(N, H, W, C, wgrad_r(W), wgrad_tw(W), kWgCB);
  int items, per_wg, groups;
  wgrad_split(a, num_cus, items, per_wg, groups);
  dwconv_wgrad_reduce_kernel<<<(unsigned)(a.ctiles * (K * K + 1)), kThreads, 0, s>>>(partial, dw, db, C, K * K, groups);
}

}  // namespace kern
}  // namespace ringdp
