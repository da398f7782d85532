// fp32 NCHW convolution / linear / max-pool kernels: the MNIST ConvNet at the reference's
// precision (ref/launch_dist.py:50-59 trains in fp32).
// This header: the implicit-GEMM core with its loaders, epilogues and launch templates, instantiated by
// conv_f32_fwd.hip, conv_f32_dgrad.hip and conv_f32_wgrad.hip; conv_f32_pool.hip holds the pool kernels.
//
// Every conv product (forward, data gradient, weight gradient; fc1 is a 1x1 conv over a 1x1
// image) is one implicit GEMM on the exact-f32 matrix cores (v_mfma_f32_16x16x4_f32, f32 in /
// f32 accumulate - the same arithmetic as an fmaf chain, so results track ATen fp32 to
// reduction-order rounding).  Operands are gathered straight from the NCHW tensors (im2col never
// materialised) into double-buffered LDS k-tiles of 16; 4 waves each own a 32x32 block of the
// output (2x2 MFMA tiles), the workgroup tile is 64x64, 128x32 or 32x128 by the GEMM's shape.
//
// The f32 MFMA issues one 16x16x4 product per 32 cycles, so the operand gathers have to cost
// well under that per element.  The round-2 kernel spent ~10x the MFMA time in 64-bit divides in
// the loaders; here every index is 32-bit and the divides are gone from the k-loop:
//   * the thread-fixed index of an operand (its GEMM row for m-contiguous operands, its column
//     for k-contiguous ones) is decomposed once per tile;
//   * for m-contiguous operands the k decomposition (channel, ky, kx) -> (offset, dy, dx) is a
//     per-workgroup LDS table built at kernel start;
//   * for k-contiguous operands (the weight gradients, k = batch x pixel) every lane of a row of
//     the tile shares one k per k-tile, decomposed with multiply-high divisions (FastDiv).
// MFMAs take the B fragment as their row operand, so a lane's results run along m - the NCHW
// pixel index - and each store instruction writes 64-B runs of the output plane.
// Tensors whose element count reaches 2^31 are processed in batch chunks by the host launchers.
// Weight gradients reduce over B*OH*OW, so they run split-K into per-slice slabs that a
// fixed-order reduction sums (deterministic).  Max-pool forward fuses the ReLU and stores a 1-byte
// argmax code; its backward is a gather (each input position sums the windows whose code points
// at it), so the overlapping 2x2/s1 pool needs no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "conv_f32_host.h"
#include "device_common.h"

namespace ringdp::kern {
namespace {

using dev::f32x4;

constexpr int BK = 16, TPB = 256;

// n / d for 0 <= n < 2^31 without a divide: q = (mulhi(n, mul) + n) >> shift.
struct FastDiv {
  uint32_t d, mul, shift;
};
FastDiv make_fdiv(uint32_t d) {
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  const uint64_t m = ((1ull << 32) * ((1ull << s) - d)) / d + 1;
  return FastDiv{d, static_cast<uint32_t>(m), s};
}
__device__ __forceinline__ int fdiv(int n, const FastDiv& f) {
  return static_cast<int>((__umulhi(static_cast<uint32_t>(n), f.mul) + static_cast<uint32_t>(n)) >> f.shift);
}

// (dy, dx) packed as two int16 halves; "never in bounds" marker for padding rows / columns
__device__ __forceinline__ int pack_dyx(int dy, int dx) { return (dy & 0xffff) | (dx << 16); }
__device__ __forceinline__ int unpack_dy(int v) { return static_cast<int>(static_cast<short>(v & 0xffff)); }
__device__ __forceinline__ int unpack_dx(int v) { return v >> 16; }
constexpr int kOut = -0x2000;  // added to a coordinate <= 1024 it can never land in [0, H)

// ---------------------------------------------------------------- operand loaders
// GEMM C[M][N] = sum_k A(m, k) * B(k, n).  kMC: the operand's thread-fixed index is contiguous in
// memory (lanes walk m), with a per-workgroup k table; otherwise lanes walk k.
// A loader resolves an element to a Ref: an element offset into its source and a valid flag.  The
// kernel reads every element with a raw buffer load (SGPR resource + 32-bit VGPR offset): invalid
// elements (zero padding, past an edge) get an offset beyond the resource's range and the hardware
// returns 0, so the loads are branch-free, their count is static and they need no 64-bit address
// arithmetic.  u8 pixels are normalised at the stash, where their padding (0 AFTER normalisation)
// needs the valid flag.
constexpr int kBadOff = 0x20000000;  // x 4 bytes = 2^31: past every source (chunks stay < 2^31 bytes)
struct Ref {
  int off, ok;
};
__device__ __forceinline__ Ref ref_if(bool ok, int off) { return Ref{ok ? off : kBadOff, ok ? 1 : 0}; }
__device__ __forceinline__ bool in2(int y, int x, int H, int W) {
  return static_cast<unsigned>(y) < static_cast<unsigned>(H) && static_cast<unsigned>(x) < static_cast<unsigned>(W);
}

template <bool U8>
struct Src {  // fp32 tensor, or raw uint8 pixels normalised as (v / 255 - mean) * inv_std
  typedef typename std::conditional<U8, unsigned char, float>::type T;
  static constexpr bool kU8 = U8;
  const T* p;
  int bytes;  // buffer-resource range
  float mean, inv_std;
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc() const {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), 0, bytes, 0x00020000);
  }
  __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, int off) const {
    if constexpr (U8) return __builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0);
    else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off * 4, 0, 0));
  }
  __device__ __forceinline__ float cvt(T v) const {
    if constexpr (U8) return (static_cast<float>(v) * (1.0f / 255.0f) - mean) * inv_std;
    else return v;
  }
};

// PAD = false (a valid conv over an fp32 input): every (m, k) is in bounds, so rows past M and
// k past K are clamped onto real elements instead of checked - the rows are never stored and the
// weights past K are zero.
// WIN: window-major output pixels, m = (b, py, px, wy, wx) with (oy, ox) = (2 py + wy, 2 px + wx), so
// the 4 pixels of a 2x2/s2 pooling window are 4 consecutive m (the PoolOut epilogue); `ow` then
// divides by the pooled width.
// MODE 2: one image per 128-row m tile, m = (b, p < 128), p >= OH*OW clamped onto the last pixel
// (those rows are never stored) - the PoolS1Out epilogue pools a whole image from LDS.
template <bool U8, bool PAD, int MODE = 0>
struct FwdA {  // A(m = (b, oy, ox), k = (c, ky, kx)) = x[b, c, oy + ky - pad, ox + kx - pad]
  static constexpr bool kMC = true;
  Src<U8> src;
  int C, H, W, R, pad, OW, K, M;
  FastDiv ohw, ow;
  struct O {
    int base, y, x;
  };
  __device__ O outer(int m) const {
    if constexpr (!PAD) m = min(m, M - 1);
    else if (m >= M) return O{0, kOut, kOut};
    int b, r;
    if constexpr (MODE == 2) {
      b = m >> 7;
      r = min(m & 127, static_cast<int>(ohw.d) - 1);
    } else {
      b = fdiv(m, ohw);
      r = m - b * static_cast<int>(ohw.d);
    }
    int oy, ox;
    if constexpr (MODE == 1) {
      const int w = r >> 2, py = fdiv(w, ow);
      oy = 2 * py + ((r >> 1) & 1);
      ox = 2 * (w - py * static_cast<int>(ow.d)) + (r & 1);
    } else {
      oy = fdiv(r, ow);
      ox = r - oy * OW;
    }
    return O{b * C * H * W + (oy - pad) * W + (ox - pad), oy - pad, ox - pad};
  }
  __device__ int2 ktab(int k) const {  // (offset, dy|dx)
    if constexpr (!PAD) k = min(k, K - 1);
    else if (k >= K) return int2{0, pack_dyx(kOut, kOut)};
    const int rr = R * R, c = k / rr, t = k - c * rr, ky = t / R, kx = t - ky * R;
    return int2{c * H * W + ky * W + kx, pack_dyx(ky, kx)};
  }
  __device__ Ref ref(const O& o, int2 kt) const {  // zero padding after Normalize
    if constexpr (!PAD) return Ref{o.base + kt.x, 1};
    else return ref_if(in2(o.y + unpack_dy(kt.y), o.x + unpack_dx(kt.y), H, W), o.base + kt.x);
  }
};

struct DgradA {  // A(m = (b, iy, ix), k = (n, ky, kx)) = dz[b, n, iy + pad - ky, ix + pad - kx]
  static constexpr bool kMC = true;
  Src<false> src;
  int Kout, W, R, OH, OW, pad, K, M;
  FastDiv hw, w;
  struct O {
    int base, y, x;
  };
  __device__ O outer(int m) const {
    if (m >= M) return O{0, kOut, kOut};
    const int b = fdiv(m, hw), r = m - b * static_cast<int>(hw.d);
    const int iy = fdiv(r, w), ix = r - iy * W;
    return O{b * Kout * OH * OW + (iy + pad) * OW + (ix + pad), iy + pad, ix + pad};
  }
  __device__ int2 ktab(int k) const {
    if (k >= K) return int2{0, pack_dyx(kOut, kOut)};
    const int rr = R * R, n = k / rr, t = k - n * rr, ky = t / R, kx = t - ky * R;
    return int2{n * OH * OW - ky * OW - kx, pack_dyx(-ky, -kx)};
  }
  __device__ Ref ref(const O& o, int2 kt) const {
    return ref_if(in2(o.y + unpack_dy(kt.y), o.x + unpack_dx(kt.y), OH, OW), o.base + kt.x);
  }
};

struct WeightB {  // B(k = (c, ky, kx), n) = w[n][c][ky][kx]; lanes walk k
  static constexpr bool kMC = false;
  Src<false> src;
  int K, N;
  typedef int O;
  typedef int KS;
  __device__ O outer(int n) const { return n < N ? n * K : -1; }
  __device__ KS kstate(int k, int kend) const { return k < kend ? k : -1; }
  __device__ Ref ref(O o, KS k) const { return ref_if((o | k) >= 0, o + k); }
};

struct DgradB {  // B(k = (n, ky, kx), c) = w[n][c][ky][kx]; lanes walk k
  static constexpr bool kMC = false;
  Src<false> src;
  int C, rr, K;
  FastDiv frr;
  typedef int O;
  typedef int KS;
  __device__ O outer(int c) const { return c < C ? c * rr : -1; }
  __device__ KS kstate(int k, int kend) const {
    if (k >= kend) return -1;
    const int n = fdiv(k, frr);
    return n * C * rr + (k - n * rr);
  }
  __device__ Ref ref(O o, KS k) const { return ref_if((o | k) >= 0, o + k); }
};

struct WgradA {  // A(m = n, k = (b, r)) = dz[b, n, r]     (k runs over batch x output pixels)
  static constexpr bool kMC = false;
  Src<false> src;
  int Kout, ohwi;
  FastDiv ohw;
  typedef int O;
  typedef int KS;
  __device__ O outer(int n) const { return n < Kout ? n * ohwi : -1; }
  __device__ KS kstate(int k, int kend) const {
    if (k >= kend) return -1;
    const int b = fdiv(k, ohw);
    return b * Kout * ohwi + (k - b * ohwi);
  }
  __device__ Ref ref(O o, KS k) const { return ref_if((o | k) >= 0, o + k); }
};

// PAD = false: as FwdA - columns past Nw and k past the slice are clamped onto real elements (the
// columns are never stored, A is zero past the slice).
template <bool U8, bool PAD>
struct WgradB {  // B(k = (b, oy, ox), j = (c, ky, kx)) = x[b, c, oy + ky - pad, ox + kx - pad]
  static constexpr bool kMC = false;
  Src<U8> src;
  int C, H, W, R, pad, OW, Nw;
  FastDiv ohw, ow;
  struct O {
    int off, dyx;  // dyx never in bounds past the last column
  };
  struct KS {
    int base, y, x;  // y = oy - pad, x = ox - pad; y = kOut when k is past the slice
  };
  __device__ O outer(int j) const {
    if constexpr (!PAD) j = min(j, Nw - 1);
    else if (j >= Nw) return O{0, pack_dyx(kOut, kOut)};
    const int rr = R * R, c = j / rr, t = j - c * rr, ky = t / R, kx = t - ky * R;
    return O{c * H * W + ky * W + kx, pack_dyx(ky, kx)};
  }
  __device__ KS kstate(int k, int kend) const {
    if constexpr (!PAD) k = min(k, kend - 1);
    else if (k >= kend) return KS{0, kOut, kOut};
    const int b = fdiv(k, ohw), r = k - b * static_cast<int>(ohw.d);
    const int oy = fdiv(r, ow), ox = r - oy * OW;
    return KS{b * C * H * W + (oy - pad) * W + (ox - pad), oy - pad, ox - pad};
  }
  __device__ Ref ref(const O& o, const KS& k) const {
    if constexpr (!PAD) return Ref{k.base + o.off, 1};
    return ref_if(in2(k.y + unpack_dy(o.dyx), k.x + unpack_dx(o.dyx), H, W), k.base + o.off);
  }
};

// ---------------------------------------------------------------- epilogues
struct NCHWOut {  // C[m = (b, p)][n] (+ bias[n]) -> out[b, n, p]
  static constexpr bool kPool = false, kPoolS1 = false;
  float* out;
  const float* bias;
  int N, M;
  FastDiv hw;
  __device__ int row(int m) const {  // offset of out[b, 0, p]
    const int b = fdiv(m, hw);
    return b * N * static_cast<int>(hw.d) + (m - b * static_cast<int>(hw.d));
  }
  __device__ void store(int rowoff, int n, float v) const {
    out[rowoff + n * static_cast<int>(hw.d)] = v + (bias ? bias[n] : 0.f);
  }
};

// split-K data gradient (small batches): slice z stores its partial dx, NCHW, into slab plane z
struct NCHWSlabOut {
  static constexpr bool kPool = false, kPoolS1 = false;
  float* out;
  int N, M, plane;  // plane = M * N elements
  FastDiv hw;
  __device__ int row(int m) const {
    const int b = fdiv(m, hw);
    return static_cast<int>(blockIdx.z) * plane + b * N * static_cast<int>(hw.d) + (m - b * static_cast<int>(hw.d));
  }
  __device__ void store(int rowoff, int n, float v) const { out[rowoff + n * static_cast<int>(hw.d)] = v; }
};

struct SlabOut {  // split-K slice z: slab[z][m][n]
  static constexpr bool kPool = false, kPoolS1 = false;
  float* slab;
  int N, M;
  __device__ int row(int m) const { return static_cast<int>(blockIdx.z) * M * N + m * N; }
  __device__ void store(int rowoff, int n, float v) const { slab[rowoff + n] = v; }
};

// Fused ReLU + 2x2/s2 max-pool over window-major m (FwdA<.., WIN>): the 4 pixels of a window are
// the 4 lanes 4q..4q+3 of a 16-lane MFMA row group, reduced with two lane exchanges.
// a[b, n, w] = relu(max_t (C[m][n] + bias[n])), code[b, n, w] = first argmax t (255: not live); the
// pre-activation is never written.
struct PoolOut {
  static constexpr bool kPool = true, kPoolS1 = false;
  float* a;
  unsigned char* code;
  const float* bias;
  int N, M, phw;  // phw = pooled pixels per plane
  FastDiv hw;     // conv output pixels per plane
  __device__ int row(int m) const {  // offset of a[b, 0, w]
    const int b = fdiv(m, hw);
    return b * N * phw + ((m - b * static_cast<int>(hw.d)) >> 2);
  }
};

// Fused ReLU + 2x2/s1 (overlapping) max-pool over one image per 128-row tile (FwdA<.., 2>): the tile's
// C + bias goes to LDS and the workgroup pools the whole image from there.
struct PoolS1Out {
  static constexpr bool kPool = false, kPoolS1 = true;
  float* a;
  unsigned char* code;
  const float* bias;
  int N, OW, PW, phw;  // conv output width, pooled width, pooled pixels per plane
  FastDiv fphw, fpw;
};

template <int CTL>
__device__ __forceinline__ void pool_quad_step(float& best, int& bt) {
  const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, best), CTL, 0xF,
                                                                         0xF, false));
  const int ot = __builtin_amdgcn_update_dpp(0, bt, CTL, 0xF, 0xF, false);
  if (ov > best || (ov == best && ot < bt)) {
    best = ov;
    bt = ot;
  }
}

// ---------------------------------------------------------------- the GEMM core
// grid: x = m tiles, y = n tiles, z = k slices (each covers k_per_slice of K).  WM x WN waves, each
// owning a (16 TM) x (16 TN) block of the output (TM x TN MFMA tiles).  On gfx950 the f32 MFMA runs
// at the f32 VALU rate and the loaders' VALU work competes with it (PMC: MFMA busy 48 % with 5.7
// VALU instructions per MFMA on 32x32 wave blocks), so the wave blocks are as large as the GEMM's
// narrow side allows: elements gathered per MFMA per lane = 16 / BN (A) + 16 / BM (B).
// With WM * WN < 4 the remaining waves split each k-tile's MFMA steps between them and the partial
// accumulators are summed in a fixed wave order at the end (the 32x32 tile of conv1's weight
// gradient).  ktab_n > 0: the A operand's k table (K rounded up to BK) in dynamic LDS.
template <int WM, int WN, int TM, int TN, class LA, class LB, class Epi>
__global__ __launch_bounds__(TPB) void gemm_f32_kernel(int M, int N, int K, int k_per_slice, int ktab_n, int bias_col,
                                                       LA la, LB lb, Epi epi) {
  constexpr int BM = 16 * TM * WM, BN = 16 * TN * WN, KSPLIT = 4 / (WM * WN);
  static_assert(KSPLIT * WM * WN == 4 && BK / 4 >= KSPLIT, "4 waves");
  constexpr int LDA = BM + 16, LDB = BN + 16;  // row stride = 16 banks mod 64: conflict-free MFMA reads
  constexpr int EA = BM * BK / TPB, EB = BN * BK / TPB;
  constexpr int LDT = BM + 4;  // PoolS1Out staging row stride
  constexpr int SM_AB = 2 * BK * (LDA + LDB), SM = (Epi::kPoolS1 && BN * LDT > SM_AB) ? BN * LDT : SM_AB;
  __shared__ float smem[SM];
  auto As = reinterpret_cast<float(*)[BK][LDA]>(smem);
  auto Bs = reinterpret_cast<float(*)[BK][LDB]>(smem + 2 * BK * LDA);
  extern __shared__ int2 ktab[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wk = wave / (WM * WN), wmn = wave % (WM * WN);
  const int wm = (wmn / WN) * 16 * TM, wn = (wmn % WN) * 16 * TN;
  const int m0 = static_cast<int>(blockIdx.x) * BM;
  const int n0 = static_cast<int>(blockIdx.y) * BN;
  const int kbeg = static_cast<int>(blockIdx.z) * k_per_slice;
  const int kend = min(kbeg + k_per_slice, K);

  if constexpr (LA::kMC) {
    for (int k = tid; k < ktab_n; k += TPB) ktab[k] = la.ktab(k);
  }

  // thread-fixed operand state.  kMC: index o = tid % BO, k rows tid / BO + (TPB / BO) * i.
  // otherwise: k = tid % BK (one per k-tile), index rows tid / BK + (TPB / BK) * i.
  typename LA::O oa[LA::kMC ? 1 : EA];
  typename LB::O ob[LB::kMC ? 1 : EB];
  if constexpr (LA::kMC) oa[0] = la.outer(m0 + tid % BM);
  else
#pragma unroll
    for (int i = 0; i < EA; ++i) oa[i] = la.outer(m0 + tid / BK + (TPB / BK) * i);
  if constexpr (LB::kMC) ob[0] = lb.outer(n0 + tid % BN);
  else
#pragma unroll
    for (int i = 0; i < EB; ++i) ob[i] = lb.outer(n0 + tid / BK + (TPB / BK) * i);
  if constexpr (LA::kMC) __syncthreads();  // k table visible

  // the next k-tile's raw elements (loaded branch-free while the current tile is multiplied); u8
  // sources also keep a valid bit per element, applied when the tile is stashed
  const auto rsa = la.src.rsrc();
  const auto rsb = lb.src.rsrc();
  constexpr bool UA = decltype(la.src)::kU8, UB = decltype(lb.src)::kU8;
  typename decltype(la.src)::T ra[EA];
  typename decltype(lb.src)::T rb[EB];
  uint32_t va = 0, vb = 0;
  static_assert(EA <= 32 && EB <= 32, "valid bits");
  auto fetch = [&](int k0) {
    va = 0;
    vb = 0;
#pragma unroll
    for (int i = 0; i < EA; ++i) {
      Ref r;
      if constexpr (LA::kMC) r = la.ref(oa[0], ktab[k0 + tid / BM + (TPB / BM) * i]);
      else r = la.ref(oa[i], la.kstate(k0 + tid % BK, kend));
      ra[i] = la.src.load(rsa, r.off);
      if constexpr (UA) va |= static_cast<uint32_t>(r.ok) << i;
    }
#pragma unroll
    for (int i = 0; i < EB; ++i) {
      Ref r;
      if constexpr (LB::kMC) r = lb.ref(ob[0], ktab[k0 + tid / BN + (TPB / BN) * i]);
      else r = lb.ref(ob[i], lb.kstate(k0 + tid % BK, kend));
      rb[i] = lb.src.load(rsb, r.off);
      if constexpr (UB) vb |= static_cast<uint32_t>(r.ok) << i;
    }
  };
  // bias gradient (weight-gradient GEMMs, bias_col >= 0): row sums of A, accumulated by the n-tile 0
  // workgroups as they stash A (a k-contiguous dz tile) and reduced over the 16 k lanes at the end
  const bool bias_rows = !LA::kMC && bias_col >= 0 && blockIdx.y == 0;
  float bsum[LA::kMC ? 1 : EA];
#pragma unroll
  for (int i = 0; i < (LA::kMC ? 1 : EA); ++i) bsum[i] = 0.f;
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < EA; ++i) {
      float v;
      if constexpr (UA) v = ((va >> i) & 1) ? la.src.cvt(ra[i]) : 0.f;
      else v = ra[i];
      if constexpr (!LA::kMC) {
        if (bias_rows) bsum[i] += v;
      }
      if constexpr (LA::kMC) As[buf][tid / BM + (TPB / BM) * i][tid % BM] = v;
      else As[buf][tid % BK][tid / BK + (TPB / BK) * i] = v;
    }
#pragma unroll
    for (int i = 0; i < EB; ++i) {
      float v;
      if constexpr (UB) v = ((vb >> i) & 1) ? lb.src.cvt(rb[i]) : 0.f;
      else v = rb[i];
      if constexpr (LB::kMC) Bs[buf][tid / BN + (TPB / BN) * i][tid % BN] = v;
      else Bs[buf][tid % BK][tid / BK + (TPB / BK) * i] = v;
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = dev::zero_f32x4();

  const int lr = lane & 15, lk = lane >> 4;
  // this wave's k steps of a tile: all of them, or with KSPLIT waves per block every KSPLIT-th one
  // (wave-uniform start)
  constexpr int NKK = BK / 4 / KSPLIT;
  const int kk0 = 4 * __builtin_amdgcn_readfirstlane(wk);
  auto mfma_tile = [&](int buf) {
#pragma unroll
    for (int t = 0; t < NKK; ++t) {
      const int kk = (KSPLIT == 1 ? 4 * t : kk0 + 4 * KSPLIT * t) + lk;
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[buf][kk][wm + 16 * i + lr];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[buf][kk][wn + 16 * j + lr];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)  // B as the row operand: D[n][m], lane l holds n = 4 (l >> 4) + r, m = l & 15
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[i][j], 0, 0, 0);
    }
  };
  if (kbeg < kend) {
    fetch(kbeg);
    stash(0);
  }
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) fetch(k0 + BK);  // next tile in flight during the MFMAs
    mfma_tile(buf);
    if (more) stash(buf ^ 1);  // the other buffer's last readers passed the previous barrier
    __syncthreads();
    buf ^= 1;
  }
  if constexpr (!LA::kMC) {
    if (bias_rows) {
      static_assert(BK == 16, "bias rows: one 16-lane group per A row");
#pragma unroll
      for (int i = 0; i < EA; ++i) {
        float v = bsum[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        const int m = m0 + tid / BK + (TPB / BK) * i;
        if ((tid % BK) == 0 && m < M) epi.store(epi.row(m), bias_col, v);
      }
    }
  }
  if constexpr (KSPLIT > 1) {
    __shared__ f32x4 red[KSPLIT > 1 ? (KSPLIT - 1) * TM * TN * 64 : 1];
    if (wk > 0)
#pragma unroll
      for (int q = 0; q < TM * TN; ++q) red[((wk - 1) * TM * TN + q) * 64 + lane] = acc[q / TN][q % TN];
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int w = 0; w < KSPLIT - 1; ++w)
#pragma unroll
      for (int q = 0; q < TM * TN; ++q) acc[q / TN][q % TN] += red[(w * TM * TN + q) * 64 + lane];
  }
  if constexpr (Epi::kPoolS1) {
    static_assert(BM == 128, "one image per 128-row tile");
    float* T = smem;  // [BN][LDT]; the k-loop ended with a barrier, As / Bs are dead
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nl = wn + j * 16 + 4 * lk + r, n = n0 + nl;
          T[nl * LDT + wm + i * 16 + lr] = acc[i][j][r] + (epi.bias && n < N ? epi.bias[n] : 0.f);
        }
    __syncthreads();
    const int b = m0 >> 7;
    for (int idx = tid; idx < BN * epi.phw; idx += TPB) {
      const int nl = fdiv(idx, epi.fphw), q = idx - nl * epi.phw;
      if (n0 + nl >= N) break;
      const int py = fdiv(q, epi.fpw), px = q - py * epi.PW;
      const float* t = T + nl * LDT + py * epi.OW + px;
      const float v[4] = {t[0], t[1], t[epi.OW], t[epi.OW + 1]};
      float best = v[0];
      int bt = 0;
#pragma unroll
      for (int u = 1; u < 4; ++u)
        if (v[u] > best) { best = v[u]; bt = u; }
      const bool live = best > 0.f;
      const int64_t o = (static_cast<int64_t>(b) * N + n0 + nl) * epi.phw + q;
      epi.a[o] = live ? best : 0.f;
      epi.code[o] = live ? static_cast<unsigned char>(bt) : 255;
    }
  } else if constexpr (Epi::kPool) {
    const int tap = lr & 3;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm + i * 16 + lr;  // M is a multiple of 4: a window is all in or all out
      const int rowoff = epi.row(min(m, M - 1));
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + wn + j * 16 + 4 * lk + r;
          // bias before the max, exactly as conv-then-pool (argmax ties included)
          float best = acc[i][j][r] + (epi.bias && n < N ? epi.bias[n] : 0.f);
          int bt = tap;
          // first maximum in window order wins, as max_pool2d; quad lane exchanges by DPP
          pool_quad_step<0xB1>(best, bt);  // xor 1: quad_perm [1,0,3,2]
          pool_quad_step<0x4E>(best, bt);  // xor 2: quad_perm [2,3,0,1]
          if (tap == 0 && m < M && n < N) {
            const bool live = best > 0.f;
            epi.a[rowoff + n * epi.phw] = live ? best : 0.f;
            epi.code[rowoff + n * epi.phw] = live ? static_cast<unsigned char>(bt) : 255;
          }
        }
    }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm + i * 16 + lr;
      if (m >= M) continue;
      const int rowoff = epi.row(m);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + wn + j * 16 + 4 * lk + r;
          if (n < N) epi.store(rowoff, n, acc[i][j][r]);
        }
    }
  }
}

// Workgroup tile layouts (WM, WN waves of TM x TN MFMA tiles), chosen per GEMM by its narrow side.
enum Layout { L32x32K4, L256x32, L128x64, L64x128, L32x128 };

constexpr int layout_bm(Layout l) { return l == L256x32 ? 256 : l == L128x64 ? 128 : l == L64x128 ? 64 : 32; }
constexpr int layout_bn(Layout l) { return l == L256x32 ? 32 : l == L128x64 ? 64 : l == L32x32K4 ? 32 : 128; }

// Forward / data-gradient GEMMs: m = pixels (huge), n = channels.  Weight gradients: m = output
// channels, n = input channels x taps (+ bias column), k = batch x pixels.
Layout pick_layout(int M, int N, int slices) {
  if (M <= 32 && N <= 32) return L32x32K4;
  if (M <= 32) return L32x128;
  Layout l = L64x128;
  if (N <= 32) l = L256x32;
  else if (N <= 64 || M >= 128) l = L128x64;
  // Small batches (the reference's 100 images per rank): the big tiles leave most CUs idle with one
  // long K loop each (conv3's data gradient at B=100: 79 workgroups, 97 us); 32x32 tiles with the
  // k-range split over the 4 waves fill the chip instead.
  const int bm = l == L256x32 ? 256 : (l == L128x64 ? 128 : 64), bn = l == L256x32 ? 32 : (l == L128x64 ? 64 : 128);
  const long blocks = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  if (blocks * slices < f32_num_cus()) return L32x32K4;
  return l;
}

template <int WM, int WN, int TM, int TN, class LA, class LB, class Epi>
void launch_layout(int M, int N, int K, int per, int slices, int bias_col, const LA& la, const LB& lb,
                   const Epi& epi, hipStream_t s) {
  constexpr int BM = 16 * TM * WM, BN = 16 * TN * WN;
  dim3 grid(static_cast<unsigned>((M + BM - 1) / BM), static_cast<unsigned>((N + BN - 1) / BN),
            static_cast<unsigned>(slices));
  const int ktab_n = LA::kMC ? (K + BK - 1) / BK * BK : 0;
  hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, TM, TN, LA, LB, Epi>), grid, dim3(TPB), ktab_n * sizeof(int2), s, M,
                     N, K, per, ktab_n, bias_col, la, lb, epi);
}

template <class LA, class LB, class Epi>
void launch_gemm(int M, int N, int K, int per, int slices, int bias_col, const LA& la, const LB& lb,
                 const Epi& epi, hipStream_t s) {
  switch (pick_layout(M, N, slices)) {
    case L32x32K4: launch_layout<1, 1, 2, 2>(M, N, K, per, slices, bias_col, la, lb, epi, s); break;
    case L256x32: launch_layout<4, 1, 4, 2>(M, N, K, per, slices, bias_col, la, lb, epi, s); break;
    case L128x64: launch_layout<4, 1, 2, 4>(M, N, K, per, slices, bias_col, la, lb, epi, s); break;
    case L64x128: launch_layout<2, 2, 2, 4>(M, N, K, per, slices, bias_col, la, lb, epi, s); break;
    case L32x128: launch_layout<1, 4, 2, 2>(M, N, K, per, slices, bias_col, la, lb, epi, s); break;
  }
}

}  // namespace
}  // namespace ringdp::kern
