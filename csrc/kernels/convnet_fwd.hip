// MNIST ConvNet hot path for CDNA4 (gfx950): hand-written HIP, bf16 MFMA + LDS tiling.
//
// Model (ref/launch_dist.py:9-41):
//   conv1 1->32 k5 p1 (28->26) -> ReLU -> MaxPool(2,2) (13)
//   conv2 32->64 k3 (13->11)  -> ReLU -> MaxPool(2,1) (10)   [overlapping windows]
//   conv3 64->128 k3 (10->8)  -> ReLU -> MaxPool(2,2) (4)  -> view(-1, 2048) -> fc1 2048->10
//
// Kernel blocks (one autograd Function each, see ringdp/ops/convnet.py):
//   F1  conv1 + ReLU + pool1                       -> a1 [B,13,13,32] bf16 + argmax|relu byte
//   F2  conv2 + ReLU + pool2 (2x2/s1)              -> a2 [B,10,10,64] bf16 + pool2 code byte
//   F3  conv3 + ReLU + pool3, then fc1 (MFMA GEMM)  -> logits [B,10] fp32 (+ a3, argmax)
// conv2's pre-activation z2 is never materialised: F2 keeps only what F3 and the backward need
// (a2 = relu(pool2(z2)) and, per pooled value, the first-max position or "no gradient"), and F3's
// backward scatters d(a2) through those codes into dz2, a plain linear-layer gradient for conv2.
//
// MI355X-first design:
//   * weight-stationary: weights are packed once per forward (cn_pack_weights) into bf16 MFMA
//     B-fragment order; every workgroup keeps its fragments in VGPRs for all the images it
//     processes; images stream through LDS with one-image-ahead register prefetch;
//   * window-ordered M: the GEMM rows of a conv followed by a 2x2/s2 pool are ordered
//     (pool window, position-in-window), so each lane's 4 accumulator registers of a
//     v_mfma_f32_16x16x32_bf16 tile are exactly one pool window -> bias + max + argmax + ReLU are
//     done in registers (conv1, conv3), no LDS round trip;
//   * fc1 runs as a small MFMA GEMM over a3 (cheaper than reducing 10 logits across a workgroup);
//   * backward: dgrad is a weight-stationary full correlation over a zero-ringed LDS image; wgrad is
//     a TN GEMM whose operands are read with ds_read_b64_tr_b16 (the transposed read also does the
//     im2col gather), split over images into fp32 slabs reduced in a fixed order (deterministic);
//   * one multi-segment reduction launch per layer backward.
// Units: this file (weight pack, forward), convnet_bwd12.hip (F2 / F1 backward), convnet_bwd3.hip (F3 backward: fc1
// and conv3), convnet_reduce.hip (slab reduction, shared host helpers); shared: convnet_device.h, convnet_host.h.
#include "convnet_device.h"
#include "convnet_host.h"
#include "sgd_device.h"

namespace ringdp {
namespace kern {

namespace {

struct PackSrc {
  const float* w1;
  const float* w2;
  const float* w3;
  const float* wfc;
};

// fp32 master weight of packed element e
__device__ __forceinline__ float pack_value(int e, const PackSrc& ws) {
  const float* __restrict__ w1 = ws.w1;
  const float* __restrict__ w2 = ws.w2;
  const float* __restrict__ w3 = ws.w3;
  const float* __restrict__ wfc = ws.wfc;
  float v = 0.f;
  if (e < P2F_OFF) {  // [nt][ks][lane][8]: k = ks*32 + 8*(lane>>4) + j -> kh = ks*4 + (lane>>4), kw = j
    // n-tile nt, column c = channel 2c + nt: a lane's two accumulator tiles are a channel pair
    const int j = e & 7, lane = (e >> 3) & 63, ks = (e >> 9) & 1, nt = e >> 10;
    const int co = 2 * (lane & 15) + nt, kh = ks * 4 + (lane >> 4), kw = j;
    v = (kh < 5 && kw < 5) ? w1[co * 25 + kh * 5 + kw] : 0.f;
  } else if (e < P2D_OFF) {  // forward fragments of conv2 / conv3: B[k = tap*CIN + ci][n = co]
    const bool l2 = e < P3F_OFF;
    const int r = e - (l2 ? P2F_OFF : P3F_OFF);
    const int CIN = l2 ? 32 : 64, KS = l2 ? 9 : 18;
    const float* w = l2 ? w2 : w3;
    const int j = r & 7, lane = (r >> 3) & 63, ks = (r >> 9) % KS, nt = (r >> 9) / KS;
    const int co = nt * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + j;
    v = w[(co * CIN + k % CIN) * 9 + k / CIN];
  } else if (e >= P3D_OFF && e < PFC_OFF) {
    // conv3 dgrad, scatter form: A[row = ci][k = co] of tap t = W3[co][ci][t]; [ci tile][tap][kstep][lane][8]
    const int r = e - P3D_OFF;
    const int j = r & 7, lane = (r >> 3) & 63, ks = (r >> 9) % 36, nt = (r >> 9) / 36;
    const int ci = nt * 16 + (lane & 15), tap = ks >> 2, co = (ks & 3) * 32 + 8 * (lane >> 4) + j;
    v = w3[(co * 64 + ci) * 9 + tap];
  } else if (e < PFC_OFF) {  // dgrad fragments: B[k = tap'*COUT + co][n = ci] = W[co][ci][8 - tap']
    const bool l2 = e < P3D_OFF;
    const int r = e - (l2 ? P2D_OFF : P3D_OFF);
    const int CIN = l2 ? 32 : 64, COUT = l2 ? 64 : 128, KS = l2 ? 18 : 36;
    const float* w = l2 ? w2 : w3;
    const int j = r & 7, lane = (r >> 3) & 63, ks = (r >> 9) % KS, nt = (r >> 9) / KS;
    const int ci = nt * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + j;
    v = w[((k % COUT) * CIN + ci) * 9 + (8 - k / COUT)];
  } else if (e < PFF_OFF) {
    const int r = e - PFC_OFF;
    const int n = r % 10, co = (r / 10) % 128, wd = r / 1280;
    v = wfc[n * 2048 + co * 16 + wd];
  } else {  // [ks][lane][8]: B[k = ks*32 + 8*(lane>>4) + j][n = lane & 15], k = window*128 + co
    const int r = e - PFF_OFF;
    const int j = r & 7, lane = (r >> 3) & 63, ks = r >> 9;
    const int n = lane & 15, k = ks * 32 + 8 * (lane >> 4) + j;
    v = n < 10 ? wfc[n * 2048 + (k & 127) * 16 + (k >> 7)] : 0.f;
  }
  return v;
}

// packs elements [first, PACK_TOTAL) with `nblocks` workgroups (this one is `blk`), 4 per thread
__device__ __forceinline__ void pack_range(const PackSrc& ws, bf16* __restrict__ out, int first, int blk, int nblocks) {
  for (int e0 = first + 4 * (blk * 256 + (int)threadIdx.x); e0 < PACK_TOTAL; e0 += 4 * 256 * nblocks) {
    bf16x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (bf16)pack_value(e0 + j, ws);  // PACK_TOTAL % 4 == 0
    *reinterpret_cast<bf16x4*>(out + e0) = q;
  }
}
static_assert(PACK_TOTAL % 4 == 0 && P2F_OFF % 4 == 0, "packed regions in whole 8-B runs");

__global__ __launch_bounds__(256) void pack_weights_kernel(PackSrc ws, bf16* __restrict__ out) {
  pack_range(ws, out, 0, blockIdx.x, gridDim.x);
}

// The inverse of pack_value: the packed slots of one master weight element (conv1: 1, conv2 / conv3 / fc1: the
// forward and the backward copy), so the optimizer can write next step's fragments as it updates the fp32
// masters (no pack launch per forward).  `which`: 0 conv1 [32][1][5][5], 1 conv2 [64][32][3][3],
// 2 conv3 [128][64][3][3], 3 fc1 [10][2048]; l: the element's index in its tensor.  Padding slots (conv1
// taps past 5x5, fc1 columns past 10) never change: the first pack zeroed them.
__device__ __forceinline__ int frag_slot(int ks, int lane, int j, int nt, int KS) { return ((nt * KS + ks) * 64 + lane) * 8 + j; }
__device__ __forceinline__ void pack_scatter(int which, int l, bf16 v, bf16* __restrict__ out) {
  if (which == 0) {
    const int co = l / 25, r = l - co * 25, kh = r / 5, kw = r - kh * 5;
    out[P1_OFF + frag_slot(kh >> 2, ((kh & 3) << 4) | (co >> 1), kw, co & 1, 2)] = v;
  } else if (which == 1) {  // forward: k = tap*32 + ci; data gradient: k = (8 - tap)*64 + co, n = ci
    const int co = l / 288, ci = (l / 9) & 31, t = l % 9;
    const int kf = t * 32 + ci, kd = (8 - t) * 64 + co;
    out[P2F_OFF + frag_slot(kf >> 5, (((kf >> 3) & 3) << 4) | (co & 15), kf & 7, co >> 4, 9)] = v;
    out[P2D_OFF + frag_slot(kd >> 5, (((kd >> 3) & 3) << 4) | (ci & 15), kd & 7, ci >> 4, 18)] = v;
  } else if (which == 2) {  // forward: k = tap*64 + ci; data gradient (scatter form): ks = tap*4 + co/32
    const int co = l / 576, ci = (l / 9) & 63, t = l % 9;
    const int kf = t * 64 + ci;
    out[P3F_OFF + frag_slot(kf >> 5, (((kf >> 3) & 3) << 4) | (co & 15), kf & 7, co >> 4, 18)] = v;
    out[P3D_OFF + frag_slot(t * 4 + (co >> 5), (((co >> 3) & 3) << 4) | (ci & 15), co & 7, ci >> 4, 36)] = v;
  } else {  // fc1 column c = co*16 + window: backward [window][co][n], forward B fragments k = window*128 + co
    const int n = l >> 11, c = l & 2047, co = c >> 4, wd = c & 15;
    out[PFC_OFF + wd * 1280 + co * 10 + n] = v;
    const int k = wd * 128 + co;
    out[PFF_OFF + frag_slot(k >> 5, (((k >> 3) & 3) << 4) | n, k & 7, 0, 0)] = v;
  }
}

struct PackDst {
  bf16* out;
  int64_t off[4];  // each weight's first element in the flat parameter range
};
constexpr int kPackLen[4] = {32 * 25, 64 * 32 * 9, 128 * 64 * 9, 10 * 2048};

// SGD over a flat fp32 range (params / grads / momentum laid out identically, as elementwise.hip's
// sgd_flat_kernel) that also stores every updated ConvNet weight into its packed bf16 slots.
template <bool MOM>
__global__ __launch_bounds__(256) void cn_sgd_pack_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, int64_t n, SgdArgs a, PackDst d) {
  const SgdDev sd = load_sgd(a);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = MOM ? reinterpret_cast<float4*>(m)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    sgd_elem<MOM>(pv.x, gv.x, mv.x, sd);
    sgd_elem<MOM>(pv.y, gv.y, mv.y, sd);
    sgd_elem<MOM>(pv.z, gv.z, mv.z, sd);
    sgd_elem<MOM>(pv.w, gv.w, mv.w, sd);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (MOM) reinterpret_cast<float4*>(m)[i] = mv;
    const float v[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int64_t l0 = 4 * i - d.off[w];
      if (l0 + 3 < 0 || l0 >= kPackLen[w]) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (l0 + k >= 0 && l0 + k < kPackLen[w]) pack_scatter(w, (int)(l0 + k), (bf16)v[k], d.out);
    }
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pv = p[i], mv = MOM ? m[i] : 0.f;
    sgd_elem<MOM>(pv, g[i], mv, sd);
    p[i] = pv;
    if (MOM) m[i] = mv;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (i >= d.off[w] && i - d.off[w] < kPackLen[w]) pack_scatter(w, (int)(i - d.off[w]), (bf16)pv, d.out);
  }
}

// Packed 16-bit VALU ops (two channels per instruction).  The constant 1 of min(m - v, 1) is made opaque
// to the optimiser (an empty asm that "defines" it): with a visible constant, LLVM turns the min into a
// per-element compare + select and scalarises the whole chain (the pool2 loop of the fused forward was
// 130 VALU + 40 SALU per 8 channels; this form is ~66 v_pk_* VALU).  (Every op as inline asm instead
// compiles to the same VALU count plus an s_nop between dependent asm statements.)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 opaque_u16x2(uint32_t v) {
  asm volatile("" : "+v"(v));
  return __builtin_bit_cast(u16x2, v);
}

// relu(max over a 2x2 window) of 8 bf16 channels, plus the pool2 code byte per channel: one-hot bit
// dy*2+dx of the first maximum in (0,0),(0,1),(1,0),(1,1) order (torch max_pool2d semantics), 0 = the
// pooled value is 0 (no gradient flows).  Done on the raw bf16 bit patterns with packed int16
// ops (2 channels per instruction): for values >= 0 the integer order is the float order and any
// negative value is a negative int16, so max(v0..v3, 0) over int16 IS relu(max).  Per channel pair:
// k_i = min(m - v_i, 1) is 0 iff v_i == m (u16 difference; a negative v_i wraps to non-zero), the first
// index with v_i == m is k0 + k0 k1 + k0 k1 k2 = k0 + (k0 k1)(1 + k2), and the code is (1 << idx) * min(m, 1).
__device__ __forceinline__ void pool2_code8(const bf16* r0, int rs, int w, bf16x8& out, uint2& code) {
  const uint4 v0 = *reinterpret_cast<const uint4*>(r0);
  const uint4 v1 = *reinterpret_cast<const uint4*>(r0 + rs);
  const uint4 v2 = *reinterpret_cast<const uint4*>(r0 + w * rs);
  const uint4 v3 = *reinterpret_cast<const uint4*>(r0 + (w + 1) * rs);
  const u16x2 one = opaque_u16x2(0x00010001u);
  const uint32_t a[4] = {v0.x, v0.y, v0.z, v0.w}, b[4] = {v1.x, v1.y, v1.z, v1.w},
                 c[4] = {v2.x, v2.y, v2.z, v2.w}, d[4] = {v3.x, v3.y, v3.z, v3.w};
  // stage-major over the 4 channel pairs: dependent packed ops are never adjacent (gfx950 pads a packed
  // 16-bit result read by the next instruction with an s_nop, 4 cycles each)
  s16x2 sa[4], sb[4], sc[4], x0[4], x1[4], sm[4];
  u16x2 k0[4], k1[4], k2[4], t1[4], idx[4];
  uint32_t m[4], cd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sa[j] = __builtin_bit_cast(s16x2, a[j]);
    sb[j] = __builtin_bit_cast(s16x2, b[j]);
    sc[j] = __builtin_bit_cast(s16x2, c[j]);
    x0[j] = __builtin_elementwise_max(sa[j], sb[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) x1[j] = __builtin_elementwise_max(sc[j], __builtin_bit_cast(s16x2, d[j]));
#pragma unroll
  for (int j = 0; j < 4; ++j) sm[j] = __builtin_elementwise_max(x0[j], x1[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) sm[j] = __builtin_elementwise_max(sm[j], (s16x2)0);
#pragma unroll
  for (int j = 0; j < 4; ++j) k0[j] = __builtin_bit_cast(u16x2, sm[j]) - __builtin_bit_cast(u16x2, sa[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) k1[j] = __builtin_bit_cast(u16x2, sm[j]) - __builtin_bit_cast(u16x2, sb[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) k2[j] = __builtin_bit_cast(u16x2, sm[j]) - __builtin_bit_cast(u16x2, sc[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k0[j] = __builtin_elementwise_min(k0[j], one);
    k1[j] = __builtin_elementwise_min(k1[j], one);
    k2[j] = __builtin_elementwise_min(k2[j], one);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) t1[j] = k0[j] * k1[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) k2[j] = k2[j] + one;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = t1[j] * k2[j] + k0[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) t1[j] = __builtin_elementwise_min(__builtin_bit_cast(u16x2, sm[j]), one);
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = one << idx[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[j] = __builtin_bit_cast(uint32_t, sm[j]);
    cd[j] = __builtin_bit_cast(uint32_t, idx[j] * t1[j]);
  }
  out = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
  // codes (one per 16-bit half, < 16) -> 8 bytes: v_perm_b32 picks bytes 0 / 2 of two registers each
  code = make_uint2(__builtin_amdgcn_perm(cd[1], cd[0], 0x06040200u), __builtin_amdgcn_perm(cd[3], cd[2], 0x06040200u));
}

// First-max argmax over the 4 registers of a window + bias + ReLU (torch max_pool2d semantics:
// strict '>' keeps the first maximum in (0,0),(0,1),(1,0),(1,1) order).
__device__ __forceinline__ float pool4(const f32x4& c, float bias, int& arg) {
  float bm = c[0];
  arg = 0;
#pragma unroll
  for (int r = 1; r < 4; ++r)
    if (c[r] > bm) {
      bm = c[r];
      arg = r;
    }
  return fmaxf(bm + bias, 0.f);
}

// ================================================================== F1: conv1 (MFMA)
// relu(max) + argmax of a 2x2 window (the 4 accumulator registers of a window-ordered m-tile, bias
// included), as one signed-integer max over keys (bits(c_i) with the low 2 bits replaced by 3 - i): for
// positive values the int order is the float order, ties keep the first index (torch semantics), and a
// window whose maximum is <= 0 has no gradient, so its argmax is irrelevant.  Returns the pooled value's
// bits (<= 2 ulp of fp32 below the exact value) and the code byte (one-hot argmax, 0 if the ReLU is off).
__device__ __forceinline__ uint32_t pool4_key(const f32x4& c, uint32_t& code) {
  // v_bitop3_b32 0xBA = (S0 & ~S1) | S2: one instruction per key
  const int k0 = (int)__builtin_amdgcn_bitop3_b32(__float_as_uint(c[0]), 3u, 3u, 0xBA);
  const int k1 = (int)__builtin_amdgcn_bitop3_b32(__float_as_uint(c[1]), 3u, 2u, 0xBA);
  const int k2 = (int)__builtin_amdgcn_bitop3_b32(__float_as_uint(c[2]), 3u, 1u, 0xBA);
  const int k3 = (int)(__float_as_uint(c[3]) & ~3u);
  const int km = max(max(max(k0, k1), k2), max(k3, 0));  // two v_max3_i32
  code = km > 0 ? 1u << (~(uint32_t)km & 3u) : 0u;  // one-hot: bit dy*2+dx = where the gradient goes
  return (uint32_t)km;
}

// F1: 4 waves; per image 43 m-tiles of 16 window-ordered rows (169 windows), 2 n-tiles (channel pairs),
// K = 2 k-steps (filter rows 0-3 | 4).  Wave w owns m-tiles w, w+4, ..: their LDS offsets are
// computed once per workgroup and kept in registers.  Pooled outputs (one dword = 2 channels) and codes
// (2 bytes) are collected in LDS and written with 16-B stores; the next image's pixels are loaded into
// registers while this one computes.
constexpr int C1F_MT = 11;  // m-tiles per wave (wave 3: 10)
// copy stride padded 960 -> 1048 elements: the 16 A-row reads of a ds_read_b128 lane group then hit
// 2x fewer conflicting bank slots (modelled: 11.9 -> 8.2 LDS cycles per read, ideal 4)
constexpr int C1F_CS = 1048;
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));  // the builtin nontemporal store takes native vectors
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
// PACK: this launch also packs every layer's weights (cn_pack_weights) for the kernels after it: workgroups
// >= conv_blocks do only that, and the conv1 workgroups build their own fragments from the fp32 masters
// (one launch per step fewer; at the reference batch every launch is ~5 us of a ~100 us step).
template <bool U8, bool PACK>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const void* __restrict__ xin,
                                                        const bf16* __restrict__ packed,
                                                        const float* __restrict__ bias,
                                                        bf16* __restrict__ a1,
                                                        uint8_t* __restrict__ idx1, int B,
                                                        float mean, float inv_std, float in_scale,
                                                        PackSrc ws, bf16* __restrict__ pack_out,
                                                        int conv_blocks) {
  if (PACK && (int)blockIdx.x >= conv_blocks) {
    pack_range(ws, pack_out, 0, blockIdx.x - conv_blocks, gridDim.x - conv_blocks);
    return;
  }
  __shared__ __attribute__((aligned(16))) bf16 xs[2][8 * C1F_CS];
  __shared__ __attribute__((aligned(16))) uint32_t ot[172 * 16];      // rows >= 169: dropped tiles
  __shared__ __attribute__((aligned(16))) uint8_t ct[C1I_IMG + 64];   // + a dump row for them
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, gq = lane >> 4;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P1_OFF);
  bf16x8 bw[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (PACK) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bw[nt][ks][j] = (bf16)pack_value(P1_OFF + ((nt * 2 + ks) * 64 + lane) * 8 + j, ws);
      } else {
        bw[nt][ks] = pk[(nt * 2 + ks) * 64 + lane];
      }
    }
  const float bias0 = bias[2 * r16], bias1 = bias[2 * r16 + 1];
  const f32x4 bias0v = {bias0, bias0, bias0, bias0}, bias1v = {bias1, bias1, bias1, bias1};
  // per m-tile: A-row offset inside a copy buffer (elements; kh row added per k-step) and code offset
  int aoff[C1F_MT], coff[C1F_MT];
#pragma unroll
  for (int j = 0; j < C1F_MT; ++j) {
    const int mt = wave + 4 * j;
    const int w = min(4 * mt + (r16 >> 2), 168), i = r16 & 3;  // rows >= 676: clamped, dropped
    const int oh = 2 * (w / 13) + (i >> 1), ow = 2 * (w % 13) + (i & 1);
    aoff[j] = (ow & 7) * C1F_CS + oh * XC_W + (ow & ~7) + gq * XC_W;
    const int wc = 4 * mt + gq;
    coff[j] = wc < 169 ? (wc / 13) * 256 + r16 * 16 + wc % 13 : C1I_IMG + lane;
  }
  for (int i = tid; i < 2 * 8 * C1F_CS / 8; i += 256) reinterpret_cast<bf16x8*>(&xs[0][0])[i] = zero_bf16x8();
  for (int i = tid; i < C1I_IMG / 16; i += 256) reinterpret_cast<uint4*>(ct)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  uint32_t pu = 0;
  float4 pf = make_float4(0.f, 0.f, 0.f, 0.f);
  int b = blockIdx.x;
  if (b < B) {
    c1_load<U8>(xin, b, tid, pu, pf);
    c1_store<U8, 8, XC_W, C1F_CS>(xs[0], tid, pu, pf, mean, inv_std, in_scale);
  }
  __syncthreads();
  int cur = 0;
  const int nblk = PACK ? conv_blocks : (int)gridDim.x;
  for (; b < B; b += nblk) {
    const int nb = b + nblk;
    if (nb < B) c1_load<U8>(xin, nb, tid, pu, pf);
    const bf16* x = xs[cur];
    // software-pipelined: the MFMAs of tile j are issued before the epilogue of tile j-1
    auto epilogue = [&](int j, const f32x4& c0, const f32x4& c1) {
      uint32_t g0, g1;
      const uint32_t v0 = pool4_key(c0, g0), v1 = pool4_key(c1, g1);
      const bf16x2v pv = __builtin_convertvector(f32x2v{__uint_as_float(v0), __uint_as_float(v1)}, bf16x2v);
      ot[(4 * (wave + 4 * j) + gq) * 16 + r16] = __builtin_bit_cast(uint32_t, pv);  // v_cvt_pk_bf16_f32
      ct[coff[j]] = (uint8_t)(g0 | (g1 << 4));
    };
    f32x4 p0 = zero_f32x4(), p1 = zero_f32x4();
#pragma unroll
    for (int j = 0; j < C1F_MT; ++j) {
      f32x4 c0 = bias0v, c1 = bias1v;  // the bias rides in the accumulator (one channel per lane)
      const bool live = j < C1F_MT - 1 || wave < 3;  // wave-uniform
      if (live) {
        const bf16* xr = x + aoff[j];
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(xr);
        const bf16x8 a1v = *reinterpret_cast<const bf16x8*>(xr + (4 - gq) * XC_W);  // filter row 4
        c0 = mfma16x16x32(a0, bw[0][0], c0);
        c1 = mfma16x16x32(a0, bw[1][0], c1);
        c0 = mfma16x16x32(a1v, bw[0][1], c0);
        c1 = mfma16x16x32(a1v, bw[1][1], c1);
      }
      if (j > 0) epilogue(j - 1, p0, p1);
      if (live && j == C1F_MT - 1) epilogue(j, c0, c1);
      p0 = c0;
      p1 = c1;
    }
    if (nb < B) c1_store<U8, 8, XC_W, C1F_CS>(xs[cur ^ 1], tid, pu, pf, mean, inv_std, in_scale);
    __syncthreads();  // output tile complete; next image's copies written
    const uint4* os = reinterpret_cast<const uint4*>(ot);
    uint4* og = reinterpret_cast<uint4*>(a1 + (int64_t)b * C1A_IMG);
    for (int c = tid; c < C1A_IMG / 8; c += 256) og[c] = os[c];
    const uint4* cs = reinterpret_cast<const uint4*>(ct);
    uint4* cg = reinterpret_cast<uint4*>(idx1 + (int64_t)b * C1I_IMG);
    for (int c = tid; c < C1I_IMG / 16; c += 256) cg[c] = cs[c];
    __syncthreads();  // output tile read out before the next image overwrites it
    cur ^= 1;
  }
}

// ================================================================== F2: conv2 + ReLU + pool2
// 256 threads; wave (wm, wn) owns n-tiles {2wn, 2wn+1} x m-tiles {4wm..4wm+3} (121 rows -> 128).
// forward m-tile -> output position map (255 = padding row): every full tile holds two positions of
// each residue (y*13 + x) mod 8, one among lanes {0-3,12-15} and one among {4-11}, so with 96-B rows
// the 16 rows of a ds_read_b128 lane group land on 16 distinct 16-B bank slots (modelled 10.5 -> 4
// LDS cycles per operand read; generator: tools/lds_bank_model.py)
__constant__ uint8_t c2f_tile_pos[128] = {0,3,6,1,8,17,12,9,18,13,10,11,4,7,2,5,14,23,20,15,28,31,26,29,32,27,22,25,24,21,16,19,34,37,40,35,42,51,46,43,44,41,36,45,38,33,30,39,48,57,54,49,62,65,60,55,58,61,56,59,52,47,50,53,68,71,66,63,76,77,74,69,78,75,70,79,72,67,64,73,82,85,80,83,88,91,94,89,92,95,90,93,86,81,84,87,96,105,100,97,102,111,108,103,112,109,104,107,106,101,98,99,116,119,114,117,255,255,255,255,255,255,118,255,120,115,110,113};
constexpr int C2_CRS = 72;  // bf16 per LDS row of the output staging tile (64 + 8)

__global__ __launch_bounds__(256, 3) void conv2_fwd_kernel(const bf16* __restrict__ a1,
                                                           const bf16* __restrict__ packed,
                                                           const float* __restrict__ bias,
                                                           bf16* __restrict__ a2, uint8_t* __restrict__ idx2,
                                                           int B) {
  __shared__ __attribute__((aligned(16))) bf16 X[2][169 * C2_XRS];
  __shared__ __attribute__((aligned(16))) bf16 Cs[121 * C2_CRS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q8 = (lane >> 4) * 8;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P2F_OFF);
  bf16x8 bw[2][9];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 9; ++ks) bw[t][ks] = pk[((2 * wn + t) * 9 + ks) * 64 + lane];
  // operands swapped (weights = A): a lane's 4 accumulators are 4 consecutive channels of one
  // position, staged with one 8-byte LDS store
  const int c4 = (lane >> 4) * 4;
  f32x4 bv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[t][i] = bias[(2 * wn + t) * 16 + c4 + i];
  int base[4], opos[4];  // padding rows read a valid address; their outputs are dropped
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    opos[mt] = c2f_tile_pos[(4 * wm + mt) * 16 + r16];
    const int mm = opos[mt] == 255 ? 0 : opos[mt];
    base[mt] = (mm / 11) * 13 + mm % 11;
  }
  bf16x8 pre[3];
  auto load = [&](int bb) {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(a1 + (int64_t)bb * 169 * 32);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = tid + 256 * k;
      if (c < 676) pre[k] = src[c];
    }
  };
  auto store = [&](bf16* dst) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = tid + 256 * k;
      if (c < 676) *reinterpret_cast<bf16x8*>(dst + (c >> 2) * C2_XRS + (c & 3) * 8) = pre[k];
    }
  };
  int b = blockIdx.x;
  if (b < B) {
    load(b);
    store(X[0]);
  }
  __syncthreads();
  int cur = 0;
  for (; b < B; b += gridDim.x) {
    const int nb = b + gridDim.x;
    if (nb < B) load(nb);
    const bf16* x = X[cur];
    f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = zero_f32x4();
#pragma unroll
    for (int ks = 0; ks < 9; ++ks) {
      const int shift = (ks / 3) * 13 + ks % 3;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(x + (base[mt] + shift) * C2_XRS + q8);
        acc[mt][0] = mfma16x16x32(bw[0][ks], a, acc[mt][0]);
        acc[mt][1] = mfma16x16x32(bw[1][ks], a, acc[mt][1]);
      }
    }
    __syncthreads();  // previous image's pooling reads of Cs are complete
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = opos[mt];
      if (m < 121) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const f32x4 v = acc[mt][t] + bv[t];
          *reinterpret_cast<bf16x4*>(Cs + m * C2_CRS + (2 * wn + t) * 16 + c4) =
              bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
        }
      }
    }
    if (nb < B) store(X[cur ^ 1]);
    __syncthreads();
    // relu + overlapping 2x2/s1 pool of the staged z2 tile -> a2 and the pool2 codes
    bf16x8* da = reinterpret_cast<bf16x8*>(a2 + (int64_t)b * 6400);
    uint2* di = reinterpret_cast<uint2*>(idx2 + (int64_t)b * 6400);
    for (int it = tid; it < 800; it += 256) {
      const int p = it >> 3, c = (it & 7) * 8;
      bf16x8 v;
      uint2 code;
      pool2_code8(Cs + ((p / 10) * 11 + p % 10) * C2_CRS + c, C2_CRS, 11, v, code);
      da[it] = v;
      di[it] = code;
    }
    cur ^= 1;
  }
}

// ================================================================== F3: conv3 + ReLU + pool3 + fc1
// 256 threads; wave w owns output channels 32w..32w+31 (n-tiles 2w, 2w+1) for all 16 pool windows.
// conv3 forward A-operand image: 160-B rows and this pool-window order of the m-tiles make every
// ds_read_b128 fragment read conflict-free (modelled with the b128 lane groups of MI355X_MICROARCH.md:
// 1.0 LDS cycles per read, was 2.0 with 144-B rows and the natural window order; the measured
// SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_LDS was 3.0).  Entry 4*mt + j = the pool window (row-major
// in the 4x4 window grid) whose 4 positions are rows 4j..4j+3 of m-tile mt.
constexpr int C3F_XRS = 80;
__constant__ uint8_t c3f_win[16] = {1, 9, 13, 11, 10, 3, 15, 8, 7, 12, 0, 5, 4, 6, 2, 14};

// FC (small batches): fc1 runs in this launch too.  Each lane multiplies its 8 pooled values by their
// 10 fc1 weights (the [window][co][n] pack, staged in LDS once per workgroup) and the 256 lanes' partial
// logits are summed through LDS in a fixed order.  At B <= a few thousand the separate fc1 launch (and
// its ~1.5 us kernel boundary) cost more than this; at large B the MFMA fc1 pass over a3 is cheaper.
constexpr int C3F_FCW = 16 * 128 * 10;  // bf16 fc1 weights in LDS
template <bool FC>
__global__ __launch_bounds__(256, 2) void conv3_fwd_kernel(const bf16* __restrict__ a2,
                                                           const bf16* __restrict__ packed,
                                                           const float* __restrict__ bias,
                                                           bf16* __restrict__ a3,
                                                           uint8_t* __restrict__ idx3, int B,
                                                           const float* __restrict__ bfc,
                                                           float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) bf16 R[100 * 64];
  __shared__ __attribute__((aligned(16))) bf16 X[100 * C3F_XRS];
  __shared__ __attribute__((aligned(16))) char fcs[FC ? C3F_FCW * 2 + 10 * 256 * 4 : 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bf16* fw = reinterpret_cast<bf16*>(fcs);                      // [window][co][n]
  float* fred = reinterpret_cast<float*>(fcs + C3F_FCW * 2);    // [n][256 lanes]
  if (FC) {
    const uint4* src = reinterpret_cast<const uint4*>(packed + PFC_OFF);
    for (int c = tid; c < C3F_FCW / 8; c += 256) reinterpret_cast<uint4*>(fw)[c] = src[c];
  }
  const int r16 = lane & 15, q8 = (lane >> 4) * 8;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P3F_OFF);
  bf16x8 bw[2][18];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) bw[t][ks] = pk[((2 * wave + t) * 18 + ks) * 64 + lane];
  float bv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) bv[t] = bias[32 * wave + 16 * t + r16];
  int base[4], wcol[4];  // A row of this lane per m-tile; pool window of this lane's accumulators
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    base[mt] = win_pos(4 * c3f_win[4 * mt + (r16 >> 2)] + (r16 & 3), 10);
    wcol[mt] = c3f_win[4 * mt + (lane >> 4)];
  }
  int b = blockIdx.x;
  if (b < B) a2_glds(a2, b, R, wave, lane, 4);
  for (; b < B; b += gridDim.x) {
    c_dma_wait();
    __syncthreads();  // R has landed; the previous image's X reads are done
    a2_relayout<C3F_XRS>(R, X, tid, 256);
    __syncthreads();  // X complete, R free
    const int nb = b + gridDim.x;
    if (nb < B) a2_glds(a2, nb, R, wave, lane, 4);  // lands while the MFMAs below run
    f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = zero_f32x4();
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) {
      const int tap = ks >> 1, c0 = (ks & 1) * 32;
      const int shift = (tap / 3) * 10 + tap % 3;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(X + (base[mt] + shift) * C3F_XRS + c0 + q8);
        acc[mt][0] = mfma16x16x32(a, bw[0][ks], acc[mt][0]);
        acc[mt][1] = mfma16x16x32(a, bw[1][ks], acc[mt][1]);
      }
    }
    float part[10];
#pragma unroll
    for (int n = 0; n < 10; ++n) part[n] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int wc = wcol[mt], co = 32 * wave + 16 * t + r16;
        int g;
        const bf16 pb = (bf16)pool4(acc[mt][t], bv[t], g);
        const int64_t o = ((int64_t)b * 16 + wc) * 128 + co;
        a3[o] = pb;
        idx3[o] = (uint8_t)g;
        if (FC) {
          const float pv = (float)pb;
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(fw + (wc * 128 + co) * 10);  // 4-B aligned
#pragma unroll
          for (int h = 0; h < 5; ++h) {
            const uint32_t u = wp[h];
            part[2 * h] = fmaf(pv, __uint_as_float(u << 16), part[2 * h]);
            part[2 * h + 1] = fmaf(pv, __uint_as_float(u & 0xffff0000u), part[2 * h + 1]);
          }
        }
      }
    if (FC) {
#pragma unroll
      for (int n = 0; n < 10; ++n) fred[n * 256 + tid] = part[n];
      __syncthreads();
      // 160 threads: logit n = t >> 4 sums lanes c + 16 i (i < 16), then 16 lanes combine by shuffles
      if (tid < 160) {
        const int n = tid >> 4, c = tid & 15;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) v += fred[n * 256 + c + 16 * i];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (c == 0) logits[(int64_t)b * 10 + n] = v + bfc[n];
      }
      // the next image's top barrier orders these reads before fred is rewritten
    }
  }
}

// fc1 as its own MFMA GEMM: logits[b][n] = sum_k a3[b][k] * Wfc'[k][n] + bfc[n], k = window*128 + co.
// One wave per 16 images; A fragments stream straight from global (16 B per lane, no LDS), the
// 64 B-fragments (N = 10 padded to 16) sit in LDS.  Unfused from conv3 because reducing 10 logits
// across 256 lanes per image cost the conv3 kernel more than this whole pass over a3.
constexpr int FC1_G = 8;  // 16-image groups per workgroup
__global__ __launch_bounds__(256) void fc1_fwd_kernel(const bf16* __restrict__ a3,
                                                      const bf16* __restrict__ packed,
                                                      const float* __restrict__ bfc,
                                                      float* __restrict__ logits, int B) {
  // The 4 waves split K (512 each) and hold their 16 B-fragments in VGPRs, loaded once from the
  // L2-resident pack.  A bandwidth-bound pass over a3 (4 KB per image): group g+1's A fragments are
  // loaded while group g's MFMAs and cross-wave sum run (two register sets; one set in flight had run at
  // ~2.9 TB/s).  Partials are summed in a fixed order.
  __shared__ f32x4 red[2][3][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16x8* src = reinterpret_cast<const bf16x8*>(packed + PFF_OFF);
  bf16x8 w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = src[(wave * 16 + j) * 64 + lane];
  const int g0 = blockIdx.x * FC1_G;
  const int ng = min(FC1_G, cdiv(B, 16) - g0);
  auto load = [&](int g, bf16x8 (&av)[16]) {
    const int row = min((g0 + g) * 16 + (lane & 15), B - 1);
    const bf16x8* ap = reinterpret_cast<const bf16x8*>(a3 + (int64_t)row * 2048) + (lane >> 4) + wave * 64;
#pragma unroll
    for (int j = 0; j < 16; ++j) av[j] = ap[j * 4];
  };
  auto group = [&](int g, const bf16x8 (&av)[16]) {
    const int b0 = (g0 + g) * 16;
    f32x4 acc0 = zero_f32x4(), acc1 = zero_f32x4();
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
      acc0 = mfma16x16x32(av[j], w[j], acc0);
      acc1 = mfma16x16x32(av[j + 1], w[j + 1], acc1);
    }
    const f32x4 acc = acc0 + acc1;
    if (wave > 0) red[g & 1][wave - 1][lane] = acc;  // two slots: one barrier per group
    __syncthreads();
    if (wave == 0) {
      const f32x4 t = acc + red[g & 1][0][lane] + red[g & 1][1][lane] + red[g & 1][2][lane];
      const int nn = lane & 15;
      if (nn < 10) {
        const float bn = bfc[nn];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int bb = b0 + (lane >> 4) * 4 + i;
          if (bb < B) logits[(int64_t)bb * 10 + nn] = t[i] + bn;
        }
      }
    }
  };
  bf16x8 va[16], vb[16];
  if (ng > 0) load(0, va);
  for (int g = 0; g < ng; g += 2) {  // unrolled by 2: register sets are not indexable
    if (g + 1 < ng) load(g + 1, vb);
    group(g, va);
    if (g + 1 < ng) {
      if (g + 2 < ng) load(g + 2, va);
      group(g + 1, vb);
    }
  }
}

// ================================================================== F1+F2+F3: fused forward
// The whole forward of one image in one 512-thread workgroup, a1 / a2 never re-read from HBM (the
// three separate launches move 64 KB per image, this one 40 KB: the forward is HBM- as much as
// MFMA-bound).  Waves 0-3 are the PRODUCER (conv1 + pool1, conv2 + pool2 of image s), waves 4-7 the
// CONSUMER (conv3 + pool3 + fc1 of image s-1, one step behind).  A step is three barrier-separated
// phases, the same barriers for both halves:
//   phase 1  producer: conv1 MFMAs on the staged input -> pooled a1 straight into conv2's operand
//                      rows (X2) + codes (CT)               consumer: conv3 k-steps 0-8 of image s-1
//   phase 2  producer: next input -> XS; a1 / idx1 -> HBM; conv2 MFMAs -> Cs
//                                                           consumer: conv3 k-steps 9-17
//   phase 3  producer: pool2 of Cs -> a2 / idx2 (HBM) and conv3's operand rows X3
//                                                           consumer: pool3 -> a3 / idx3, fc1 partials
// Each LDS buffer has one writer phase and its readers in other phases, so every buffer is single.
// The layouts are the separate kernels' (conv1_fwd_kernel / conv2_fwd_kernel / conv3_fwd_kernel<true>).
constexpr int FF_XS = 8 * C1F_CS * 2;      // 16768: conv1 input, 8 shifted copies
constexpr int FF_X2 = 172 * C2_XRS * 2;    // 16512: a1 in conv2 operand rows (+3 dump rows)
constexpr int FF_CT = C1I_IMG + 64;        // 3392: conv1 codes (+ dump row)
constexpr int FF_CS = 121 * C2_CRS * 2;    // 17424: conv2 output tile
constexpr int FF_X3H = 100 * C3F_XRS;      // bf16 per a2 image in conv3 operand rows (16000 B)
constexpr int FF_X3 = 2 * FF_X3H * 2;      // double-buffered: the consumer reads image s-1 while image s lands
constexpr int FF_FW = C3F_FCW * 2;         // 40960: fc1 weights [window][co][n]
constexpr int FF_FR = 10 * 256 * 4;        // 10240: fc1 partial logits [n][256]
constexpr int FF_OFF_X2 = FF_XS, FF_OFF_CT = FF_OFF_X2 + FF_X2, FF_OFF_CS = FF_OFF_CT + FF_CT,
              FF_OFF_X3 = FF_OFF_CS + FF_CS, FF_OFF_FW = FF_OFF_X3 + FF_X3, FF_OFF_FR = FF_OFF_FW + FF_FW;
constexpr int FF_LDS = FF_OFF_FR + FF_FR;  // 137296
static_assert(FF_OFF_X2 % 16 == 0 && FF_OFF_CT % 16 == 0 && FF_OFF_CS % 16 == 0 && FF_OFF_X3 % 16 == 0 &&
                  FF_OFF_FW % 16 == 0 && FF_LDS <= 160 * 1024,
              "fused forward LDS");

// RINGDP_FF_STAMPS (diagnostic builds only, tools/build_variant.py): lane 0 of every wave records s_memtime at
// the 7 phase points of steps [FF_ST_S0, FF_ST_S0 + 8) into LDS past FF_LDS; workgroup FF_ST_BLK prints them
// at the end (per-phase time of the producer and consumer roles)
#ifdef RINGDP_FF_STAMPS
constexpr int FF_ST_S0 = 100, FF_ST_BLK = 5, FF_ST_BYTES = 8 * 8 * 8 * 8;
#define FF_ST(k) CN_STAMP(FF_LDS, FF_ST_S0, 8, s, k)
#else
constexpr int FF_ST_BYTES = 0;
#define FF_ST(k) do {} while (0)
#endif

// RINGDP_FF_ABLATE (diagnostic builds only, tools/build_variant.py; timing only, wrong results): bit 0 empties
// the producer role, bit 1 the consumer role.  A compile-time constant, 0 in every normal build: nothing reads
// the environment for it and no launch argument can select it.
#ifndef RINGDP_FF_ABLATE
#define RINGDP_FF_ABLATE 0
#endif
constexpr int FF_ABLATE = RINGDP_FF_ABLATE;

__device__ __forceinline__ bf16x8 ff_frag(const bf16* __restrict__ packed, int off, int lane) {
  return reinterpret_cast<const bf16x8*>(packed + off)[lane];
}

// pool2 + ReLU of the staged conv2 tile (800 items: position p, 8-channel chunk) -> a2 / idx2 in HBM and the
// conv3 operand rows of buffer X3b.  All of it is the producer's phase 3: the consumer's phase 3 holds no pool2
// code beside conv3's 144 weight registers (phase 3 is consumer-bound, profiles/r06/fwd_stamps.md; giving the
// consumer a share of the items measured no faster, profiles/r06/fwd_pool2/p2_resweep.txt).
__device__ __forceinline__ void ff_pool2(const bf16* Cs, bf16* X3b, bf16* __restrict__ a2, uint8_t* __restrict__ idx2,
                                         int b, int t) {
  // uniform per-image bases, 32-bit per-item offsets (no 64-bit address math per item); 3 or 4 items per
  // thread (800 items, the producer's 256 threads)
  bf16x8* da = reinterpret_cast<bf16x8*>(a2 + (int64_t)b * 6400);
  uint2* di = reinterpret_cast<uint2*>(idx2 + (int64_t)b * 6400);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int it = t + 256 * k;
    if (it >= 800) break;
    const int p = it >> 3, c = (it & 7) * 8;
    const int y = (p * 205) >> 11;  // p / 10 for p < 100
    bf16x8 v;
    uint2 code;
    pool2_code8(Cs + (p + y) * C2_CRS + c, C2_CRS, 11, v, code);  // row y * 11 + (p - 10 y) = p + y
    __builtin_nontemporal_store(v, &da[it]);  // streamed: see ff_producer's a1 / idx1 copy-out
    __builtin_nontemporal_store(u32x2v{code.x, code.y}, reinterpret_cast<u32x2v*>(&di[it]));
    *reinterpret_cast<bf16x8*>(X3b + p * C3F_XRS + c) = v;
  }
}

template <bool U8>
__device__ __forceinline__ void ff_producer(char* smem, const void* __restrict__ xin, const bf16* __restrict__ packed,
                            const float* __restrict__ b1, const float* __restrict__ b2,
                            bf16* __restrict__ a1, uint8_t* __restrict__ idx1, bf16* __restrict__ a2,
                            uint8_t* __restrict__ idx2, int B, int b0, int bstep, int nsteps, float mean,
                            float inv_std, float in_scale) {
  bf16* XS = reinterpret_cast<bf16*>(smem);
  bf16* X2 = reinterpret_cast<bf16*>(smem + FF_OFF_X2);
  uint32_t* X2u = reinterpret_cast<uint32_t*>(X2);
  uint8_t* CT = reinterpret_cast<uint8_t*>(smem + FF_OFF_CT);
  bf16* Cs = reinterpret_cast<bf16*>(smem + FF_OFF_CS);
  bf16* X3 = reinterpret_cast<bf16*>(smem + FF_OFF_X3);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // tid < 256
  const int r16 = lane & 15, gq = lane >> 4;
  // ---- conv1 setup (conv1_fwd_kernel)
  bf16x8 bw1[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) bw1[nt][ks] = ff_frag(packed, P1_OFF + (nt * 2 + ks) * 512, lane);
  const float c1b0 = b1[2 * r16], c1b1 = b1[2 * r16 + 1];
  const f32x4 bias0v = {c1b0, c1b0, c1b0, c1b0}, bias1v = {c1b1, c1b1, c1b1, c1b1};
  int aoff[C1F_MT], coff[C1F_MT];
#pragma unroll
  for (int j = 0; j < C1F_MT; ++j) {
    const int mt = wave + 4 * j;
    const int w = min(4 * mt + (r16 >> 2), 168), i = r16 & 3;
    const int oh = 2 * (w / 13) + (i >> 1), ow = 2 * (w % 13) + (i & 1);
    aoff[j] = (ow & 7) * C1F_CS + oh * XC_W + (ow & ~7) + gq * XC_W;
    const int wc = 4 * mt + gq;
    coff[j] = wc < 169 ? (wc / 13) * 256 + r16 * 16 + wc % 13 : C1I_IMG + lane;
  }
  // ---- conv2 setup (conv2_fwd_kernel)
  const int wm = wave >> 1, wn = wave & 1, q8 = (lane >> 4) * 8, c4 = (lane >> 4) * 4;
  bf16x8 bw2[2][9];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 9; ++ks) bw2[t][ks] = ff_frag(packed, P2F_OFF + ((2 * wn + t) * 9 + ks) * 512, lane);
  f32x4 bv2[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv2[t][i] = b2[(2 * wn + t) * 16 + c4 + i];
  int base2[4], opos2[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    opos2[mt] = c2f_tile_pos[(4 * wm + mt) * 16 + r16];
    const int mm = opos2[mt] == 255 ? 0 : opos2[mt];
    base2[mt] = (mm / 11) * 13 + mm % 11;
  }
  // zero ring of the input copies and the never-written code columns (px 13..15), once
  for (int i = tid; i < FF_XS / 16; i += 256) reinterpret_cast<bf16x8*>(XS)[i] = zero_bf16x8();
  for (int i = tid; i < C1I_IMG / 16; i += 256) reinterpret_cast<uint4*>(CT)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();  // [S0a] zeroing before the first input store
  uint32_t pu = 0;
  float4 pf = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b0 < B) {
    c1_load<U8>(xin, b0, tid, pu, pf);
    c1_store<U8, 8, XC_W, C1F_CS>(XS, tid, pu, pf, mean, inv_std, in_scale);
  }
  __syncthreads();  // [S0b] first input staged
  for (int s = 0; s < nsteps; ++s) {
    const int b = b0 + s * bstep;
    const bool live = b < B;
    const int nb = b + bstep;
    FF_ST(0);
    // ---------------- phase 1: conv1 -> X2 / CT
    if (live) {
      if (nb < B) c1_load<U8>(xin, nb, tid, pu, pf);
      auto epilogue = [&](int j, const f32x4& c0, const f32x4& c1) {
        uint32_t g0, g1;
        const uint32_t v0 = pool4_key(c0, g0), v1 = pool4_key(c1, g1);
        const bf16x2v pv = __builtin_convertvector(f32x2v{__uint_as_float(v0), __uint_as_float(v1)}, bf16x2v);
        X2u[(4 * (wave + 4 * j) + gq) * (C2_XRS / 2) + r16] = __builtin_bit_cast(uint32_t, pv);
        CT[coff[j]] = (uint8_t)(g0 | (g1 << 4));
      };
      f32x4 p0 = zero_f32x4(), p1 = zero_f32x4();
#pragma unroll
      for (int j = 0; j < C1F_MT; ++j) {
        f32x4 c0 = bias0v, c1 = bias1v;
        const bool lv = j < C1F_MT - 1 || wave < 3;
        if (lv) {
          const bf16* xr = XS + aoff[j];
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(xr);
          const bf16x8 a1v = *reinterpret_cast<const bf16x8*>(xr + (4 - gq) * XC_W);
          c0 = mfma16x16x32(a0, bw1[0][0], c0);
          c1 = mfma16x16x32(a0, bw1[1][0], c1);
          c0 = mfma16x16x32(a1v, bw1[0][1], c0);
          c1 = mfma16x16x32(a1v, bw1[1][1], c1);
        }
        if (j > 0) epilogue(j - 1, p0, p1);
        if (lv && j == C1F_MT - 1) epilogue(j, c0, c1);
        p0 = c0;
        p1 = c1;
      }
    }
    FF_ST(1);
    __syncthreads();  // [S1] X2 / CT complete, XS free
    FF_ST(2);
    // ---------------- phase 2: next input; a1 / idx1 out; conv2 -> Cs
    f32x4 acc[4][2];
    if (live) {
      if (nb < B) c1_store<U8, 8, XC_W, C1F_CS>(XS, tid, pu, pf, mean, inv_std, in_scale);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = zero_f32x4();
#pragma unroll
      for (int ks = 0; ks < 9; ++ks) {
        const int shift = (ks / 3) * 13 + ks % 3;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(X2 + (base2[mt] + shift) * C2_XRS + q8);
          acc[mt][0] = mfma16x16x32(bw2[0][ks], a, acc[mt][0]);
          acc[mt][1] = mfma16x16x32(bw2[1][ks], a, acc[mt][1]);
        }
      }
      // a1 / idx1 to HBM while the MFMAs drain.  These and pool2's a2 / idx2 (33.5 of the 39.5 KB an image
      // writes) are next read by the backward kernels, after more traffic than the Infinity Cache holds, so
      // they are nontemporal stores: as plain stores they were still being written back to HBM while
      // fc1_fwd_kernel streamed a3 (B=65536: that pass 94 -> 53 us, this kernel unchanged;
      // profiles/r15/head_bytes/README.md).  a3 / idx3 stay plain: nontemporal 2-B / 1-B stores cost this
      // kernel 9 us.
      u32x4v* og = reinterpret_cast<u32x4v*>(a1 + (int64_t)b * C1A_IMG);
      for (int c = tid; c < C1A_IMG / 8; c += 256)
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4v*>(X2 + (c >> 2) * C2_XRS + (c & 3) * 8), og + c);
      const u32x4v* cs = reinterpret_cast<const u32x4v*>(CT);
      u32x4v* cg = reinterpret_cast<u32x4v*>(idx1 + (int64_t)b * C1I_IMG);
      for (int c = tid; c < C1I_IMG / 16; c += 256) __builtin_nontemporal_store(cs[c], cg + c);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int m = opos2[mt];
        if (m < 121) {
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 v = acc[mt][t] + bv2[t];
            *reinterpret_cast<bf16x4*>(Cs + m * C2_CRS + (2 * wn + t) * 16 + c4) =
                bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
          }
        }
      }
    }
    FF_ST(3);
    __syncthreads();  // [S2] Cs complete
    FF_ST(4);
    // ---------------- phase 3: pool2 -> a2 / idx2 (HBM) + X3
    if (live) ff_pool2(Cs, X3 + (s & 1) * FF_X3H, a2, idx2, b, tid);
    FF_ST(5);
    __syncthreads();  // [S3] X3 complete; Cs, X2, CT free
    FF_ST(6);
  }
}

// the consumer's conv3 k-steps per phase: [0, KA) beside conv1, [KA, KB) beside conv2, [KB, 18) beside pool2
// (other splits measured the same within noise, profiles/r06/rejected/README.md)
constexpr int FF_KA = 4, FF_KB = 11;
__device__ __forceinline__ void ff_consumer(char* smem, const bf16* __restrict__ packed,
                            const float* __restrict__ b3, const float* __restrict__ bfc, bf16* __restrict__ a3,
                            uint8_t* __restrict__ idx3, float* __restrict__ logits, int B, int b0, int bstep,
                            int nsteps) {
  bf16* X3 = reinterpret_cast<bf16*>(smem + FF_OFF_X3);
  bf16* fw = reinterpret_cast<bf16*>(smem + FF_OFF_FW);
  float* fred = reinterpret_cast<float*>(smem + FF_OFF_FR);
  const int tid = threadIdx.x - 256, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q8 = (lane >> 4) * 8;
  // fc1 in this launch unless logits == nullptr (large batches: fc1_fwd_kernel, an MFMA pass over a3, takes
  // its ~200 VALU per lane and image out of phase 1, where the producer's conv1 epilogue is VALU-bound too)
  const bool fc = logits != nullptr;
  if (fc) {
    const uint4* src = reinterpret_cast<const uint4*>(packed + PFC_OFF);
    for (int c = tid; c < C3F_FCW / 8; c += 256) reinterpret_cast<uint4*>(fw)[c] = src[c];
  }
  bf16x8 bw[2][18];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) bw[t][ks] = ff_frag(packed, P3F_OFF + ((2 * wave + t) * 18 + ks) * 512, lane);
  float bv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) bv[t] = b3[32 * wave + 16 * t + r16];
  const float bn = tid < 160 ? bfc[tid >> 4] : 0.f;
  int base[4], wcol[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    base[mt] = win_pos(4 * c3f_win[4 * mt + (r16 >> 2)] + (r16 & 3), 10);
    wcol[mt] = c3f_win[4 * mt + (lane >> 4)];
  }
  __syncthreads();  // [S0a]
  __syncthreads();  // [S0b]  (fw is complete past these)
  auto fc_reduce = [&](int bb) {  // after a barrier that follows the fred writes of image bb
    if (tid < 160) {
      const int n = tid >> 4, c = tid & 15;
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) v += fred[n * 256 + c + 16 * i];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (c == 0) logits[(int64_t)bb * 10 + n] = v + bn;
    }
  };
  f32x4 acc[4][2];
  // conv3 k-steps [k0, k1) of the image in buffer xb
  auto mfma_ks = [&](const bf16* xb, auto k0c, auto k1c) {
#pragma unroll
    for (int ks = decltype(k0c)::value; ks < decltype(k1c)::value; ++ks) {
      const int tap = ks >> 1, c0 = (ks & 1) * 32;
      const int shift = (tap / 3) * 10 + tap % 3;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(xb + (base[mt] + shift) * C3F_XRS + c0 + q8);
        acc[mt][0] = mfma16x16x32(a, bw[0][ks], acc[mt][0]);
        acc[mt][1] = mfma16x16x32(a, bw[1][ks], acc[mt][1]);
      }
    }
  };
  // Step s: pool3 / fc1-partials epilogue of image s-2 and the first 4 k-steps of image s-1 (phase 1,
  // beside the producer's MFMA-light conv1), fc1 reduction of s-2 + k-steps 4-10 (phase 2), k-steps
  // 11-17 (phase 3, beside the producer's VALU-only pool2): the MFMA pipe has work in every phase.
  for (int s = 0; s < nsteps; ++s) {
    const int bm = b0 + (s - 1) * bstep, be = bm - bstep;
    const bool live_m = s >= 1 && bm < B, live_e = s >= 2 && be < B;
    const bf16* xb = X3 + ((s - 1) & 1) * FF_X3H;
    FF_ST(0);
    // ---------------- phase 1
    if (live_e) {
      float part[10];
#pragma unroll
      for (int n = 0; n < 10; ++n) part[n] = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int wc = wcol[mt], co = 32 * wave + 16 * t + r16;
          int g;
          const bf16 pb = (bf16)pool4(acc[mt][t], bv[t], g);
          const int64_t o = ((int64_t)be * 16 + wc) * 128 + co;
          a3[o] = pb;
          idx3[o] = (uint8_t)g;
          if (!fc) continue;
          const float pv = (float)pb;
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(fw + (wc * 128 + co) * 10);
#pragma unroll
          for (int h = 0; h < 5; ++h) {
            const uint32_t u = wp[h];
            part[2 * h] = fmaf(pv, __uint_as_float(u << 16), part[2 * h]);
            part[2 * h + 1] = fmaf(pv, __uint_as_float(u & 0xffff0000u), part[2 * h + 1]);
          }
        }
      if (fc) {
#pragma unroll
        for (int n = 0; n < 10; ++n) fred[n * 256 + tid] = part[n];
      }
    }
    if (live_m) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = zero_f32x4();
      mfma_ks(xb, std::integral_constant<int, 0>{}, std::integral_constant<int, FF_KA>{});
    }
    FF_ST(1);
    __syncthreads();  // [S1]
    FF_ST(2);
    // ---------------- phase 2
    if (live_e && fc) fc_reduce(be);
    if (live_m) mfma_ks(xb, std::integral_constant<int, FF_KA>{}, std::integral_constant<int, FF_KB>{});
    FF_ST(3);
    __syncthreads();  // [S2]
    FF_ST(4);
    // ---------------- phase 3: k-steps 11-17
    if (live_m) mfma_ks(xb, std::integral_constant<int, FF_KB>{}, std::integral_constant<int, 18>{});
    FF_ST(5);
    __syncthreads();  // [S3]
    FF_ST(6);
  }
}

template <bool U8>
__global__ __launch_bounds__(512, 1) void fused_fwd_kernel(const void* __restrict__ xin,
                                                          const bf16* __restrict__ packed,
                                                          const float* __restrict__ b1, const float* __restrict__ b2,
                                                          const float* __restrict__ b3, const float* __restrict__ bfc,
                                                          bf16* __restrict__ a1, uint8_t* __restrict__ idx1,
                                                          bf16* __restrict__ a2, uint8_t* __restrict__ idx2,
                                                          bf16* __restrict__ a3, uint8_t* __restrict__ idx3,
                                                          float* __restrict__ logits, int B, float mean,
                                                          float inv_std, float in_scale) {
  __shared__ __attribute__((aligned(16))) char ff_smem[FF_LDS + FF_ST_BYTES];
  const int b0 = blockIdx.x, bstep = gridDim.x;
  const int nimg = b0 < B ? (B - b0 + bstep - 1) / bstep : 0;
  const int nsteps = nimg + 2;  // the consumer's MFMAs trail by one step, its epilogue by two
  // wave-uniform role split (an SGPR condition: the two roles are separate code paths, not one
  // exec-masked sequence whose live ranges the register allocator would have to overlap)
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) < 4)
    ff_producer<U8>(ff_smem, xin, packed, b1, b2, a1, idx1, a2, idx2, (FF_ABLATE & 1) ? 0 : B, b0, bstep, nsteps,
                    mean, inv_std, in_scale);
  else
    ff_consumer(ff_smem, packed, b3, bfc, a3, idx3, logits, (FF_ABLATE & 2) ? 0 : B, b0, bstep, nsteps);
#ifdef RINGDP_FF_STAMPS
  __syncthreads();
  if (blockIdx.x == FF_ST_BLK && threadIdx.x == 0 && nsteps > FF_ST_S0 + 8) {
    const unsigned long long* st = reinterpret_cast<const unsigned long long*>(ff_smem + FF_LDS);
    for (int w = 0; w < 8; ++w)
      for (int k = 0; k < 8; ++k) {
        const unsigned long long* r = st + (w * 8 + k) * 8;
        const unsigned long long t0 = st[k * 8];  // wave 0's step start
        printf("FFST w%d s%d %lld %lld %lld %lld %lld %lld %lld\n", w, k, (long long)(r[0] - t0),
               (long long)(r[1] - t0), (long long)(r[2] - t0), (long long)(r[3] - t0), (long long)(r[4] - t0),
               (long long)(r[5] - t0), (long long)(r[6] - t0));
      }
  }
#endif
}

// largest batch whose fc1 runs inside the conv3 forward launch (RINGDP_CN_FC_FUSED_MAX overrides)
int fc_fused_max_batch() {
  static const int v = env_int("RINGDP_CN_FC_FUSED_MAX", 4096);
  return v;
}

// workgroups per CU of a persistent forward kernel; the RINGDP_CN_WPC_<kernel> knob overrides (A/B runs)
int wpc(const char* knob, int dflt) { return std::max(1, env_int(knob, dflt)); }

}  // namespace

// ================================================================== launchers
int64_t cn_packed_elems() { return PACK_TOTAL; }

void cn_pack_weights(const float* w1, const float* w2, const float* w3, const float* wfc, void* out,
                     hipStream_t s) {
  pack_weights_kernel<<<cdiv(PACK_TOTAL, 1024), 256, 0, s>>>(PackSrc{w1, w2, w3, wfc}, static_cast<bf16*>(out));
}

void cn_conv1_fwd(const void* x, bool u8, const void* packed, const float* b1, void* a1, uint8_t* idx1,
                  int B, float mean, float inv_std, float in_scale, hipStream_t s, const float* const* pack_w,
                  void* pack_out) {
  static const int per_cu = wpc("RINGDP_CN_WPC_C1F", 3);  // 51 KiB LDS: 3 workgroups per CU
  const int grid = clampi(B, 1, per_cu * num_cus());
  const bf16* pk = static_cast<const bf16*>(packed);
  bf16* a1b = static_cast<bf16*>(a1);
  const PackSrc ws = pack_w ? PackSrc{pack_w[0], pack_w[1], pack_w[2], pack_w[3]} : PackSrc{};
  const int g = pack_w ? grid + cdiv(PACK_TOTAL, 1024) : grid;  // + the pack workgroups (4 elements per thread)
  bf16* po = pack_w ? static_cast<bf16*>(pack_out) : nullptr;
  dispatch_bool(u8, [&](auto U8) {
    dispatch_bool(pack_w != nullptr, [&](auto PACK) {
      conv1_fwd_kernel<decltype(U8)::value, decltype(PACK)::value>
          <<<g, 256, 0, s>>>(x, pk, b1, a1b, idx1, B, mean, inv_std, in_scale, ws, po, grid);
    });
  });
}

void cn_sgd_flat_pack(float* p, const float* g, float* m, int64_t n, const SgdArgs& a, const int64_t* offsets,
                      void* packed, hipStream_t s) {
  if (n <= 0) return;
  PackDst d{static_cast<bf16*>(packed), {offsets[0], offsets[1], offsets[2], offsets[3]}};
  const int grid = std::max<int64_t>(1, std::min<int64_t>((n / 4 + 256) / 256, 2048));
  dispatch_bool(m && a.momentum != 0.f, [&](auto MOM) {
    cn_sgd_pack_kernel<decltype(MOM)::value><<<grid, 256, 0, s>>>(p, g, m, n, a, d);
  });
}

void cn_forward_fused(const void* x, bool u8, const float* const* w, const float* b1, const float* b2,
                      const float* b3, const float* bfc, void* packed, void* a1, uint8_t* idx1, void* a2,
                      uint8_t* idx2, void* a3, uint8_t* idx3, float* logits, int B, float mean, float inv_std,
                      float in_scale, hipStream_t s, bool do_pack) {
  static const int per_cu = wpc("RINGDP_CN_WPC_FF", 1);  // 121 KiB LDS: one 512-thread workgroup per CU
  const int grid = clampi(B, 1, per_cu * num_cus());
  bf16* pk = static_cast<bf16*>(packed);
  bf16 *a1b = static_cast<bf16*>(a1), *a2b = static_cast<bf16*>(a2), *a3b = static_cast<bf16*>(a3);
  // The weight pack is a launch of its own (do_pack false: the optimizer wrote these fragments when it last
  // updated the weights); packing inside the forward launch was measured and removed (docs/ARCHITECTURE.md).
  if (do_pack) pack_weights_kernel<<<cdiv(PACK_TOTAL, 1024), 256, 0, s>>>(PackSrc{w[0], w[1], w[2], w[3]}, pk);
  const bool fc_in = B <= fc_fused_max_batch();  // else fc1 as its own MFMA pass over a3
  float* lg = fc_in ? logits : nullptr;
  dispatch_bool(u8, [&](auto U8) {
    fused_fwd_kernel<decltype(U8)::value><<<grid, 512, 0, s>>>(x, pk, b1, b2, b3, bfc, a1b, idx1, a2b, idx2, a3b, idx3,
                                                               lg, B, mean, inv_std, in_scale);
  });
  if (!fc_in) fc1_fwd_kernel<<<cdiv(B, 16 * FC1_G), 256, 0, s>>>(a3b, pk, bfc, logits, B);
}

void cn_conv2_fwd(const void* a1, const void* packed, const float* b2, void* a2, uint8_t* idx2, int B,
                  hipStream_t s) {
  static const int per_cu = wpc("RINGDP_CN_WPC_C2F", 3);  // 49 KiB LDS, 157 VGPRs: 3 per CU (303 -> 260 us)
  const int grid = clampi(B, 1, per_cu * num_cus());
  conv2_fwd_kernel<<<grid, 256, 0, s>>>(static_cast<const bf16*>(a1), static_cast<const bf16*>(packed), b2,
                                        static_cast<bf16*>(a2), idx2, B);
}

void cn_conv3_fc_fwd(const void* a2, const void* packed, const float* b3, const float* bfc, float* logits,
                     void* a3, uint8_t* idx3, int B, hipStream_t s) {
  static const int per_cu = wpc("RINGDP_CN_WPC_C3F", 2);
  const int grid = clampi(B, 1, per_cu * num_cus());
  const bf16 *a2b = static_cast<const bf16*>(a2), *pk = static_cast<const bf16*>(packed);
  if (B <= fc_fused_max_batch()) {
    conv3_fwd_kernel<true><<<grid, 256, 0, s>>>(a2b, pk, b3, static_cast<bf16*>(a3), idx3, B, bfc, logits);
    return;
  }
  conv3_fwd_kernel<false><<<grid, 256, 0, s>>>(a2b, pk, b3, static_cast<bf16*>(a3), idx3, B, nullptr, nullptr);
  fc1_fwd_kernel<<<cdiv(B, 16 * FC1_G), 256, 0, s>>>(static_cast<const bf16*>(a3), pk, bfc, logits, B);
}

}  // namespace kern
}  // namespace ringdp
