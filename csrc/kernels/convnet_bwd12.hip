// bf16 ConvNet (design: convnet_fwd.hip), F2 and F1 backward: conv2 backward, conv1 wgrad, and the two fused as one
// launch (4-wave and 8-wave), their work splits and launchers.  One unit: apart, these kernels compile to other code.
#include "convnet_device.h"
#include "convnet_host.h"

namespace ringdp {
namespace kern {

namespace {

__device__ __forceinline__ bf16x8 ones_column_frag(int lane) {
  const bf16 one = (bf16)((lane & 15) == 0 ? 1.f : 0.f);
  return bf16x8{one, one, one, one, one, one, one, one};
}

// a * b per 16-bit half (v_pk_mul_lo_u16)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_mul_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, b));
}

// ================================================================== F2 backward
// conv2's ReLU and pool2 are undone by F3's backward, so dz2 is the conv output gradient directly:
//   dgrad: da1 = full-corr(dz2 image, flipped W2)  [13x13x32]
//   wgrad: dW2t[n = tap*32 + ci][co] = sum_pos dz2[pos][co] * a1[pos + tap][ci]; db2 via a ones tile
constexpr int C2_PW = 15, C2_PRS = 80, C2_ORS = 40, C2_DRS = 72;
// dgrad m-tile -> output position map (255 = padding row).  Each full tile holds two positions of every
// residue (y*15 + x) mod 8, one among lanes {0-3,12-15} and one among lanes {4-11}: with 160-B rows
// (C2_PRS 80) the 16 rows of every ds_read_b128 lane group then land on 16 distinct 16-B bank slots
// (modelled 11.3 -> 4.7 LDS cycles per A-fragment read, ideal 4; generator: tools/lds_bank_model.py).
__constant__ uint8_t c2d_tile_pos[176] = {0,1,2,3,8,9,10,11,12,19,20,13,4,5,6,7,14,15,16,17,22,23,24,25,32,39,34,27,18,33,26,21,28,29,30,31,36,37,38,45,52,53,48,41,46,47,40,35,42,43,44,59,50,51,58,65,66,67,62,55,60,61,54,49,56,57,72,73,64,71,78,79,80,81,76,69,74,75,68,63,70,85,86,87,84,91,92,93,94,95,90,83,88,89,82,77,98,99,100,101,104,105,106,107,108,109,110,111,102,103,96,97,112,113,114,115,118,119,120,121,122,137,130,125,116,123,124,117,126,127,128,129,132,133,134,135,150,151,144,139,136,143,138,131,140,141,142,149,146,147,148,163,164,165,158,153,156,157,152,145,154,155,162,168,160,161,255,255,255,255,255,167,255,255,166,159};
constexpr int C2D_P = C2_PW * C2_PW * C2_PRS * 2;  // 32400
constexpr int C2D_O = 169 * C2_ORS * 2;            // 13520 (x2: double-buffered output tile)
// wgrad dz2 tile: rows k in blocks of 8 (80-element rows, 704-element blocks): the 8 rows of a tr16
// 32-lane group (k, k+1, k+2, k+3, k+8, ..) then cover the 8 32-B bank slots once (modelled 4 -> 2)
__device__ __forceinline__ int c2_drow(int r) { return (r >> 3) * 704 + (r & 7) * 80; }
constexpr int C2W_D = 16 * 704 * 2;                // 22528
constexpr int C2W_X = 169 * C2_XRS * 2;            // 13520
constexpr int C2B_LDS = (C2D_P + 2 * C2D_O) > (C2W_D + C2W_X) ? (C2D_P + 2 * C2D_O) : (C2W_D + C2W_X);
constexpr int C2_WSLAB = 288 * 64 + 64;

__device__ __forceinline__ void conv2_dgrad_role(char* smem, const bf16* __restrict__ dz2, const bf16* __restrict__ packed,
                                 bf16* __restrict__ da1, int B, int block, int nblocks) {
  bf16* P = reinterpret_cast<bf16*>(smem);
  bf16* O = reinterpret_cast<bf16*>(smem + C2D_P);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = wave & 1, mg = wave >> 1;  // n-tile (16 input channels), m-tiles mg, mg+4, mg+8
  const int r16 = lane & 15, q8 = (lane >> 4) * 8;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P2D_OFF);
  bf16x8 bw[18];
#pragma unroll
  for (int ks = 0; ks < 18; ++ks) bw[ks] = pk[(nt * 18 + ks) * 64 + lane];
  int base[3];  // padding rows read a valid address; their outputs are dropped
  int opos[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int mt = min(mg + 4 * k, 10);
    const int mm = c2d_tile_pos[mt * 16 + r16] == 255 ? 0 : c2d_tile_pos[mt * 16 + r16];
    base[k] = (mm / 13) * C2_PW + mm % 13;
#pragma unroll
    for (int i = 0; i < 4; ++i) opos[k][i] = c2d_tile_pos[mt * 16 + (lane >> 4) * 4 + i];
  }
  for (int c = tid; c < C2D_P / 16; c += 512) reinterpret_cast<bf16x8*>(P)[c] = zero_bf16x8();
  auto copy_out = [&](int bb, const bf16* src) {
    bf16x8* dst = reinterpret_cast<bf16x8*>(da1 + (int64_t)bb * 169 * 32);
    for (int c = tid; c < 676; c += 512) dst[c] = *reinterpret_cast<const bf16x8*>(src + (c >> 2) * C2_ORS + (c & 3) * 8);
  };
  bf16x8 pz[2];
  auto load = [&](int bb) {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(dz2 + (int64_t)bb * 121 * 64);
    pz[0] = src[tid];
    if (tid + 512 < 968) pz[1] = src[tid + 512];
  };
  // m-tiles mg, mg+4, mg+8 < 11: 3 for waves with mg < 3, 2 for mg == 3 (compile-time trip counts)
  auto mfma_phase = [&](auto nk_c, bf16* Oc) {
    constexpr int NK = decltype(nk_c)::value;
    f32x4 acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = zero_f32x4();
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) {
      const int tapp = ks >> 1, c0 = (ks & 1) * 32;
      const int shift = (tapp / 3) * C2_PW + tapp % 3;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        acc[k] = mfma16x16x32(*reinterpret_cast<const bf16x8*>(P + (base[k] + shift) * C2_PRS + c0 + q8), bw[ks],
                              acc[k]);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = opos[k][i];
        if (m < 169) Oc[m * C2_ORS + nt * 16 + r16] = (bf16)acc[k][i];
      }
    }
  };
  int b = block, prev = -1, cur = 0;
  if (b < B) load(b);
  for (; b < B; b += nblocks) {
    __syncthreads();
    if (prev >= 0) copy_out(prev, O + (cur ^ 1) * 169 * C2_ORS);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = tid + 512 * k;
      if (c < 968) {
        const int pos = c >> 3, cc = (c & 7) * 8;
        *reinterpret_cast<bf16x8*>(P + ((pos / 11 + 2) * C2_PW + pos % 11 + 2) * C2_PRS + cc) = pz[k];
      }
    }
    const int nb = b + nblocks;
    if (nb < B) load(nb);
    __syncthreads();
    bf16* Oc = O + cur * 169 * C2_ORS;
    if (mg < 3)
      mfma_phase(std::integral_constant<int, 3>{}, Oc);
    else
      mfma_phase(std::integral_constant<int, 2>{}, Oc);
    prev = b;
    cur ^= 1;
  }
  __syncthreads();
  if (prev >= 0) copy_out(prev, O + (cur ^ 1) * 169 * C2_ORS);
}

__device__ __forceinline__ void conv2_wgrad_role(char* smem, const bf16* __restrict__ a1, const bf16* __restrict__ dz2,
                                 float* __restrict__ slabs, int B, int nslices, int slice) {
  bf16* D = reinterpret_cast<bf16*>(smem);
  bf16* X = reinterpret_cast<bf16*>(smem + C2W_D);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // m-tile wm (co 16wm..), n-tiles 9wn..9wn+8
  const int g16 = lane & 15, grp = lane >> 4, q = g16 >> 2, p = g16 & 3;
  const bf16x8 onesf = ones_column_frag(lane);
  f32x4 acc[9], accb = zero_f32x4();
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = zero_f32x4();
  for (int c = tid; c < C2W_D / 16; c += 512) reinterpret_cast<bf16x8*>(D)[c] = zero_bf16x8();  // rows >= 121 stay 0
  const int per = cdiv(B, nslices);
  const int b_lo = slice * per, b_hi = min(B, b_lo + per);
  bf16x8 pz[2], pa[2];
  auto load = [&](int bb) {
    const bf16x8* zs = reinterpret_cast<const bf16x8*>(dz2 + (int64_t)bb * 121 * 64);
    const bf16x8* as = reinterpret_cast<const bf16x8*>(a1 + (int64_t)bb * 169 * 32);
    pz[0] = zs[tid];
    if (tid + 512 < 968) pz[1] = zs[tid + 512];
    pa[0] = as[tid];
    if (tid + 512 < 676) pa[1] = as[tid + 512];
  };
  if (b_lo < b_hi) load(b_lo);
  for (int b = b_lo; b < b_hi; ++b) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = tid + 512 * k;
      if (c < 968) *reinterpret_cast<bf16x8*>(D + c2_drow(c >> 3) + (c & 7) * 8) = pz[k];
      if (c < 676) *reinterpret_cast<bf16x8*>(X + (c >> 2) * C2_XRS + (c & 3) * 8) = pa[k];
    }
    if (b + 1 < b_hi) load(b + 1);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kb = ks * 32 + grp * 8;
      const int m0 = wm * 16;
      const bf16x4 alo = lds_read_tr16(D + c2_drow(kb + q) + m0 + 4 * p);
      const bf16x4 ahi = lds_read_tr16(D + c2_drow(kb + 4 + q) + m0 + 4 * p);
      const bf16x8 af = bf16x8{alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
      const int k0 = min(kb + q, 120), k1 = min(kb + 4 + q, 120);  // rows >= 121 of D are zero
      const int x0 = (k0 / 11) * 13 + k0 % 11, x1 = (k1 / 11) * 13 + k1 % 11;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int n0 = (9 * wn + j) * 16;  // n = tap*32 + ci
        const int tap = n0 >> 5, c0 = n0 & 31;
        const int shift = (tap / 3) * 13 + tap % 3;
        const bf16x4 lo = lds_read_tr16(X + (x0 + shift) * C2_XRS + c0 + 4 * p);
        const bf16x4 hi = lds_read_tr16(X + (x1 + shift) * C2_XRS + c0 + 4 * p);
        const bf16x8 bf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[j] = mfma16x16x32(af, bf, acc[j]);
      }
      if (wn == 0) accb = mfma16x16x32(af, onesf, accb);
    }
  }
  float* slab = slabs + (int64_t)slice * C2_WSLAB;
  const int co = wm * 16 + grp * 4;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int n = (9 * wn + j) * 16 + g16;
    *reinterpret_cast<f32x4*>(slab + (int64_t)n * 64 + co) = acc[j];
  }
  if (wn == 0 && g16 == 0) *reinterpret_cast<f32x4*>(slab + 288 * 64 + co) = accb;
}

__global__ __launch_bounds__(512) void conv2_bwd_kernel(const bf16* __restrict__ a1,
                                                        const bf16* __restrict__ dz2,
                                                        const bf16* __restrict__ packed,
                                                        bf16* __restrict__ da1, int B,
                                                        float* __restrict__ slabs, int nslices,
                                                        int n_dgrad) {
  __shared__ __attribute__((aligned(16))) char smem[C2B_LDS];
  if ((int)blockIdx.x < n_dgrad)
    conv2_dgrad_role(smem, dz2, packed, da1, B, blockIdx.x, n_dgrad);
  else
    conv2_wgrad_role(smem, a1, dz2, slabs, B, nslices, blockIdx.x - n_dgrad);
}

// ================================================================== F1 backward (conv1 wgrad)
// dW1[co][t] = sum_{b, oh, ow} dC[b][oh][ow][co] * xpad[b][oh + kh][ow + kw]  as a TN GEMM with
// K = spatial positions in rows of 32 (k = oh*32 + ow, ow >= 26 zero): the X operand for tap
// (kh, kw) and 8 consecutive ow is one aligned ds_read_b128 of shifted copy kw.  dC = unpool(da1) *
// relu-mask is never materialised: the A fragment of lane (co, 8 positions ow..ow+7 of row oh) covers 4
// pool windows px..px+3 of window row oh/2, so it is built in registers from ONE ds_read_b64_tr_b16 of
// the compact da1 image (4 windows x 16 channels) and ONE 8-byte read of the code rows: element
// (window k, dx) = da1 if bit (oh&1)*2 + dx of the window's one-hot code is set, else 0.  Tap column t = 25 of the padded N is a ones
// column -> db1 for free.  The 4 waves split K (rows oh = wave mod 4) and cover all 2x2 output tiles,
// so every A and B fragment feeds 2 MFMAs; da1 and the codes of the next image land by LDS-DMA while
// the current one computes.
constexpr int C1_WSLAB = 32 * 25 + 32;
constexpr int C1W_RS = 48, C1W_CS = 1520;          // padded copies: B-operand reads 16 -> 6 LDS cycles
constexpr int C1W_XS = 0;                          // 5 shifted copies of the input image (bf16)
constexpr int C1W_D = 5 * C1W_CS * 2;              // 15200: da1 image [169 (+3 zero) windows][32] bf16, x2
constexpr int C1W_DSZ = 172 * 32 * 2;              // 11008
constexpr int C1W_C = C1W_D + 2 * C1W_DSZ;         // 37216: code rows [13][16][16][2] bytes, x2
constexpr int C1W_LDS = C1W_C + 2 * C1I_IMG;       // 43872 -> 3 workgroups per CU

template <bool U8>
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const void* __restrict__ xin,
                                                          const bf16* __restrict__ da1,
                                                          const uint8_t* __restrict__ idx1, int B,
                                                          float mean, float inv_std, float in_scale,
                                                          float* __restrict__ slabs, int nslices) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[C1W_LDS];  // one array: keeps the DMA in flight
  bf16* xs = reinterpret_cast<bf16*>(lds + C1W_XS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4, q = i16 >> 2, p = i16 & 3;
  // B operand (x) per n-tile: lane column t = 16 nt + i16; t = 25 is the ones column, t > 25 zero
  const int t1 = 16 + i16;
  const int xoff0 = (i16 % 5) * C1W_CS + (i16 / 5) * C1W_RS + 8 * g;
  const int xoff1 = t1 < 25 ? (t1 % 5) * C1W_CS + (t1 / 5) * C1W_RS + 8 * g : 0;
  const uint32_t b1fill = t1 == 25 ? 0x3f803f80u : 0u;  // bf16 1.0 pairs
  for (int i = tid; i < C1W_C / 16; i += 256) reinterpret_cast<uint4*>(lds)[i] = make_uint4(0, 0, 0, 0);
  const int per = cdiv(B, nslices);
  const int b_lo = min(B, blockIdx.x * per), b_hi = min(B, b_lo + per);
  auto dma = [&](int bb, int k) {
    const bf16* src = da1 + (int64_t)bb * C1A_IMG;
    uint8_t* dd = lds + C1W_D + k * C1W_DSZ;
    for (int i = wave; i < 11; i += 4) {
      const int c = i * 64 + lane;
      if (c < C1A_IMG / 8) glds16_async(src + c * 8, dd + i * 1024);
    }
    const uint8_t* cs = idx1 + (int64_t)bb * C1I_IMG;
    uint8_t* cd = lds + C1W_C + k * C1I_IMG;
    for (int i = wave; i < 7; i += 4) {
      const int c = i * 64 + lane;
      if (c < C1I_IMG / 16) glds16_async(cs + c * 16, cd + i * 1024);
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m) acc[m][0] = acc[m][1] = zero_f32x4();
  uint32_t xu = 0;
  float4 xf = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();  // zero fill done before any DMA / copy write lands
  if (b_lo < b_hi) {
    c1_load<U8>(xin, b_lo, tid, xu, xf);
    dma(b_lo, 0);
    c1_store<U8, 5, C1W_RS, C1W_CS>(xs, tid, xu, xf, mean, inv_std, in_scale);
  }
  int cur = 0;
  for (int b = b_lo; b < b_hi; ++b) {
    c_dma_wait();
    __syncthreads();  // copies of image b written, its da1 / codes landed
    if (b + 1 < b_hi) {
      c1_load<U8>(xin, b + 1, tid, xu, xf);
      dma(b + 1, cur ^ 1);
    }
    const bf16* D = reinterpret_cast<const bf16*>(lds + C1W_D + cur * C1W_DSZ);
    const uint8_t* CB = lds + C1W_C + cur * C1I_IMG;
    const int dy = wave & 1;  // ks = wave (mod 4): every k-step of a wave is the same window row half
    for (int ks = wave; ks < 26; ks += 4) {
      const int py = ks >> 1;
      bf16x8 A[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        // (bit-cast the whole vector: __builtin_bit_cast of a single vector element miscompiles to element 0)
        const uint2 d = __builtin_bit_cast(uint2, lds_read_tr16(D + (py * 13 + 4 * g + q) * 32 + m * 16 + 4 * p));
        const int co = m * 16 + i16;
        const uint32_t cu = *reinterpret_cast<const uint32_t*>(CB + py * 256 + (co >> 1) * 16 + 4 * g);
        const int csh = 4 * (co & 1) + 2 * dy;
        uint32_t pr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t dv = k & 1 ? (k < 2 ? d.x : d.y) >> 16 : (k < 2 ? d.x : d.y) & 0xffffu;
          // the two one-hot bits of window row dy: 1 -> dx = 0, 2 -> dx = 1, 0 -> no gradient
          const uint32_t sel = __builtin_amdgcn_ubfe(cu, 8 * k + csh, 2);
          pr[k] = dv * ((sel * 0x8001u) & 0x10001u);  // dv, dv << 16 or 0
        }
        A[m] = __builtin_bit_cast(bf16x8, make_uint4(pr[0], pr[1], pr[2], pr[3]));
      }
      const bf16x8 B0 = *reinterpret_cast<const bf16x8*>(xs + xoff0 + ks * C1W_RS);
      bf16x8 B1 = *reinterpret_cast<const bf16x8*>(xs + xoff1 + ks * C1W_RS);
      if (t1 >= 25) B1 = __builtin_bit_cast(bf16x8, make_uint4(b1fill, b1fill, b1fill, b1fill));
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        acc[m][0] = mfma16x16x32(A[m], B0, acc[m][0]);
        acc[m][1] = mfma16x16x32(A[m], B1, acc[m][1]);
      }
    }
    if (b + 1 < b_hi) {
      __syncthreads();  // every wave is done reading the copies of image b
      c1_store<U8, 5, C1W_RS, C1W_CS>(xs, tid, xu, xf, mean, inv_std, in_scale);
    }
    cur ^= 1;
  }
  // combine the 4 K-groups in a fixed order (deterministic) and write this workgroup's slab
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);  // [wave][tile][lane][4]: 16 KiB
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      *reinterpret_cast<f32x4*>(red + ((wave * 4 + m * 2 + n) * 64 + lane) * 4) = acc[m][n];
  __syncthreads();
  const int tile = tid >> 6;
  f32x4 sum = *reinterpret_cast<const f32x4*>(red + (tile * 64 + lane) * 4);
#pragma unroll
  for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<const f32x4*>(red + ((w * 4 + tile) * 64 + lane) * 4);
  float* slab = slabs + (int64_t)blockIdx.x * C1_WSLAB;
  const int tap = (tile & 1) * 16 + i16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = (tile >> 1) * 16 + g * 4 + r;
    if (tap < 25) slab[co * 25 + tap] = sum[r];
    if (tap == 25) slab[800 + co] = sum[r];
  }
}

// ================================================================== F2 backward + F1 wgrad, fused
// The conv2 data gradient of an image (da1, 13x13x32) has exactly one consumer: conv1's weight gradient.
// The dgrad workgroups therefore keep da1 in LDS and run conv1 wgrad on it right away (the input image
// and its pool1 codes arrive by register load / LDS-DMA while conv2 dgrad computes): da1 never goes to
// HBM (2 x 354 MB per step at B=32768), and conv1 wgrad + its reduction are no longer launches of their
// own.  Each dgrad workgroup leaves one conv1 slab (C1_WSLAB), reduced with conv2's slabs in one launch.
// conv1 part: the 8 waves split K (rows oh = wave mod 8; dy = wave & 1 stays fixed per wave) and cover
// all 2x2 output tiles, as conv1_wgrad_kernel does with 4 waves.
constexpr int C12_O = 172 * C2_ORS * 2;             // 13760: da1 [169 + 3 zero windows][32 (+8 pad)] bf16
constexpr int C12_XS = 5 * C1W_CS * 2;              // 15200: 5 shifted copies of the input image
// P | O[2] | xs[2] | codes[2]: image i uses buffer set i & 1, so conv1 wgrad of image i-1 runs interleaved
// with conv2 dgrad of image i (2 waves per SIMD: the MFMA stream of one hides the LDS/VALU of the other)
constexpr int C12_OFF_O = C2D_P, C12_OFF_X = C12_OFF_O + 2 * C12_O, C12_OFF_C = C12_OFF_X + 2 * C12_XS;
constexpr int C12_LDS = C12_OFF_C + 2 * C1I_IMG;    // 96976
constexpr int C12B_LDS = C12_LDS > (C2W_D + C2W_X) ? C12_LDS : (C2W_D + C2W_X);
static_assert(C2D_P % 16 == 0 && C12_O % 16 == 0 && C12_XS % 16 == 0, "16-B aligned LDS buffers");
static_assert(8 * 4 * 64 * 4 * 4 <= C12_OFF_X, "conv1 cross-wave reduction fits in P + O");

template <bool U8>
__device__ __forceinline__ void conv12_dgrad_role(char* smem, const void* __restrict__ xin, const uint8_t* __restrict__ idx1,
                                  const bf16* __restrict__ dz2, const bf16* __restrict__ packed, int B, int block,
                                  int nblocks, float mean, float inv_std, float in_scale,
                                  float* __restrict__ slabs1) {
  bf16* P = reinterpret_cast<bf16*>(smem);
  auto Obuf = [&](int k) { return reinterpret_cast<bf16*>(smem + C12_OFF_O + k * C12_O); };
  auto Xbuf = [&](int k) { return reinterpret_cast<bf16*>(smem + C12_OFF_X + k * C12_XS); };
  auto Cbuf = [&](int k) { return reinterpret_cast<uint8_t*>(smem + C12_OFF_C + k * C1I_IMG); };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- conv2 dgrad operands (as conv2_dgrad_role)
  const int nt = wave & 1, mg = wave >> 1;
  const int r16 = lane & 15, q8 = (lane >> 4) * 8;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P2D_OFF);
  bf16x8 bw[18];
#pragma unroll
  for (int ks = 0; ks < 18; ++ks) bw[ks] = pk[(nt * 18 + ks) * 64 + lane];
  int base[3];
  int opos[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int mt = min(mg + 4 * k, 10);
    const int mm = c2d_tile_pos[mt * 16 + r16] == 255 ? 0 : c2d_tile_pos[mt * 16 + r16];
    base[k] = (mm / 13) * C2_PW + mm % 13;
#pragma unroll
    for (int i = 0; i < 4; ++i) opos[k][i] = c2d_tile_pos[mt * 16 + (lane >> 4) * 4 + i];
  }
  // ---- conv1 wgrad operands (as conv1_wgrad_kernel)
  const int i16 = lane & 15, g = lane >> 4, q = i16 >> 2, p = i16 & 3;
  const int t1 = 16 + i16;
  const int xoff0 = (i16 % 5) * C1W_CS + (i16 / 5) * C1W_RS + 8 * g;
  const int xoff1 = t1 < 25 ? (t1 % 5) * C1W_CS + (t1 / 5) * C1W_RS + 8 * g : 0;
  const uint32_t b1fill = t1 == 25 ? 0x3f803f80u : 0u;
  const int dy = wave & 1;
  f32x4 acc1[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m) acc1[m][0] = acc1[m][1] = zero_f32x4();
  // zero P (its ring stays zero), both O (windows 169..171 stay zero) and both copy sets (ring stays zero)
  for (int c = tid; c < C12_OFF_C / 16; c += 512) reinterpret_cast<bf16x8*>(smem)[c] = zero_bf16x8();
  // next image, staged in registers: dz2 rows, input pixels, pool1 code rows
  bf16x8 pz[2];
  uint4 pc = make_uint4(0, 0, 0, 0);
  uint32_t xu = 0;
  float4 xf = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load = [&](int bb) {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(dz2 + (int64_t)bb * 121 * 64);
    pz[0] = src[tid];
    if (tid + 512 < 968) pz[1] = src[tid + 512];
    if (tid < C1I_IMG / 16) pc = reinterpret_cast<const uint4*>(idx1 + (int64_t)bb * C1I_IMG)[tid];
    c1_load<U8>(xin, bb, tid, xu, xf);
  };
  auto stage = [&](int k) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + 512 * j;
      if (c < 968) {
        const int pos = c >> 3, cc = (c & 7) * 8;
        *reinterpret_cast<bf16x8*>(P + ((pos / 11 + 2) * C2_PW + pos % 11 + 2) * C2_PRS + cc) = pz[j];
      }
    }
    if (tid < C1I_IMG / 16) reinterpret_cast<uint4*>(Cbuf(k))[tid] = pc;
    c1_store<U8, 5, C1W_RS, C1W_CS>(Xbuf(k), tid, xu, xf, mean, inv_std, in_scale);
  };
  // conv1 wgrad k-step j (rows oh = wave + 8j; j = 3 only for waves 0, 1) of the image in buffer set k
  auto c1_step = [&](int j, int k) {
    const int ks0 = wave + 8 * j;
    const bool ok = ks0 < 26;  // wave-uniform
    const int ks = ok ? ks0 : 0;
    const int py = ks >> 1;
    const bf16* O = Obuf(k);
    const bf16* xs = Xbuf(k);
    const uint8_t* CB = Cbuf(k);
    bf16x8 A[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint2 d = __builtin_bit_cast(uint2, lds_read_tr16(O + (py * 13 + 4 * g + q) * C2_ORS + m * 16 + 4 * p));
      const int co = m * 16 + i16;
      const uint32_t cu = *reinterpret_cast<const uint32_t*>(CB + py * 256 + (co >> 1) * 16 + 4 * g);
      const int csh = 4 * (co & 1) + 2 * dy;
      uint32_t pr[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t dv = e & 1 ? (e < 2 ? d.x : d.y) >> 16 : (e < 2 ? d.x : d.y) & 0xffffu;
        const uint32_t sel = __builtin_amdgcn_ubfe(cu, 8 * e + csh, 2);
        pr[e] = ok ? dv * ((sel * 0x8001u) & 0x10001u) : 0u;
      }
      A[m] = __builtin_bit_cast(bf16x8, make_uint4(pr[0], pr[1], pr[2], pr[3]));
    }
    const bf16x8 B0 = *reinterpret_cast<const bf16x8*>(xs + xoff0 + ks * C1W_RS);
    bf16x8 B1 = *reinterpret_cast<const bf16x8*>(xs + xoff1 + ks * C1W_RS);
    if (t1 >= 25) B1 = __builtin_bit_cast(bf16x8, make_uint4(b1fill, b1fill, b1fill, b1fill));
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      acc1[m][0] = mfma16x16x32(A[m], B0, acc1[m][0]);
      acc1[m][1] = mfma16x16x32(A[m], B1, acc1[m][1]);
    }
  };
  // conv2 dgrad of the image staged in P -> O[k]; with C1 set, conv1 k-steps of buffer set k ^ 1 are
  // issued between its k-steps (after dgrad k-steps 3, 7, 11, 15)
  auto phase = [&](auto nk_c, auto c1_c, int k) {
    constexpr int NK = decltype(nk_c)::value;
    constexpr bool C1 = decltype(c1_c)::value;
    f32x4 acc[NK];
#pragma unroll
    for (int m = 0; m < NK; ++m) acc[m] = zero_f32x4();
#pragma unroll
    for (int ks = 0; ks < 18; ++ks) {
      const int tapp = ks >> 1, c0 = (ks & 1) * 32;
      const int shift = (tapp / 3) * C2_PW + tapp % 3;
#pragma unroll
      for (int m = 0; m < NK; ++m)
        acc[m] = mfma16x16x32(*reinterpret_cast<const bf16x8*>(P + (base[m] + shift) * C2_PRS + c0 + q8), bw[ks],
                              acc[m]);
      if (C1 && (ks & 3) == 3 && ks < 16) c1_step(ks >> 2, k ^ 1);
    }
    bf16* O = Obuf(k);
#pragma unroll
    for (int m = 0; m < NK; ++m) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pos = opos[m][i];
        if (pos < 169) O[pos * C2_ORS + nt * 16 + r16] = (bf16)acc[m][i];
      }
    }
  };
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using T = std::true_type;
  using Fa = std::false_type;
  __syncthreads();  // zero fill done
  int b = block, k = 0;
  if (b < B) load(b);
  for (int i = 0; b < B; ++i, b += nblocks, k ^= 1) {
    __syncthreads();  // readers of P and of buffer set k (image i-2) are done
    stage(k);
    const int nb = b + nblocks;
    if (nb < B) load(nb);
    __syncthreads();  // image i staged; O[k ^ 1] (image i-1's da1) complete
    if (i == 0) {
      if (mg < 3) phase(I3{}, Fa{}, k);
      else phase(I2{}, Fa{}, k);
    } else {
      if (mg < 3) phase(I3{}, T{}, k);
      else phase(I2{}, T{}, k);
    }
  }
  __syncthreads();
  if (b != block) {  // at least one image: conv1 wgrad of the last one (buffer set k ^ 1)
#pragma unroll
    for (int j = 0; j < 4; ++j) c1_step(j, k ^ 1);
  }
  // combine the 8 K-groups in a fixed order (deterministic) and write this workgroup's conv1 slab
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [wave][tile][lane][4]: 32 KiB over P + O
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
      *reinterpret_cast<f32x4*>(red + ((wave * 4 + m * 2 + n) * 64 + lane) * 4) = acc1[m][n];
  __syncthreads();
  if (tid >= 256) return;
  const int tile = tid >> 6;
  f32x4 sum = *reinterpret_cast<const f32x4*>(red + (tile * 64 + lane) * 4);
#pragma unroll
  for (int w = 1; w < 8; ++w) sum += *reinterpret_cast<const f32x4*>(red + ((w * 4 + tile) * 64 + lane) * 4);
  float* slab = slabs1 + (int64_t)block * C1_WSLAB;
  const int tap = (tile & 1) * 16 + i16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = (tile >> 1) * 16 + g * 4 + r;
    if (tap < 25) slab[co * 25 + tap] = sum[r];
    if (tap == 25) slab[800 + co] = sum[r];
  }
}

template <bool U8>
__global__ __launch_bounds__(512) void conv12_bwd_kernel(const void* __restrict__ xin,
                                                         const uint8_t* __restrict__ idx1,
                                                         const bf16* __restrict__ a1,
                                                         const bf16* __restrict__ dz2,
                                                         const bf16* __restrict__ packed, int B,
                                                         float mean, float inv_std, float in_scale,
                                                         float* __restrict__ slabs2, int nslices,
                                                         float* __restrict__ slabs1, int n_dgrad) {
  __shared__ __attribute__((aligned(16))) char smem[C12B_LDS];
  if ((int)blockIdx.x < n_dgrad)
    conv12_dgrad_role<U8>(smem, xin, idx1, dz2, packed, B, blockIdx.x, n_dgrad, mean, inv_std, in_scale, slabs1);
  else
    conv2_wgrad_role(smem, a1, dz2, slabs2, B, nslices, blockIdx.x - n_dgrad);
}

// ---- conv2 backward + conv1 wgrad with wave-specialised / pipelined 8-wave workgroups (the conv3 bwd8
// scheme; batches above fc_in_c3_max_batch).  One 512-thread workgroup per CU:
//   dgrad: waves 0-3 run conv2's data gradient of image s (both 16-channel n-tiles per wave, so every
//     A-fragment read feeds 2 MFMAs: half the LDS reads of conv12_dgrad_role) into da1 O[s&1]; beside them
//     waves 4-7 stage image s+1 (dz2 -> P, input copies, pool1 codes; registers loaded two steps ahead).
//     conv1's weight gradient of image s-1 (from O[(s-1)&1]) runs on the sparse MFMA, 13 steps of one window
//     row each: 12 on waves 4-7 and 1 on wave 3 after its conv2 phase, none on waves 0-2, which end their
//     conv2 phase when the helper waves end their steps (profiles/r13/c1_wgrad_sparse/README.md).  One barrier
//     per image.  The input copies and codes of image s-1 are still read while image s+1 is staged: three of
//     those.
//   wgrad: conv2's weight gradient, 8 waves each 2 co tiles x 4-5 n-tiles (14 tr16 reads per 10 MFMAs per
//     k-step instead of 20 per 9), image i+2 staged from registers while image i's MFMAs run (waves 0-3
//     before their k-steps, waves 4-7 after theirs).
constexpr int C12V_DG = 2 * (C2D_P + C12_O) + 3 * (C12_XS + C1I_IMG);  // 155104
constexpr int C12V_WG = 3 * (C2W_D + C2W_X);                           // 108144
constexpr int C12V_LDS = C12V_DG > C12V_WG ? C12V_DG : C12V_WG;
static_assert(C12V_LDS <= 160 * 1024 && C1I_IMG % 16 == 0, "conv12 backward (8-wave) LDS");

// RINGDP_C12_ABLATE (diagnostic builds only, tools/build_variant.py; timing only, wrong results): bit 0 skips
// conv1's weight gradient in the 8-wave conv12 backward, bit 1 the conv2 dgrad MFMAs, bit 2 the conv2 weight
// gradient.  A compile-time constant, 0 in every normal build: nothing reads the environment for it.
// Unlike the other two ablation macros it still reaches its kernel as the run-time argument `ablate` (the
// launcher passes this constant, nothing else), with the parent's uses of that argument unchanged, bit 3 (the
// VALU / DMA half at issue priority 1) included: with the argument folded away conv12_bwd8_kernel measured
// 2.3 % slower (917.6 vs 896.8 us, profiles/r07/variant_removal/README.md), and that schedule is not chased here.
#ifndef RINGDP_C12_ABLATE
#define RINGDP_C12_ABLATE 0
#endif
constexpr int C12_ABLATE = RINGDP_C12_ABLATE;

// RINGDP_C12_STAMPS (diagnostic builds only, tools/build_variant.py): lane 0 of every wave records s_memtime at
// up to 4 phase points of steps [C12_ST_S0, C12_ST_S0 + 8) into LDS past C12V_LDS; dgrad workgroup C12_ST_BLK
// ("C12ST d") and wgrad slice C12_ST_BLK ("C12ST w") print them at the end, relative to their wave 0's first
// stamp.  dgrad MFMA waves: 0 step start (just past the previous barrier), 1 last MFMA issued, 2 da1 stored, 3
// conv1 share done; dgrad helper waves: 0 stage done, 1 loads issued, 2 conv1 share done, 3 past the barrier;
// wgrad waves: 0 stage done, 1 last k-step done, 2 past the barrier.
#ifdef RINGDP_C12_STAMPS
constexpr int C12_ST_S0 = 100, C12_ST_BLK = 5, C12_ST_BYTES = 8 * 8 * 4 * 8;
#define C12_ST(s, k) CN_STAMP(C12V_LDS, C12_ST_S0, 4, s, k)
#else
constexpr int C12_ST_BYTES = 0;
#define C12_ST(s, k) do {} while (0)
#endif

template <bool U8>
__device__ __forceinline__ void conv12_dgrad8_role(char* smem, const void* __restrict__ xin,
                                                   const uint8_t* __restrict__ idx1, const bf16* __restrict__ dz2,
                                                   const bf16* __restrict__ packed, int B, int block, int nblocks,
                                                   float mean, float inv_std, float in_scale,
                                                   float* __restrict__ slabs1, int ablate) {
  auto Pb = [&](int k) { return reinterpret_cast<bf16*>(smem + k * C2D_P); };
  auto Ob = [&](int k) { return reinterpret_cast<bf16*>(smem + 2 * C2D_P + k * C12_O); };
  auto Xb = [&](int k) { return reinterpret_cast<bf16*>(smem + 2 * (C2D_P + C12_O) + k * C12_XS); };
  auto Cb = [&](int k) { return reinterpret_cast<uint8_t*>(smem + 2 * (C2D_P + C12_O) + 3 * C12_XS + k * C1I_IMG); };
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = block < B ? (B - block + nblocks - 1) / nblocks : 0;
  // zero rings of both dz2 images, the zero windows 169..171 of both da1 images, the rings of the copies
  for (int c = tid; c < (2 * (C2D_P + C12_O) + 3 * C12_XS) / 16; c += 512)
    reinterpret_cast<bf16x8*>(smem)[c] = zero_bf16x8();
  __syncthreads();
  if ((ablate & 8) && wave >= 4) __builtin_amdgcn_s_setprio(1);
  // ---- conv1's weight gradient of one image on the sparse MFMA.  pool1 is 2x2 / stride 2, so of the four dC
  // positions of a window at most one is live, and an aligned group of four dense columns (k = oh * 32 + ow) is two
  // neighbouring windows in one row half: the 2-of-4 pattern of v_smfmac_f32_16x16x64_bf16 (layout: smfmac16x16x64).
  // One sparse step covers window row py, i.e. the dense k-steps 2py (dy = 0) and 2py + 1 (dy = 1): 13 steps of
  // 4 MFMAs per image.  Lane (i16 = channel, G = lane >> 4) holds row half dy = G >> 1, windows 8 (G & 1) .. + 7:
  //   values: two ds_read_b64_tr_b16 of the da1 image deliver the eight windows in slot order, two per dword.  da1
  //     is not masked, so a slot keeps its value only if the window's one-hot code has a bit in row dy (a
  //     ReLU-dead window has none, windows 13..15 have zero code bytes): one 0 / 1 factor per 16-bit half, so a
  //     dead slot is +0.0 whatever the da1 bits were.
  //   index: slot e stands for column 2 (e & 1) + dx of its group, dx = the upper of the code's two row-dy bits.
  //   B: the dense fragments of k-steps 2py and 2py + 1 back to back (tap column 25 all ones -> db1).
  // The MFMA waves 0-2 end their conv2 phase last and take none; wave 3 (2 m-tiles) takes C12_S3 steps and the
  // helper waves share the first 13 - C12_S3 (vw, vw + 4, ..).  Every wave sums its own steps over all images
  // (none: zeros); the 8 partial sums are combined at the end in a fixed order.  All LDS addresses are 32-bit
  // byte offsets from smem: a per-lane part formed once and scalar per-image and per-step parts.  (Formed from
  // pointers they compiled to 64-bit multiply-adds whose undefined high halves shared registers with the global
  // loads in flight, and the loop waited for those.)
  constexpr int C12_S3 = 1, C12_SH = 13 - C12_S3;
  static_assert(C12_SH >= 4 && C12_S3 >= 0, "conv1 step partition");
  const int k0 = wave < 4 ? C12_SH : wave - 4, kst = wave < 4 ? 1 : 4;
  const int kcnt = wave < 3 ? 0 : wave == 3 ? C12_S3 : (C12_SH - (wave - 4) + 3) / 4;
  const int i16 = lane & 15, g = lane >> 4, q = i16 >> 2, p = i16 & 3;
  const int t1 = 16 + i16;
  const int xoff0 = (i16 % 5) * C1W_CS + (i16 / 5) * C1W_RS + 8 * g;
  const int xoff1 = t1 < 25 ? (t1 % 5) * C1W_CS + (t1 / 5) * C1W_RS + 8 * g : 0;
  const uint32_t b1fill = t1 == 25 ? 0x3f803f80u : 0u;
  f32x4 acc1[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m) acc1[m][0] = acc1[m][1] = zero_f32x4();
  const int o_lane = ((8 * (g & 1) + q) * C2_ORS + 4 * p) * 2;
  const int c_lane = (i16 >> 1) * 16 + 8 * (g & 1);
  const uint32_t csh = 4 * (i16 & 1) + 2 * (g >> 1);  // this lane's two code bits: channel parity, row half
  struct C1F {
    uint2 d[2][2];  // [m-tile][windows 8 (G & 1) .., + 4]
    uint2 cu[2];
    bf16x8 b0[2], b1[2];  // [row half]
  };
  // oimg / ximg / cimg: byte offsets of the image's da1, input copies and codes
  auto c1_read = [&](int py, int oimg, int ximg, int cimg, C1F& f) {
    int oa = oimg + py * (13 * C2_ORS * 2) + o_lane, ca = cimg + py * 256 + c_lane;
    int x0 = ximg + py * (2 * C1W_RS * 2) + xoff0 * 2, x1 = ximg + py * (2 * C1W_RS * 2) + xoff1 * 2;
    asm("" : "+v"(oa), "+v"(ca), "+v"(x0), "+v"(x1));  // one VGPR address each; the rest are immediate offsets
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        f.d[m][h] = __builtin_bit_cast(
            uint2, lds_read_tr16(reinterpret_cast<const bf16*>(smem + oa) + h * 4 * C2_ORS + m * 16));
      f.cu[m] = *reinterpret_cast<const uint2*>(smem + ca + m * 128);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f.b0[h] = *reinterpret_cast<const bf16x8*>(smem + x0 + h * C1W_RS * 2);
      f.b1[h] = *reinterpret_cast<const bf16x8*>(smem + x1 + h * C1W_RS * 2);
    }
  };
  auto c1_mma = [&](const C1F& f) {
    bf16x8 A[2];
    int ix[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint32_t ux = f.cu[m].x >> csh, uy = f.cu[m].y >> csh;  // byte e, bits 0-1: 1 -> dx 0, 2 -> dx 1, 0 -> dead
      const uint32_t lx = (ux | (ux >> 1)) & 0x01010101u, ly = (uy | (uy >> 1)) & 0x01010101u;
      // byte e of lx / ly -> the 16-bit half of slot e: v_perm_b32 selectors, 0x0c = a zero byte
      A[m] = __builtin_bit_cast(
          bf16x8, make_uint4(pk_mul_u16(f.d[m][0].x, __builtin_amdgcn_perm(0u, lx, 0x0c010c00u)),
                             pk_mul_u16(f.d[m][0].y, __builtin_amdgcn_perm(0u, lx, 0x0c030c02u)),
                             pk_mul_u16(f.d[m][1].x, __builtin_amdgcn_perm(0u, ly, 0x0c010c00u)),
                             pk_mul_u16(f.d[m][1].y, __builtin_amdgcn_perm(0u, ly, 0x0c030c02u))));
      // dx of windows 0..3 at bits 8e, of windows 4..7 at bits 8e + 1; gathered to bits 2e and 2e + 1 (the
      // product's terms fall on distinct bits: no carries; the 24-bit multiply drops e = 3, taken by the shift)
      const uint32_t E = ((ux >> 1) & 0x01010101u) | (uy & 0x02020202u);
      const uint32_t G = ((__umul24(E, 0x1041u) >> 12) & 0x3fu) | ((E >> 18) & 0xc0u);
      ix[m] = (int)((G & 0x55u) | ((G & 0xaau) << 7) | 0x8888u);
    }
    bf16x16 B0 = __builtin_shufflevector(f.b0[0], f.b0[1], 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    bf16x16 B1 = __builtin_shufflevector(f.b1[0], f.b1[1], 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    if (t1 >= 25) {
      const bf16x8 fill = __builtin_bit_cast(bf16x8, make_uint4(b1fill, b1fill, b1fill, b1fill));
      B1 = __builtin_shufflevector(fill, fill, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      acc1[m][0] = smfmac16x16x64(A[m], B0, acc1[m][0], ix[m]);
      acc1[m][1] = smfmac16x16x64(A[m], B1, acc1[m][1], ix[m]);
    }
  };
  // this wave's steps of image j (its da1 is complete: call it in step j + 1)
  auto c1_image = [&](int j) {
    const int oimg = 2 * C2D_P + (j & 1) * C12_O;
    const int ximg = 2 * (C2D_P + C12_O) + (j % 3) * C12_XS;
    const int cimg = 2 * (C2D_P + C12_O) + 3 * C12_XS + (j % 3) * C1I_IMG;
    for (int i = 0, py = k0; i < kcnt; ++i, py += kst) {
      C1F f;
      c1_read(py, oimg, ximg, cimg, f);
      c1_mma(f);
    }
  };
  if (wave < 4) {
    // ---- MFMA waves: m-tiles wave, wave + 4, wave + 8 (< 11), both n-tiles.  Weights are the A operand
    // (the B-fragment pack read as A: the same lane -> (channel, k) map), so a lane's 4 results are 4
    // consecutive input channels of one position: one 8-byte store each.
    const int r16 = lane & 15, q8 = (lane >> 4) * 8, c4 = (lane >> 4) * 4;
    const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P2D_OFF);
    bf16x8 bw[2][18];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int ks = 0; ks < 18; ++ks) bw[nt][ks] = pk[(nt * 18 + ks) * 64 + lane];
    int base[3], opos[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int mt = min(wave + 4 * k, 10);
      const int mm = c2d_tile_pos[mt * 16 + r16];
      opos[k] = mm;
      base[k] = mm == 255 ? 0 : (mm / 13) * C2_PW + mm % 13;
    }
    auto phase = [&](auto nk_c, const bf16* P, bf16* O, int s) {
      constexpr int NK = decltype(nk_c)::value;
      f32x4 acc[NK][2];
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[k][0] = acc[k][1] = zero_f32x4();
#pragma unroll
      for (int ks = 0; ks < 18; ++ks) {
        const int tapp = ks >> 1, c0 = (ks & 1) * 32;
        const int shift = (tapp / 3) * C2_PW + tapp % 3;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(P + (base[k] + shift) * C2_PRS + c0 + q8);
          acc[k][0] = mfma16x16x32(bw[0][ks], a, acc[k][0]);
          acc[k][1] = mfma16x16x32(bw[1][ks], a, acc[k][1]);
        }
      }
      C12_ST(s, 1);
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (opos[k] < 169) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            *reinterpret_cast<bf16x4*>(O + opos[k] * C2_ORS + nt * 16 + c4) =
                bf16x4{(bf16)acc[k][nt][0], (bf16)acc[k][nt][1], (bf16)acc[k][nt][2], (bf16)acc[k][nt][3]};
        }
      }
    };
    lds_barrier();  // [B1] image 0 staged
    for (int s = 0; s <= n; ++s) {
      C12_ST(s, 0);
      if (s < n && !(ablate & 2)) {
        if (wave < 3)
          phase(std::integral_constant<int, 3>{}, Pb(s & 1), Ob(s & 1), s);
        else
          phase(std::integral_constant<int, 2>{}, Pb(s & 1), Ob(s & 1), s);
      }
      C12_ST(s, 2);
      if (s >= 1 && !(ablate & 1)) c1_image(s - 1);
      C12_ST(s, 3);
      lds_barrier();
    }
  } else {
    // ---- conv1-wgrad / staging waves: thread vt of 256
    const int vt = tid - 256;
    // the next images' inputs in registers, two sets: image j's set is j & 1, loaded two steps before it is
    // staged (one step of latency hiding was not enough: staging alone ran at the per-CU latency bound).
    // (Staging dz2 from the MFMA waves instead measured 935 -> 1024 us in round 5.)
    struct Regs {
      bf16x8 pz[4];
      uint4 pc;
      uint32_t xu;
      float4 xf;
    };
    Regs r0, r1;
    auto load = [&](Regs& r, int bb) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(dz2 + (int64_t)bb * 121 * 64);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (vt + 256 * j < 968) r.pz[j] = src[vt + 256 * j];
      if (vt < C1I_IMG / 16) r.pc = reinterpret_cast<const uint4*>(idx1 + (int64_t)bb * C1I_IMG)[vt];
      c1_load<U8>(xin, bb, vt, r.xu, r.xf);
    };
    auto stage = [&](const Regs& r, int k2, int k3) {
      bf16* P = Pb(k2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = vt + 256 * j;
        if (c < 968) {
          const int pos = c >> 3, cc = (c & 7) * 8;
          *reinterpret_cast<bf16x8*>(P + ((pos / 11 + 2) * C2_PW + pos % 11 + 2) * C2_PRS + cc) = r.pz[j];
        }
      }
      if (vt < C1I_IMG / 16) reinterpret_cast<uint4*>(Cb(k3))[vt] = r.pc;
      c1_store<U8, 5, C1W_RS, C1W_CS>(Xb(k3), vt, r.xu, r.xf, mean, inv_std, in_scale);
    };
    if (n > 0) {
      load(r0, block);
      stage(r0, 0, 0);
      if (n > 1) load(r1, block + nblocks);
      if (n > 2) load(r0, block + 2 * nblocks);
    }
    lds_barrier();  // [B1]
    // step s: stage image s+1 (its set (s+1) & 1), refill that set with image s+3, this wave's share of the
    // conv1 wgrad of image s-1
    auto step = [&](int s, Regs& rs) {
      if (s + 1 < n) {
        stage(rs, (s + 1) & 1, (s + 1) % 3);
        C12_ST(s, 0);
        if (s + 3 < n) load(rs, block + (s + 3) * nblocks);
      }
      C12_ST(s, 1);
      if (s >= 1 && !(ablate & 1)) c1_image(s - 1);
      C12_ST(s, 2);
      lds_barrier();
      C12_ST(s, 3);
    };
    for (int s = 0; s <= n; s += 2) {  // unrolled by 2: register sets are not indexable
      step(s, r1);
      if (s + 1 <= n) step(s + 1, r0);
    }
  }
  // combine the 8 waves' partial sums in a fixed order (deterministic) and write this workgroup's conv1 slab
  __syncthreads();  // [R0] P is free
  float* red = reinterpret_cast<float*>(smem);  // [wave][tile][lane][4]: 32 KiB over P
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
      *reinterpret_cast<f32x4*>(red + ((wave * 4 + m * 2 + nn) * 64 + lane) * 4) = acc1[m][nn];
  __syncthreads();  // [R1]
  if (wave >= 4) {
    const int tile = wave - 4;
    f32x4 sum = *reinterpret_cast<const f32x4*>(red + (tile * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 8; ++w) sum += *reinterpret_cast<const f32x4*>(red + ((w * 4 + tile) * 64 + lane) * 4);
    float* slab = slabs1 + (int64_t)block * C1_WSLAB;
    const int tap = (tile & 1) * 16 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = (tile >> 1) * 16 + g * 4 + r;
      if (tap < 25) slab[co * 25 + tap] = sum[r];
      if (tap == 25) slab[800 + co] = sum[r];
    }
  }
}

// conv2 wgrad, 8 waves: wave (wm2 = wave & 1, wn = wave >> 1) owns co tiles 2wm2, 2wm2+1 x the n-tiles
// (tap, half) of dW2t [288][64] with half = wn & 1 (input channels 16 half ..) and taps h, h+2, .. (h = wn >> 1:
// 5 taps for h = 0, 4 for h = 1); the tap part of every X address is an immediate offset (body<H>).  The
// wn = 0 waves also form the bias column sums.  Three D / X image buffers, as conv3_wgrad8_role: image i+1's
// first A fragments are read before the barrier that ends image i.  The inputs are staged from registers
// loaded one image ahead (an LDS-DMA form with per-lane sources - 37 wave-instructions per image into the
// padded layouts - measured 1044 vs 782 us for this role at B=65536).
__device__ __forceinline__ void conv2_wgrad8_role(char* smem, const bf16* __restrict__ a1, const bf16* __restrict__ dz2,
                                                  float* __restrict__ slabs, int B, int nslices, int slice) {
  auto Db = [&](int k) { return reinterpret_cast<bf16*>(smem + k * C2W_D); };
  auto Xb = [&](int k) { return reinterpret_cast<bf16*>(smem + 3 * C2W_D + k * C2W_X); };
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm2 = wave & 1, wn = wave >> 1, half = wn & 1, h = wn >> 1;
  const int g16 = lane & 15, grp = lane >> 4, q = g16 >> 2, p = g16 & 3;
  const bf16x8 onesf = ones_column_frag(lane);
  f32x4 acc[2][5], accb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    accb[m] = zero_f32x4();
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[m][j] = zero_f32x4();
  }
  // rows >= 121 of the three D images stay zero
  for (int c = tid; c < 3 * C2W_D / 16; c += 512) reinterpret_cast<bf16x8*>(smem)[c] = zero_bf16x8();
  // images slice, slice + nslices, ... (as the dgrad workgroups)
  const int n = slice < B ? (B - slice + nslices - 1) / nslices : 0;
  auto img = [&](int i) { return slice + i * nslices; };
  // inputs of later images in registers, two sets (image j: set j & 1, loaded two images before it is staged)
  struct Regs {
    bf16x8 pz[2], pa[2];
  };
  Regs r0, r1;
  auto load = [&](Regs& r, int bb) {
    const bf16x8* zs = reinterpret_cast<const bf16x8*>(dz2 + (int64_t)bb * 121 * 64);
    const bf16x8* as = reinterpret_cast<const bf16x8*>(a1 + (int64_t)bb * 169 * 32);
    r.pz[0] = zs[tid];
    if (tid + 512 < 968) r.pz[1] = zs[tid + 512];
    r.pa[0] = as[tid];
    if (tid + 512 < 676) r.pa[1] = as[tid + 512];
  };
  auto stage = [&](const Regs& r, int k) {
    bf16* D = Db(k);
    bf16* X = Xb(k);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = tid + 512 * j;
      if (c < 968) *reinterpret_cast<bf16x8*>(D + c2_drow(c >> 3) + (c & 7) * 8) = r.pz[j];
      if (c < 676) *reinterpret_cast<bf16x8*>(X + (c >> 2) * C2_XRS + (c & 3) * 8) = r.pa[j];
    }
  };
  auto readA = [&](int buf, int ks, bf16x8 (&af)[2]) {
    const bf16* D = Db(buf) + 32 * wm2 + 4 * p;
    const int kb = ks * 32 + grp * 8;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const bf16x4 alo = lds_read_tr16(D + c2_drow(kb + q) + m * 16);
      const bf16x4 ahi = lds_read_tr16(D + c2_drow(kb + 4 + q) + m * 16);
      af[m] = bf16x8{alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
    }
  };
  __syncthreads();  // zero fill before the first stage
  if (n > 0) {
    load(r0, img(0));
    stage(r0, 0);
    if (n > 1) {
      load(r1, img(1));
      stage(r1, 1);
    }
    if (n > 2) load(r0, img(2));
    if (n > 3) load(r1, img(3));
  }
  lds_barrier();
  bf16x8 af[2], afn[2];
  if (n > 0) readA(0, 0, af);
  auto body = [&](auto h_c) {
    constexpr int H = decltype(h_c)::value;
    constexpr int NJ = H == 0 ? 5 : 4;
    auto image = [&](int i, Regs& rs) {
      const int cur = i % 3;
      // image i+2 (set rs) into the buffers image i-1 used; rs refilled with image i+4.  Waves 0-3 do it before
      // their k-steps and waves 4-7 after theirs: waves w and w + 4 share a SIMD, so one of the two has MFMAs
      // to issue while the other writes LDS and forms load addresses.
      const bool early = wave < 4;
      if (early && i + 2 < n) {
        stage(rs, (i + 2) % 3);
        if (i + 4 < n) load(rs, img(i + 4));
      }
      C12_ST(i, 0);
      const int xb = (int)(Xb(cur) - reinterpret_cast<const bf16*>(smem)) + 16 * half + 4 * p;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int kb = ks * 32 + grp * 8;
        const int k0 = min(kb + q, 120), k1 = min(kb + 4 + q, 120);  // rows >= 121 of D are zero
        int x0 = xb + ((k0 / 11) * 13 + k0 % 11) * C2_XRS, x1 = xb + ((k1 / 11) * 13 + k1 % 11) * C2_XRS;
        asm("" : "+v"(x0), "+v"(x1));  // as conv3_wgrad8_role: one VGPR base + immediate tap offsets
        const bf16* S0 = reinterpret_cast<const bf16*>(smem);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int tap = 2 * j + H;
          const int shift = ((tap / 3) * 13 + tap % 3) * C2_XRS;
          const bf16x4 lo = lds_read_tr16(S0 + x0 + shift);
          const bf16x4 hi = lds_read_tr16(S0 + x1 + shift);
          const bf16x8 bf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          if (j == 2) {  // next k-step's A fragments (image i+1's first after the last k-step); af and afn
                         // alternate by k-step parity, so nothing is copied
            if (ks < 3) {
              if (ks & 1)
                readA(cur, ks + 1, af);
              else
                readA(cur, ks + 1, afn);
            } else if (i + 1 < n) {
              readA((i + 1) % 3, 0, af);
            }
          }
#pragma unroll
          for (int m = 0; m < 2; ++m) acc[m][j] = mfma16x16x32((ks & 1) ? afn[m] : af[m], bf, acc[m][j]);
        }
        if (wn == 0) {
#pragma unroll
          for (int m = 0; m < 2; ++m) accb[m] = mfma16x16x32((ks & 1) ? afn[m] : af[m], onesf, accb[m]);
        }
      }
      C12_ST(i, 1);
      if (!early && i + 2 < n) {
        stage(rs, (i + 2) % 3);
        if (i + 4 < n) load(rs, img(i + 4));
      }
      lds_barrier();
      C12_ST(i, 2);
    };
    for (int i = 0; i < n; i += 2) {  // unrolled by 2: register sets are not indexable
      image(i, r0);
      if (i + 1 < n) image(i + 1, r1);
    }
  };
  if (h == 0)
    body(std::integral_constant<int, 0>{});
  else
    body(std::integral_constant<int, 1>{});
  float* slab = slabs + (int64_t)slice * C2_WSLAB;
  const int nj = h == 0 ? 5 : 4;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int co = (2 * wm2 + m) * 16 + grp * 4;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (j < nj) {
        const int nn = ((2 * j + h) * 2 + half) * 16 + g16;  // n-tile (tap, half)
        *reinterpret_cast<f32x4*>(slab + (int64_t)nn * 64 + co) = acc[m][j];
      }
    }
    if (wn == 0 && g16 == 0) *reinterpret_cast<f32x4*>(slab + 288 * 64 + co) = accb[m];
  }
}

template <bool U8>
__global__ __launch_bounds__(512, 1) void conv12_bwd8_kernel(const void* __restrict__ xin,
                                                            const uint8_t* __restrict__ idx1,
                                                            const bf16* __restrict__ a1,
                                                            const bf16* __restrict__ dz2,
                                                            const bf16* __restrict__ packed, int B, float mean,
                                                            float inv_std, float in_scale,
                                                            float* __restrict__ slabs2, int nslices,
                                                            float* __restrict__ slabs1, int n_dgrad, int ablate) {
  __shared__ __attribute__((aligned(16))) char smem[C12V_LDS + C12_ST_BYTES];
  if ((int)blockIdx.x < n_dgrad)
    conv12_dgrad8_role<U8>(smem, xin, idx1, dz2, packed, B, blockIdx.x, n_dgrad, mean, inv_std, in_scale, slabs1,
                           ablate);
  else if (!(ablate & 4))
    conv2_wgrad8_role(smem, a1, dz2, slabs2, B, nslices, blockIdx.x - n_dgrad);
#ifdef RINGDP_C12_STAMPS
  __syncthreads();
  const bool dg = (int)blockIdx.x < n_dgrad;
  const int blk = dg ? blockIdx.x : blockIdx.x - n_dgrad, nb = dg ? n_dgrad : nslices;
  if (blk == C12_ST_BLK && threadIdx.x == 0 && (B - blk) / nb > C12_ST_S0 + 8) {
    const unsigned long long* st = reinterpret_cast<const unsigned long long*>(smem + C12V_LDS);
    const unsigned long long t0 = st[0];  // wave 0's first stamp
    for (int w = 0; w < 8; ++w)
      for (int k = 0; k < 8; ++k) {
        const unsigned long long* r = st + (w * 8 + k) * 4;
        printf("C12ST %c w%d s%d %lld %lld %lld %lld\n", dg ? 'd' : 'w', w, k, (long long)(r[0] - t0),
               (long long)(r[1] - t0), (long long)(r[2] - t0), dg ? (long long)(r[3] - t0) : 0ll);
      }
  }
#endif
}

}  // namespace

static void c2_split(int B, bool dgrad, int& nd, int& ws) {
  const int cus = num_cus();
  if (!dgrad) {
    nd = 0;
    ws = clampi(cdiv(B, 8), 1, cus);
    return;
  }
  static const double frac = env_real("RINGDP_C2_DGRAD_FRAC", 0.55, split_frac_ok);
  nd = clampi(B, 1, (int)(frac * cus));
  const int per = cdiv(B, nd);
  ws = clampi(cdiv(B, std::max(per, 2)), 1, std::max(1, cus - nd));  // >= 2 images per slab
}

// fused conv2 backward + conv1 wgrad: the dgrad role also does conv1 wgrad (104 MFMAs per image on top
// of conv2 dgrad's 396, 52 sparse ones in the 8-wave kernel; conv2 wgrad: 304).  Wave-specialised kernel (conv12_bwd8_kernel): the conv3 bwd8
// batches (use_8wave); up to them the unpipelined kernel (conv12_bwd_kernel)
static void c12_split(int B, int& nd, int& ws) {
  const int cus = num_cus();
  if (use_8wave(B)) {
    static const double frac3 = env_real("RINGDP_C12_DGRAD_FRAC", 0.56, split_frac_ok);
    nd = clampi(((int)(frac3 * cus) + 4) / 8 * 8, 8, cus - 8);  // multiples of 8: see conv2_wgrad8_role
    ws = clampi(cdiv(B, 8), 1, cus - nd);
    return;
  }
  static const double frac = env_real("RINGDP_C12_DGRAD_FRAC", 0.64, split_frac_ok);
  static const int wmin = env_int("RINGDP_C12_WMIN", 2, slab_images_ok);
  nd = clampi(B, 1, (int)(frac * cus));
  const int per = cdiv(B, nd);
  ws = clampi(cdiv(B, std::max(per, wmin)), 1, std::max(1, cus - nd));
}

static int conv1_wslices(int B) { return clampi(cdiv(B, 4), 1, 3 * num_cus()); }

int64_t cn_conv2_slab_floats(int B, bool dgrad) {
  int nd, ws;
  c2_split(B, dgrad, nd, ws);
  return (int64_t)ws * C2_WSLAB;
}
int64_t cn_conv12_slab_floats(int B) {
  int nd, ws;
  c12_split(B, nd, ws);
  return (int64_t)ws * C2_WSLAB + (int64_t)nd * C1_WSLAB;
}
int64_t cn_conv1_slab_floats(int B) { return (int64_t)conv1_wslices(B) * C1_WSLAB; }

void cn_conv2_bwd(const void* a1, const void* dz2, const void* packed, void* da1, int B, float* slabs,
                  float* dw2, float* db2, hipStream_t s) {
  int nd, ws;
  c2_split(B, da1 != nullptr, nd, ws);
  conv2_bwd_kernel<<<nd + ws, 512, 0, s>>>(static_cast<const bf16*>(a1), static_cast<const bf16*>(dz2),
                                           static_cast<const bf16*>(packed), static_cast<bf16*>(da1), B, slabs,
                                           ws, nd);
  launch_reduce({seg(slabs, C2_WSLAB, 0, 288 * 64, ws, dw2, 1, 32, 64), seg(slabs, C2_WSLAB, 288 * 64, 64, ws, db2)},
                s);
}

void cn_conv12_bwd(const void* x, bool u8, const uint8_t* idx1, const void* a1, const void* dz2,
                   const void* packed, int B, float mean, float inv_std, float in_scale, float* slabs, float* dw2,
                   float* db2, float* dw1, float* db1, hipStream_t s, const ReduceList* extra) {
  int nd, ws;
  c12_split(B, nd, ws);
  float *slabs2 = slabs, *slabs1 = slabs + (int64_t)ws * C2_WSLAB;
  const bf16 *a1b = static_cast<const bf16*>(a1), *dzb = static_cast<const bf16*>(dz2),
             *pk = static_cast<const bf16*>(packed);
  dispatch_bool(u8, [&](auto U8) {
    if (use_8wave(B))
      conv12_bwd8_kernel<decltype(U8)::value><<<nd + ws, 512, 0, s>>>(x, idx1, a1b, dzb, pk, B, mean, inv_std, in_scale,
                                                                      slabs2, ws, slabs1, nd, C12_ABLATE);
    else
      conv12_bwd_kernel<decltype(U8)::value><<<nd + ws, 512, 0, s>>>(x, idx1, a1b, dzb, pk, B, mean, inv_std, in_scale,
                                                                     slabs2, ws, slabs1, nd);
  });
  ReduceList r = extra ? *extra : ReduceList{};  // a deferred conv3 / fc1 reduction rides along
  for (const ReduceSeg& g : {seg(slabs2, C2_WSLAB, 0, 288 * 64, ws, dw2, 1, 32, 64),
                             seg(slabs2, C2_WSLAB, 288 * 64, 64, ws, db2), seg(slabs1, C1_WSLAB, 0, 800, nd, dw1),
                             seg(slabs1, C1_WSLAB, 800, 32, nd, db1)})
    r.push_back(g);
  launch_reduce(r, s);
}

void cn_conv1_wgrad(const void* x, bool u8, const void* da1, const uint8_t* idx1, int B, float mean,
                    float inv_std, float in_scale, float* slabs, float* dw1, float* db1, hipStream_t s) {
  const int ws = conv1_wslices(B);
  dispatch_bool(u8, [&](auto U8) {
    conv1_wgrad_kernel<decltype(U8)::value><<<ws, 256, 0, s>>>(x, static_cast<const bf16*>(da1), idx1, B, mean, inv_std,
                                                               in_scale, slabs, ws);
  });
  launch_reduce({seg(slabs, C1_WSLAB, 0, 800, ws, dw1), seg(slabs, C1_WSLAB, 800, 32, ws, db1)}, s);
}

}  // namespace kern
}  // namespace ringdp
