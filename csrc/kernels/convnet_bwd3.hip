// bf16 ConvNet (design: convnet_fwd.hip), F3 backward: fc1 backward, the 4-wave and the 8-wave conv3 backward
// (data gradient through pool2 + ReLU, weight gradient), their work split and launcher.
#include "convnet_device.h"
#include "convnet_host.h"

namespace ringdp::kern {
namespace {
// ================================================================== F3 backward
// (1) fc1 backward, one pass over a3: compact data gradient
//       da3m[b][w][co] = (a3 > 0) * sum_n dl[b][n] * Wfc[n][co*16 + w]     (bf16, Wfc from the pack)
//     and the fc1 weight/bias gradient of this block's images as an fp32 slab.  The conv3 backward
//     roles expand da3m to window-ordered rows (row 4w + argmax) in LDS; the 8-wave weight-gradient role feeds
//     it, unexpanded, to the sparse MFMA.
// images per workgroup: enough workgroups to fill the chip at small batches (B=100: 25 of 4 images,
// was 4 of 32 and latency-bound at 21 us), fewer fp32 slabs at large ones (B=32768: 512 of 64 images,
// halving the 84 MB of slab traffic)
__host__ __device__ inline int fc_imgs(int B) { return B <= 1024 ? 4 : (B >= 65536 ? 128 : (B >= 32768 ? 64 : 32)); }
constexpr int FC_SLAB = 10 * 2048 + 10 + 128 + 2;  // dWfc + dbfc + db3 (the conv3 bias gradient is the sum
                                                    // of d(a3) over windows: no MFMA tile needed for it),
                                                    // padded to a 16-B multiple (vector slab reduction)

// kCE: the logits gradient is formed here from the cross-entropy forward's logits / log-sum-exp
// (same expression as ce_bwd_kernel, elementwise.hip) - 80 threads per group of 8 images into LDS -
// instead of read from a [B,10] tensor: the separate ce_bwd launch disappears.
// The body runs as its own launch (fc_bwd_kernel) or as the first workgroups of the conv3 backward launch at
// small batches (conv3_bwd_kernel, blk = that workgroup's fc index; da3m == nullptr: the conv3
// roles form their own compact gradient, C3Pre::load).
template <bool kCE>
__device__ __forceinline__ void fc_bwd_body(const bf16* __restrict__ a3, const bf16* __restrict__ packed,
                                            const float* __restrict__ dl, bf16* __restrict__ da3m,
                                            float* __restrict__ slabs, int B, int imgs, const CeFuse& ce, int blk) {
  const int t = threadIdx.x;
  const int wd = t >> 4, co0 = (t & 15) * 8;  // this thread's 8 activations: window wd, channels co0..
  float wr[8][10];
  {
    // Pfc is [w][co][n]: this thread's 80 weights are contiguous (10 x 16 B)
    const bf16x8* src = reinterpret_cast<const bf16x8*>(packed + PFC_OFF + (wd * 128 + co0) * 10);
#pragma unroll
    for (int h = 0; h < 10; ++h) {
      const bf16x8 v = src[h];
#pragma unroll
      for (int e = 0; e < 8; ++e) wr[(8 * h + e) / 10][(8 * h + e) % 10] = (float)v[e];
    }
  }
  float acc[8][10];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int n = 0; n < 10; ++n) acc[j][n] = 0.f;
  float bacc = 0.f, dsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dsum[j] = 0.f;
  const int b0 = blk * imgs, nimg = min(imgs, B - b0);
  // kCE: the logits gradient of all this block's images (<= 128 x 10) formed once into LDS, one barrier
  __shared__ float gl[128 * 10];
  if constexpr (kCE) {
    const float ce_scale = ce.reduction == 0 ? 1.f : ce.grad_out[0] / ce.denom[0];
    for (int e = t; e < nimg * 10; e += 256) {
      const int k = e / 10, n = e - 10 * k, b = b0 + k;
      float g = 0.f;
      const int64_t y = ce.labels[b];
      if (y != ce.ignore_index) {
        const float p = __expf(ce.logits[(int64_t)b * 10 + n] - ce.lse[b]);
        const float q = (n == y ? (1.f - ce.eps) : 0.f) + ce.eps / 10.f;
        g = (p - q) * (ce.reduction == 0 ? ce.grad_out[b] : ce_scale);
      }
      gl[e] = g;
    }
    __syncthreads();
  }
  for (int k0 = 0; k0 < nimg; k0 += 8) {
    bf16x8 av[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k0 + k < nimg) av[k] = *reinterpret_cast<const bf16x8*>(a3 + (int64_t)(b0 + k0 + k) * 2048 + wd * 128 + co0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k0 + k < nimg) {
        const int b = b0 + k0 + k;
        float g[10];
#pragma unroll
        for (int n = 0; n < 10; ++n) g[n] = kCE ? gl[(k0 + k) * 10 + n] : dl[(int64_t)b * 10 + n];
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float aj = (float)av[k][j];
          float s = 0.f;
#pragma unroll
          for (int n = 0; n < 10; ++n) {
            s = fmaf(g[n], wr[j][n], s);
            acc[j][n] = fmaf(g[n], aj, acc[j][n]);
          }
          const float m = aj > 0.f ? s : 0.f;
          dsum[j] += m;
          v[j] = (bf16)m;
        }
        if (da3m) *reinterpret_cast<bf16x8*>(da3m + (int64_t)b * 2048 + wd * 128 + co0) = v;
        if (t < 10) bacc += kCE ? gl[(k0 + k) * 10 + t] : dl[(int64_t)b * 10 + t];
      }
    }
  }
  // slab in thread order (coalesced): element (n*8 + j)*256 + t; the reduction (mode 2) maps it back
  // to dWfc[n][co*16 + w]
  float* slab = slabs + (int64_t)blk * FC_SLAB;
#pragma unroll
  for (int n = 0; n < 10; ++n)
#pragma unroll
    for (int j = 0; j < 8; ++j) slab[(n * 8 + j) * 256 + t] = acc[j][n];
  if (t < 10) slab[20480 + t] = bacc;
  // db3 partial: sum the 16 windows (4 per wave via lane shuffles, then the 4 waves) per channel
  __shared__ float red[4][128];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = dsum[j];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    dsum[j] = v;
  }
  if ((t & 63) < 16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[t >> 6][co0 + j] = dsum[j];
  }
  __syncthreads();
  if (t < 128) slab[20490 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

template <bool kCE>
__global__ __launch_bounds__(256) void fc_bwd_kernel(const bf16* __restrict__ a3, const bf16* __restrict__ packed,
                                                     const float* __restrict__ dl, bf16* __restrict__ da3m,
                                                     float* __restrict__ slabs, int B, int imgs, CeFuse ce) {
  fc_bwd_body<kCE>(a3, packed, dl, da3m, slabs, B, imgs, ce, blockIdx.x);
}

// (2) conv3 backward, two roles in one launch of 256-thread workgroups, two per CU (a CU usually
//     hosts one of each, so one role's barrier-separated phases overlap the other's MFMA stream):
//   dgrad: da2 = full-corr(d(conv3) image, flipped W3), then pool2 + ReLU backward: each da2 value goes
//          to the z2 position its pool2 code names (F2 forward) -> dz2 [B,11,11,64];
//   wgrad: dW3t[n = tap*64 + ci][co] = sum_k D3[k][co] * a2[pos(k) + tap][ci], a workgroup pair per
//          image slice (one half of the 576 n columns each).  db3 comes from fc1's backward.
// d(conv3) image in LDS with two zero rows above and below (12 rows x 8 columns): position (Y, X) at
// Y*C3_PY + X*C3_PX bf16.  288-B positions and unpadded 2304-B rows make every B-fragment read of the
// dgrad GEMM (lanes = 2 rows x 8 columns of one 16-B channel chunk) conflict-free: 4 LDS cycles per
// ds_read_b128 (tools/lds_bank_model.py; the 12x12 ring layout with 3648-B rows read these in 8).
constexpr int C3_PX = 144;   // bf16 per position (128 + 16)
constexpr int C3_PY = 1152;  // bf16 per row of positions (8 * 144)
constexpr int C3_DARS = 68;  // floats per da2 row (64 + 4)
constexpr int C3_DRS = 136;  // bf16 per D3 row in LDS
constexpr int C3D_P = 12 * C3_PY * 2;                       // 27648
constexpr int C3D_AM = 100 * 64;                            // 6400: pool2 codes of the current image
constexpr int C3D_DA = 100 * C3_DARS * 4;                   // 27200
constexpr int C3D_LDS = C3D_P + C3D_AM + C3D_DA;
static_assert(C3D_P % 16 == 0 && C3D_LDS <= 81920, "two conv3 backward workgroups per CU");
constexpr int C3W_D = 64 * C3_DRS * 2;   // 17408
constexpr int C3W_X = 100 * C3_XRS * 2;  // 14400
constexpr int C3W_R = 100 * 64 * 2;      // 12800: DMA staging of the next a2 image
constexpr int C3W_LDS = C3W_D + C3W_X + C3W_R;
constexpr int C3B_LDS = C3D_LDS > C3W_LDS ? C3D_LDS : C3W_LDS;
constexpr int C3_WSLAB = 576 * 128;  // dW3t

// The compact F3-backward input of one image, held in registers while the previous image is
// computed on: d(a3) chunk + its pool3 argmax bytes (threads < 256).
// What the 4-wave conv3 backward roles (small batches, fc1 backward inside their launch) form an image's
// compact d(a3) from: a3, the logits gradient and the packed fc1 weights - the same expression and order as
// fc_bwd_body, so the values are bit-identical to the da3m that fc_bwd_kernel leaves for the 8-wave kernel.
struct C3Src {
  const bf16* a3;
  const bf16* packed;
  const float* dl;   // logits gradient, or null with ce
  CeFuse ce;
};

struct C3Pre {
  bf16x8 da;
  uint2 id;
  __device__ __forceinline__ void load(const C3Src& src, const uint8_t* __restrict__ idx3, int b, int tid) {
    if (tid < 256) {
      id = reinterpret_cast<const uint2*>(idx3 + (int64_t)b * 2048)[tid];
      const int wd = tid >> 4, co0 = (tid & 15) * 8;
      const bf16x8 av = reinterpret_cast<const bf16x8*>(src.a3 + (int64_t)b * 2048)[tid];
      float g[10];
      if (src.dl) {
#pragma unroll
        for (int n = 0; n < 10; ++n) g[n] = src.dl[(int64_t)b * 10 + n];
      } else {
        const CeFuse& ce = src.ce;
        const int64_t y = ce.labels[b];
        const float sc = ce.reduction == 0 ? ce.grad_out[b] : ce.grad_out[0] / ce.denom[0];
        const float lse = ce.lse[b];
#pragma unroll
        for (int n = 0; n < 10; ++n) {
          float gv = 0.f;
          if (y != ce.ignore_index) {
            const float p = __expf(ce.logits[(int64_t)b * 10 + n] - lse);
            const float q = (n == y ? (1.f - ce.eps) : 0.f) + ce.eps / 10.f;
            gv = (p - q) * sc;
          }
          g[n] = gv;
        }
      }
      const bf16x8* wsrc = reinterpret_cast<const bf16x8*>(src.packed + PFC_OFF + (wd * 128 + co0) * 10);
      bf16x8 wv[10];
#pragma unroll
      for (int h = 0; h < 10; ++h) wv[h] = wsrc[h];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < 10; ++n) s = fmaf(g[n], (float)wv[(10 * j + n) / 8][(10 * j + n) % 8], s);
        da[j] = (bf16)((float)av[j] > 0.f ? s : 0.f);
      }
    }
  }
};

// Rows 0..3 of one channel pair: d = bf16 pair (channel 2k low, 2k+1 high), t = their pool3 argmax
// (0..3) in bits 0-1 of each halfword; row i keeps a channel iff its argmax == i.  The argmax bit planes
// become halfword sign masks (two packed shifts each) and every row is one v_bitop3 - 9 VALU per 8
// outputs instead of a compare + select per output.
typedef short s16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void c3_rows(uint32_t d, uint32_t t, uint32_t& r0, uint32_t& r1, uint32_t& r2,
                                        uint32_t& r3) {
  const s16x2v ts = __builtin_bit_cast(s16x2v, t);
  const uint32_t a0 = __builtin_bit_cast(uint32_t, (s16x2v)(ts << 15) >> 15);  // halfword = -(argmax bit 0)
  const uint32_t a1 = __builtin_bit_cast(uint32_t, (s16x2v)(ts << 14) >> 15);  // halfword = -(argmax bit 1)
  // v_bitop3 truth-table index = (S0 << 2) | (S1 << 1) | S2 with S0 = d, S1 = a0, S2 = a1
  r0 = __builtin_amdgcn_bitop3_b32(d, a0, a1, 0x10);  // d & ~a0 & ~a1
  r1 = __builtin_amdgcn_bitop3_b32(d, a0, a1, 0x40);  // d &  a0 & ~a1
  r2 = __builtin_amdgcn_bitop3_b32(d, a0, a1, 0x20);  // d & ~a0 &  a1
  r3 = __builtin_amdgcn_bitop3_b32(d, a0, a1, 0x80);  // d &  a0 &  a1
}

// Expand compact item tid (window w = tid >> 4, channels cc..cc+7) to the 4 window-ordered rows.
template <typename RowPtr>
__device__ __forceinline__ void c3_expand(const C3Pre& p, int tid, RowPtr row_ptr) {
  if (tid < 256) {
    const int w = tid >> 4, cc = (tid & 15) * 8;
    const uint4 dv = __builtin_bit_cast(uint4, p.da);
    const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
    uint32_t r[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // argmax bytes 2k, 2k+1 -> the low bytes of the two halfwords
      const uint32_t id4 = k < 2 ? p.id.x : p.id.y;
      const uint32_t t = __builtin_amdgcn_perm(id4, id4, (k & 1) ? 0x0c030c02u : 0x0c010c00u);
      c3_rows(dw[k], t, r[0][k], r[1][k], r[2][k], r[3][k]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4*>(row_ptr(4 * w + i) + cc) = make_uint4(r[i][0], r[i][1], r[i][2], r[i][3]);
  }
}

// pool2 codes of one image (6400 B = 400 x 16 B) -> LDS by DMA (4 waves, 7 wave-instructions)
__device__ __forceinline__ void codes_glds(const uint8_t* __restrict__ idx2, int b, uint8_t* AM, int wave,
                                           int lane) {
  const uint8_t* src = idx2 + (int64_t)b * 6400;
  for (int k = wave; k < 7; k += 4) {
    const int slot = k * 64 + lane;
    if (slot < 400) glds16_async(src + slot * 16, AM + k * 1024);
  }
}

// dgrad per image, gathered over kernel rows and scattered over kernel columns:
//   da2[y'][x + kx][ci] += sum_{ky, co} W3[co][ci][ky][kx] * dz3[y' - ky][x][co]
// over the 8 dz3 columns x and the 10 da2 rows y', K = 128 output channels (the full correlation over
// the 10x10 a2 image with the 3x3 flipped kernel needed 252 MFMAs per wave: 900 (position, tap) pairs
// of which only 576 are non-zero; the pure scatter form 144 plus a col2im read-add-write per tap).
// Operands are swapped so a lane's 4 results are 4 consecutive input channels of one position: wave w
// owns input channels 16w..16w+15, so its col2im into the fp32 da2 image never meets another wave's.
// The kx taps of an m-tile hit the same da2 words from different lanes, so a compiler barrier keeps
// each read behind the previous write (LDS executes one wave's instructions in order).  Fixed order:
// deterministic.
__device__ __forceinline__ void conv3_dgrad_role(char* smem, const C3Src& src, const uint8_t* __restrict__ idx3,
                                 const uint8_t* __restrict__ idx2, const bf16* __restrict__ packed,
                                 bf16* __restrict__ dz2, int b_first, int b_end, int b_step) {
  bf16* P = reinterpret_cast<bf16*>(smem);
  uint8_t* AM = reinterpret_cast<uint8_t*>(smem + C3D_P);
  float* DA = reinterpret_cast<float*>(smem + C3D_P + C3D_AM);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q8 = (lane >> 4) * 8, c4 = (lane >> 4) * 4;
  const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P3D_OFF);
  bf16x8 aw[36];  // [tap][kstep] weight fragments of this wave's 16 input channels
#pragma unroll
  for (int j = 0; j < 36; ++j) aw[j] = pk[(wave * 36 + j) * 64 + lane];
  // lane r16 of m-tile mt: da2 row 2 mt + (r16 >> 3), dz3 column r16 & 7 (its kx = 0 da2 column)
  const int pbase = ((r16 >> 3) + 2) * C3_PY + (r16 & 7) * C3_PX + q8;
  const int dbase = ((r16 >> 3) * 10 + (r16 & 7)) * C3_DARS + 16 * wave + c4;
  // the zero rows of the image stay zero; only the 8x8 interior is rewritten per image
  for (int c = tid; c < C3D_P / 16; c += 256) reinterpret_cast<bf16x8*>(P)[c] = zero_bf16x8();
  // Gather over the kernel row ky, scatter over the kernel column kx.  Output m-tile mt = da2 rows
  // 2mt, 2mt+1 at the 8 dz3 columns x: for each ky the B fragments are the dz3 rows y' - ky (a row
  // offset into the zero-ringed image), and the three kx taps accumulate in three register tiles that
  // land on da2 columns x, x+1, x+2.  13 (mt, ky) pairs hold a non-zero row (mt 0 has no ky 2, mt 4
  // no ky 0): 156 MFMAs per wave (pure scatter: 144), but the fp32 col2im is one store + two
  // read-add-writes per m-tile (15 + 10 per wave) instead of a read-add-write per tap (72 + 72): the
  // 13-cycle ds_write_b128 traffic of that col2im had been as long as the MFMA stream itself.
  const int xcol = r16 & 7;
  auto mfma_phase = [&]() {
#pragma unroll
    for (int mt = 0; mt < 5; ++mt) {
      f32x4 acc[3] = {zero_f32x4(), zero_f32x4(), zero_f32x4()};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        if ((mt == 0 && ky == 2) || (mt == 4 && ky == 0)) continue;  // both rows in the zero ring
        bf16x8 bfr[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          bfr[ks] = *reinterpret_cast<const bf16x8*>(P + pbase + (2 * mt - ky) * C3_PY + ks * 32);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma16x16x32(aw[(3 * ky + kx) * 4 + ks], bfr[ks], acc[kx]);
      }
      // da2 column x + kx; the lanes of column 7 open columns 8 (kx 1) and 9 (kx 2), which no earlier
      // tap of this image wrote: they add to zero instead of the previous image's value
      f32x4* d = reinterpret_cast<f32x4*>(DA + dbase + 20 * mt * C3_DARS);
      *d = acc[0];
#pragma unroll
      for (int kx = 1; kx < 3; ++kx) {
        asm volatile("" ::: "memory");  // the read below stays behind the other lanes' write above
        f32x4 old = d[kx * (C3_DARS / 4)];
        if (xcol == 7) old = zero_f32x4();
        d[kx * (C3_DARS / 4)] = old + acc[kx];
      }
    }
  };
  // pool2 + ReLU backward, one item per (output row y, channel quad), sliding along x: window (py, px)
  // covers outputs (py..py+1, px..px+1) and its one-hot code bit dy*2+dx names the one that receives
  // its gradient, so output (y, x) sums, in a fixed order, the windows (y, x), (y, x-1), (y-1, x),
  // (y-1, x-1) masked by code bits 0, 1, 2, 3.  Each window of a row is loaded once per item and used
  // for x and x+1; a missing window row (y = 0 or 10) reads a valid one under a mask of bit 4 (never set).
  const int gy = tid >> 4, gq = (tid & 15) * 4;
  const int rowA = min(gy, 9), rowB = max(gy - 1, 0);  // dy = 0 and dy = 1 window rows
  const int sA = gy <= 9 ? 0 : 4, sB = gy >= 1 ? 2 : 4;
  auto masked_add = [](f32x4& g, uint32_t cw, int sh, const f32x4& d) {
    const uint32_t m = (cw >> sh) & 0x01010101u;  // byte j = 1 iff channel j's window picked this output
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = fmaf(d[j], (float)((m >> (8 * j)) & 0xffu), g[j]);
  };
  C3Pre pre;
  int b = b_first;
  if (b < b_end) pre.load(src, idx3, b, tid);
  for (; b < b_end; b += b_step) {
    __syncthreads();  // previous image fully consumed (P, DA, AM)
    c3_expand(pre, tid, [&](int r) {
      const int w = r >> 2, i = r & 3;
      return P + (2 * (w >> 2) + (i >> 1) + 2) * C3_PY + (2 * (w & 3) + (i & 1)) * C3_PX;
    });
    codes_glds(idx2, b, AM, wave, lane);  // this image's codes land during the MFMA phase
    const int nb = b + b_step;
    if (nb < b_end) pre.load(src, idx3, nb, tid);
    __syncthreads();
    mfma_phase();
    c_dma_wait();
    __syncthreads();
    if (tid < 176) {
      const uint32_t* cA = reinterpret_cast<const uint32_t*>(AM + rowA * 640 + gq);
      const uint32_t* cB = reinterpret_cast<const uint32_t*>(AM + rowB * 640 + gq);
      const f32x4* dA = reinterpret_cast<const f32x4*>(DA + rowA * 10 * C3_DARS + gq);
      const f32x4* dB = reinterpret_cast<const f32x4*>(DA + rowB * 10 * C3_DARS + gq);
      bf16x4* dst = reinterpret_cast<bf16x4*>(dz2 + ((int64_t)b * 121 + gy * 11) * 64 + gq);
      uint32_t pa = 0, pb = 0;  // window (., x-1)
      f32x4 qa = zero_f32x4(), qb = zero_f32x4();
#pragma unroll
      for (int x = 0; x < 11; ++x) {
        uint32_t na = 0, nb2 = 0;
        f32x4 ea = zero_f32x4(), eb = zero_f32x4();
        if (x < 10) {
          na = cA[x * 16];
          nb2 = cB[x * 16];
          ea = dA[x * (C3_DARS / 4)];
          eb = dB[x * (C3_DARS / 4)];
        }
        f32x4 g = zero_f32x4();
        if (x < 10) masked_add(g, na, sA, ea);
        if (x > 0) masked_add(g, pa, sA + 1, qa);
        if (x < 10) masked_add(g, nb2, sB, eb);
        if (x > 0) masked_add(g, pb, sB + 1, qb);
        dst[x * 16] = bf16x4{(bf16)g[0], (bf16)g[1], (bf16)g[2], (bf16)g[3]};
        pa = na;
        pb = nb2;
        qa = ea;
        qb = eb;
      }
    }
  }
}

// wgrad: workgroup half h of an image slice covers n-tiles 18h..18h+17 of dW3t [576][128];
// wave (wm, wn) owns m-tiles (co) 4wm..4wm+3 x n-tiles 18h + 9wn .. +8.
__device__ __forceinline__ void conv3_wgrad_role(char* smem, const bf16* __restrict__ a2, const C3Src& src,
                                 const uint8_t* __restrict__ idx3, float* __restrict__ slabs, int B,
                                 int nslices, int slice, int h) {
  bf16* D = reinterpret_cast<bf16*>(smem);
  bf16* X = reinterpret_cast<bf16*>(smem + C3W_D);
  bf16* R = reinterpret_cast<bf16*>(smem + C3W_D + C3W_X);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nt0 = 18 * h + 9 * wn;
  const int g16 = lane & 15, grp = lane >> 4, q = g16 >> 2, p = g16 & 3;
  f32x4 acc[4][9];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = zero_f32x4();
  const int per = cdiv(B, nslices);
  const int b_lo = slice * per, b_hi = min(B, b_lo + per);
  C3Pre pre;
  if (b_lo < b_hi) {
    pre.load(src, idx3, b_lo, tid);
    a2_glds(a2, b_lo, R, wave, lane, 4);
  }
  for (int b = b_lo; b < b_hi; ++b) {
    c_dma_wait();
    __syncthreads();  // R has landed; the previous image's D / X reads are done
    c3_expand(pre, tid, [&](int r) { return D + r * C3_DRS; });
    a2_relayout(R, X, tid, 256);
    __syncthreads();  // D, X complete; R free
    if (b + 1 < b_hi) {  // lands during the MFMAs
      pre.load(src, idx3, b + 1, tid);
      a2_glds(a2, b + 1, R, wave, lane, 4);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kb = ks * 32 + grp * 8;
      bf16x8 af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m0 = (4 * wm + i) * 16;
        const bf16x4 lo = lds_read_tr16(D + (kb + q) * C3_DRS + m0 + 4 * p);
        const bf16x4 hi = lds_read_tr16(D + (kb + 4 + q) * C3_DRS + m0 + 4 * p);
        af[i] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
      const int x0 = win_pos(kb + q, 10), x1 = win_pos(kb + 4 + q, 10);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int n0 = (nt0 + j) * 16;  // n = tap*64 + ci
        const int tap = n0 >> 6, c0 = n0 & 63;
        const int shift = (tap / 3) * 10 + tap % 3;
        const bf16x4 lo = lds_read_tr16(X + (x0 + shift) * C3_XRS + c0 + 4 * p);
        const bf16x4 hi = lds_read_tr16(X + (x1 + shift) * C3_XRS + c0 + 4 * p);
        const bf16x8 bf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma16x16x32(af[i], bf, acc[i][j]);
      }
    }
  }
  float* slab = slabs + (int64_t)slice * C3_WSLAB;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = (4 * wm + i) * 16 + grp * 4;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int n = (nt0 + j) * 16 + g16;
      *reinterpret_cast<f32x4*>(slab + (int64_t)n * 128 + co) = acc[i][j];
    }
  }
}

// The small-batch launch (B <= fc_in_c3_max_batch; larger batches: conv3_bwd8_kernel below): workgroups
// [0, n_fc) run the fc1 backward (weight / bias gradient slabs only) and the conv3 roles form each image's
// compact gradient themselves (C3Pre::load): no fc1 backward launch.  The register budget is one workgroup's
// per SIMD (the compact-gradient load holds the fc1 weights in registers).
__global__ __launch_bounds__(256, 1) void conv3_bwd_kernel(const bf16* __restrict__ a2,
                                                           const uint8_t* __restrict__ idx2, C3Src src,
                                                           const uint8_t* __restrict__ idx3,
                                                           const bf16* __restrict__ packed, bf16* __restrict__ dz2,
                                                           int B, float* __restrict__ slabs, int n_wgrad,
                                                           int n_dgrad, int b_dgrad, int n_fc,
                                                           float* __restrict__ fc_slabs, int fc_n_imgs) {
  __shared__ __attribute__((aligned(16))) char smem[C3B_LDS];
  int blk = blockIdx.x;
  if (blk < n_fc) {
    if (src.dl)
      fc_bwd_body<false>(src.a3, packed, src.dl, nullptr, fc_slabs, B, fc_n_imgs, src.ce, blk);
    else
      fc_bwd_body<true>(src.a3, packed, nullptr, nullptr, fc_slabs, B, fc_n_imgs, src.ce, blk);
    return;
  }
  blk -= n_fc;
  int b_first = blk, b_end = b_dgrad, b_step = n_dgrad;
  if (blk >= n_dgrad) {
    const int w = blk - n_dgrad;
    conv3_wgrad_role(smem, a2, src, idx3, slabs, B, n_wgrad, w >> 1, w & 1);
    // images [b_dgrad, B) of the data gradient go to the wgrad workgroups once their slice is done: a
    // dgrad workgroup is slower per image than its wgrad neighbour (pool2 backward, barrier phases), so
    // with one of each per CU the wgrad half would otherwise idle (static split: deterministic)
    if (dz2 == nullptr || b_dgrad >= B) return;
    __syncthreads();  // LDS changes role
    b_first = b_dgrad + w;
    b_end = B;
    b_step = 2 * n_wgrad;
  }
  conv3_dgrad_role(smem, src, idx3, idx2, packed, dz2, b_first, b_end, b_step);  // one call site: inlined
}

// ---- conv3 backward with 8-wave workgroups (batches above fc_in_c3_max_batch: the fc1 backward launch
// leaves the compact gradient da3m).  One 512-thread workgroup per CU, in one of two roles:
//   dgrad, wave-specialised: waves 0-3 hold the conv3 weights and only run image s's dgrad MFMAs and
//     col2im (P[s&1] -> DA[s&1]); beside them the helper waves 4-7, one per SIMD, expand image s+1's
//     compact gradient (stage -> P) and run the pool2 + ReLU backward of image s-1 (DA, codes -> dz2), all
//     256 lanes: 16 runs of 8 or 7 consecutive output positions x 16 channel quads (c3_pool2_bwd).  Wave 7,
//     whose runs are the short ones, also issues the LDS-DMA of later images and waits for it with a vmcnt
//     that leaves its own 7 dz2 stores in flight.  The helper waves run at raised priority: each shares
//     its SIMD's issue port with an MFMA wave and is the one with the dependent chain.  One barrier per
//     image: every buffer is written in one step and read in the next, so P, DA, the codes and the compact
//     stage are double-buffered.  The 4-wave role above ran these phases one after the other, each behind
//     a barrier of all four waves.
//   wgrad: 8 waves cover the whole 128 x 576 dW3t of their image slice (36 tiles each, 2 x 4 waves), so
//     an image is staged once (the 4-wave role needs a workgroup pair, each staging every image); image
//     i+1's operands (compact gradient -> sparse-MFMA A fragments, a2 -> X by LDS-DMA straight into the padded
//     rows) are staged while image i's MFMAs run.  The window-ordered d(conv3) rows have one non-zero in every
//     aligned four (pool3 is 2x2, stride 2), so the product runs on v_smfmac_f32_16x16x64_bf16 straight from
//     the compact gradient and its argmax bytes: K = 64 in one instruction, half the dense role's MFMAs.
// All global -> LDS traffic is LDS-DMA from inline asm (invisible to the compiler's vmcnt bookkeeping),
// waited for explicitly before the barrier; the dz2 stores stay in flight across it.
// LDS layouts (every fragment read, col2im access and pool2 read modelled conflict-free with the lane
// groups of MI355X_MICROARCH.md; the 4-wave kernel's layouts measured 30-46 % bank-conflict cycles):
//   da2 (fp32): 256-B position rows, the 16-B chunk k of position (y, x) at slot k ^ 2(x & 7);
//   F (wgrad): the A operand in fragment order, per m-tile 64 lanes x 16 B of values, then 64 lanes x 4 B of
//     index words: lane-linear, one ds_read_b128 + one ds_read_b32 per m-tile;  the wgrad role's compact
//     stage: 16-B chunks XOR-swizzled inside each window by the copy's source offsets (c3w_stage_off), so that
//     the 2-byte / 1-byte gathers that build F meet no bank twice;  X (wgrad): a2 rows of 80 bf16 (10 16-B
//     chunks).
constexpr int C3S_B = 2048 * 2 + 2048;  // compact stage of one image: da3m row (bf16) + pool3 argmax bytes
constexpr int C3V_DA = 100 * 64 * 4;    // 25600
constexpr int C3V_FV = 8 * 64 * 16;     // 8192: A values of the 8 m-tiles
constexpr int C3V_F = C3V_FV + 8 * 64 * 4;  // 10240: + their index words
constexpr int C3V_XRS = 80;
constexpr int C3V_X = 100 * C3V_XRS * 2;  // 16000
constexpr int C3V_DG = 2 * (C3D_P + C3V_DA + C3D_AM + C3S_B);  // 131584
constexpr int C3V_WG = 3 * C3V_X + 2 * C3V_F + 2 * C3S_B;      // 80768
constexpr int C3V_LDS = C3V_DG > C3V_WG ? C3V_DG : C3V_WG;
static_assert(C3V_LDS <= 160 * 1024 && C3V_F % 16 == 0 && C3V_X % 16 == 0, "conv3 backward (8-wave) LDS");
// float offset of 16-B chunk k (channels 4k..4k+3) of da2 position p = y * 10 + x
__device__ __forceinline__ int c3v_da(int p, int x, int k) { return p * 64 + ((k ^ (2 * (x & 7))) << 2); }
// exact 0.0 / 1.0 of byte J of v (one v_cvt_f32_ubyteJ; the compiler's form of (v >> 8J) & 0xff was a shift,
// an and and v_cvt_f32_ubyte0 per byte)
template <int J>
__device__ __forceinline__ float ubyte_f32(uint32_t v) {
  float r;
  if constexpr (J == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(v));
  else if constexpr (J == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(v));
  else if constexpr (J == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(v));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(v));
  return r;
}

// v shifted right by N lanes inside each 16-lane DPP row (0 into the row's first N lanes)
template <int N>
__device__ __forceinline__ float dpp_row_shr(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + N, 0xf, 0xf, true));
}

// wave-instruction k (0..5) of the compact stage of image b: da3m row (4 KiB), then the argmax bytes (2 KiB)
__device__ __forceinline__ void c3s_glds(const bf16* __restrict__ da3m, const uint8_t* __restrict__ idx3, int b,
                                         char* S, int k, int lane) {
  const uint32_t voff = ((k & 3) * 64 + lane) * 16;
  if (k < 4)
    glds16_sv(da3m + (int64_t)b * 2048, voff, S + k * 1024);
  else
    glds16_sv(idx3 + (int64_t)b * 2048, voff, S + k * 1024);
}

__device__ __forceinline__ void c3s_pre(const char* S, int tid, C3Pre& p) {
  if (tid < 256) {
    p.da = reinterpret_cast<const bf16x8*>(S)[tid];
    p.id = reinterpret_cast<const uint2*>(S + 4096)[tid];
  }
}

// The wgrad role's compact stage.  Same copy as c3s_glds, but the 16-B chunks of a window change places: a lane's
// LDS slot is fixed (wave base + 16 * lane), its source offset is not.  Window w = 4g + r keeps its 256 B of
// values and 128 B of argmax bytes where they were; inside them value chunk c (channels 8c..8c+7) sits at slot
// c ^ 2g and argmax chunk m (channels 16m..16m+15) at slot m ^ g.  The lanes that build m-tile m's A fragments
// read channel 16m + lane % 16 of windows 4g + r, g = lane / 16: unswizzled, their four lane groups would meet
// 1024 B (values) or 512 B (bytes) apart, on the same banks.  c3w_stage_off: wave-instruction k's source offset.
__device__ __forceinline__ uint32_t c3w_stage_off(int k, int lane) {
  if (k < 4) return (k * 64 + (lane & ~15) + ((lane & 15) ^ (2 * k))) * 16;
  const int kk = k - 4;  // windows 8kk + lane / 8: g = 2kk + lane / 32
  return (kk * 64 + (lane & ~7) + ((lane & 7) ^ (2 * kk + (lane >> 5)))) * 16;
}
__device__ __forceinline__ void c3w_stage_glds(const bf16* __restrict__ da3m, const uint8_t* __restrict__ idx3, int b,
                                               char* S, int k, uint32_t voff) {
  if (k < 4)
    glds16_sv(da3m + (int64_t)b * 2048, voff, S + k * 1024);
  else
    glds16_sv(idx3 + (int64_t)b * 2048, voff, S + k * 1024);
}

// a2 image -> C3V_XRS rows by LDS-DMA: wave-instruction k (0..15) covers LDS chunks 64k..64k+63, 10 16-B
// chunks per row, chunks 8, 9 of a row its padding (re-reading the row's first chunks); a2_rows_off is a lane's
// byte offset in the image (or ~0u past the 100 rows), a2_glds_rows issues the copy of image b
__device__ __forceinline__ uint32_t a2_rows_off(int k, int lane) {
  const int c = k * 64 + lane;
  if (c >= 1000) return ~0u;
  const int row = c / 10, sub = c - 10 * row;
  return (row * 64 + (sub & 7) * 8) * 2;
}
__device__ __forceinline__ void a2_glds_rows(const bf16* __restrict__ a2, int b, bf16* X, int k, uint32_t voff) {
  if (voff != ~0u) glds16_sv(a2 + (int64_t)b * 6400, voff, X + k * 512);
}

// pool2 + ReLU backward of one image on the 256 lanes of the four helper waves (conv3_dgrad_role's expressions,
// from the swizzled da2 image).  The 121 output positions, row-major, are cut into 16 runs: runs 0-8 of 8
// positions, runs 9-15 of 7 (9 * 8 + 7 * 7 = 121); a lane owns one channel quad of one run, so no lane forms
// more than 8 outputs (a lane per output row formed 11, on 2.75 waves) and helper wave 3, which also issues
// the LDS-DMA, forms 7.  A run keeps the walk along the row: an output's (y, x - 1) and (y - 1, x - 1) terms
// are the da2 values and codes read for the output before it.  Everything that depends on the lane alone,
// C3Pool2Map, is worked out once per workgroup, so the walk costs no address arithmetic per image.
//   entry e = i + 1: what output i reads as its own column, (min(y, 9) | max(y - 1, 0), min(x, 9)); entry 0:
//     the column before output 0's.  An output outside a row's 10 da2 columns or rows reads a clamped, valid
//     address and masks the term with shift 4, a zero bit of every code byte (as the row clamps always did).
//     Where a run crosses into the next row, output x = 0 multiplies the last row's column-9 values by 0.0:
//     exact for finite gradients, which is all the kernels promise.
//   lanes: the 16 lanes of one ds_read_b128 lane group (MI355X: {0-3,12-15,20-27}, {4-11,16-19,28-31} of each
//     32) share a run and take its 16 channel quads, so every da2 read covers one 256-B position row: no bank
//     conflict whatever the runs' columns are.
struct C3Pool2Map {
  int dst;              // bf16 offset of output 0 in the image's dz2
  int daA[9], daB[9];   // float offsets into the da2 image, rows min(y, 9) and max(y - 1, 0)
  int amA[9], amB[9];   // byte offsets into the pool2 codes, same rows
  int sh[8][4];         // code bit of the window terms (y,x), (y,x-1), (y-1,x), (y-1,x-1), or 4
  bool eight;           // the run has an 8th output
};
__device__ __forceinline__ void c3_pool2_map(int hwave, int lane, C3Pool2Map& m) {
  const int q = (lane >> 2) & 7;
  const int run = 4 * hwave + 2 * (lane >> 5) + (__builtin_popcount(q) & 1), k = (q >> 1) * 4 + (lane & 3);
  const int p0 = run < 9 ? 8 * run : 7 * run + 9;
  m.eight = run < 9;
  m.dst = p0 * 64 + k * 4;
  int gy = p0 / 11, x = p0 - 11 * gy;
  auto entry = [&](int e, int xc) {
    const int rowA = min(gy, 9), rowB = max(gy - 1, 0);
    m.daA[e] = c3v_da(rowA * 10 + xc, xc, k);
    m.daB[e] = c3v_da(rowB * 10 + xc, xc, k);
    m.amA[e] = rowA * 640 + xc * 64 + k * 4;
    m.amB[e] = rowB * 640 + xc * 64 + k * 4;
  };
  entry(0, max(x - 1, 0));
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    entry(i + 1, min(x, 9));
    const int sA = gy <= 9 ? 0 : 4, sB = gy >= 1 ? 2 : 4;
    m.sh[i][0] = x < 10 ? sA : 4;
    m.sh[i][1] = x > 0 ? sA + 1 : 4;
    m.sh[i][2] = x < 10 ? sB : 4;
    m.sh[i][3] = x > 0 ? sB + 1 : 4;
    if (++x == 11) {
      x = 0;
      ++gy;
    }
  }
}
// dz2_img: the image's dz2.  The lane's stores: 8 (7 when !m.eight), one global_store_dwordx2 each.
__device__ __forceinline__ void c3_pool2_bwd(const C3Pool2Map& m, const float* DA, const uint8_t* AM,
                                             bf16* __restrict__ dz2_img) {
  auto masked_add = [](f32x4& g, uint32_t cw, int sh, const f32x4& d) {
    const uint32_t mk = (cw >> sh) & 0x01010101u;
    g[0] = fmaf(d[0], ubyte_f32<0>(mk), g[0]);
    g[1] = fmaf(d[1], ubyte_f32<1>(mk), g[1]);
    g[2] = fmaf(d[2], ubyte_f32<2>(mk), g[2]);
    g[3] = fmaf(d[3], ubyte_f32<3>(mk), g[3]);
  };
  auto code = [&](int off) { return *reinterpret_cast<const uint32_t*>(AM + off); };
  auto da2 = [&](int off) { return *reinterpret_cast<const f32x4*>(DA + off); };
  bf16x4* dst = reinterpret_cast<bf16x4*>(dz2_img + m.dst);
  uint32_t pa = code(m.amA[0]), pb = code(m.amB[0]);
  f32x4 qa = da2(m.daA[0]), qb = da2(m.daB[0]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i == 7 && !m.eight) break;
    const uint32_t na = code(m.amA[i + 1]), nb2 = code(m.amB[i + 1]);
    const f32x4 ea = da2(m.daA[i + 1]), eb = da2(m.daB[i + 1]);
    f32x4 g = zero_f32x4();
    masked_add(g, na, m.sh[i][0], ea);
    masked_add(g, pa, m.sh[i][1], qa);
    masked_add(g, nb2, m.sh[i][2], eb);
    masked_add(g, pb, m.sh[i][3], qb);
    // nontemporal: dz2 (15.5 KB per image, read once by the conv12 backward) streams past the Infinity Cache
    // (B=65536: this kernel 927 -> 915 us, conv12_bwd8_kernel unchanged; profiles/r15/head_bytes/README.md)
    __builtin_nontemporal_store(bf16x4{(bf16)g[0], (bf16)g[1], (bf16)g[2], (bf16)g[3]}, &dst[i * 16]);
    pa = na;
    pb = nb2;
    qa = ea;
    qb = eb;
  }
}
constexpr int C3_POOL2_DMA_WAVE_STORES = 7;  // dz2 stores per image of helper wave 3 (runs 12-15)

// RINGDP_C3_ABLATE (diagnostic builds only, tools/build_variant.py; timing only, wrong results): bit 0 skips the
// pool2 backward of the 8-wave conv3 backward, bit 1 its dgrad MFMA phase, bit 2 its weight gradient.  A
// compile-time constant, 0 in every normal build: nothing reads the environment for it and no launch argument
// can select it.
#ifndef RINGDP_C3_ABLATE
#define RINGDP_C3_ABLATE 0
#endif
constexpr int C3_ABLATE = RINGDP_C3_ABLATE;

// RINGDP_C3_STAMPS (diagnostic builds only, tools/build_variant.py): lane 0 of every wave of the 8-wave dgrad
// role records s_memtime at 4 phase points of steps [C3_ST_S0, C3_ST_S0 + 8) into LDS past C3V_LDS; workgroup
// C3_ST_BLK prints them at the end, relative to wave 0's step start.  MFMA waves: 0 step start, 1 last MFMA
// group issued, 2 col2im stored, 3 past the barrier; helper waves: 0 expand done, 1 pool2 done, 2 LDS-DMA
// waited for, 3 past the barrier.
#ifdef RINGDP_C3_STAMPS
constexpr int C3_ST_S0 = 100, C3_ST_BLK = 5, C3_ST_BYTES = 8 * 8 * 4 * 8;
#define C3_ST(k) CN_STAMP(C3V_LDS, C3_ST_S0, 4, s, k)
#else
constexpr int C3_ST_BYTES = 0;
#define C3_ST(k) do {} while (0)
#endif

__device__ __forceinline__ void conv3_dgrad8_role(char* smem, const bf16* __restrict__ da3m,
                                                  const uint8_t* __restrict__ idx3, const uint8_t* __restrict__ idx2,
                                                  const bf16* __restrict__ packed, bf16* __restrict__ dz2, int b_first,
                                                  int b_end, int b_step) {
  auto Pb = [&](int k) { return reinterpret_cast<bf16*>(smem + k * C3D_P); };
  auto DAb = [&](int k) { return reinterpret_cast<float*>(smem + 2 * C3D_P + k * C3V_DA); };
  // pool2 codes of image j in AM[j & 1], issued in step j (pool2 of image j runs in step j+1)
  auto AMb = [&](int k) { return reinterpret_cast<uint8_t*>(smem + 2 * (C3D_P + C3V_DA) + k * C3D_AM); };
  auto Sb = [&](int k) { return smem + 2 * (C3D_P + C3V_DA + C3D_AM) + k * C3S_B; };
  auto codes_dma = [&](int j, int lane) {
    const uint8_t* src = idx2 + (int64_t)(b_first + j * b_step) * 6400;
    uint8_t* AM = AMb(j & 1);
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k * 64 + lane < 400) glds16_sv(src, (k * 64 + lane) * 16, AM + k * 1024);
  };
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = b_first < b_end ? (b_end - b_first + b_step - 1) / b_step : 0;
  // the zero rows of both dz3 images stay zero; the interiors are rewritten per image
  for (int c = tid; c < 2 * C3D_P / 16; c += 512) reinterpret_cast<bf16x8*>(smem)[c] = zero_bf16x8();
  if (wave < 4) {
    // ---- MFMA waves: wave w owns input channels 16w..16w+15 (as conv3_dgrad_role)
    const int r16 = lane & 15, q8 = (lane >> 4) * 8, c4 = (lane >> 4) * 4;
    const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed + P3D_OFF);
    bf16x8 aw[36];
#pragma unroll
    for (int j = 0; j < 36; ++j) aw[j] = pk[(wave * 36 + j) * 64 + lane];
    const int pbase = ((r16 >> 3) + 2) * C3_PY + (r16 & 7) * C3_PX + q8;
    const int xcol = r16 & 7, chunk = 4 * wave + (c4 >> 2);
    // da2 targets of m-tile 0: (row r16 >> 3, column xcol); lanes of column 7 also columns 8 and 9
    const int dcol = c3v_da((r16 >> 3) * 10 + xcol, xcol, chunk);
    const int dc8 = c3v_da((r16 >> 3) * 10 + 8, 8, chunk), dc9 = c3v_da((r16 >> 3) * 10 + 9, 9, chunk);
    lds_barrier();  // [B0] zero rows
    lds_barrier();  // [B1] image 0 expanded
    for (int s = 0; s <= n; ++s) {
      C3_ST(0);
      if (s < n && !(C3_ABLATE & 2)) {
        const bf16* P = Pb(s & 1);
        float* DA = DAb(s & 1);
        // the 13 (m-tile, ky) groups with a non-zero dz3 row, in order; group g+1's 4 B fragments are read
        // while group g's 12 MFMAs run (the reads issued right before their MFMAs had exposed ~100 cycles per
        // group)
        constexpr int NG = 13;
        auto gmt = [](int g) { return g < 2 ? 0 : (g < 11 ? (g - 2) / 3 + 1 : 4); };
        auto gky = [](int g) { return g < 2 ? g : (g < 11 ? (g - 2) % 3 : g - 10); };
        auto readB = [&](int g, bf16x8 (&b)[4]) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            b[ks] = *reinterpret_cast<const bf16x8*>(P + pbase + (2 * gmt(g) - gky(g)) * C3_PY + ks * 32);
        };
        bf16x8 bfa[4], bfb[4];
        readB(0, bfa);
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int mt = gmt(g), ky = gky(g);
          bf16x8(&bcur)[4] = (g & 1) ? bfb : bfa;
          bf16x8(&bnxt)[4] = (g & 1) ? bfa : bfb;
          if (g + 1 < NG) readB(g + 1, bnxt);
          if (g == 0 || gmt(g - 1) != mt) acc[0] = acc[1] = acc[2] = zero_f32x4();
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma16x16x32(aw[(3 * ky + kx) * 4 + ks], bcur[ks], acc[kx]);
          if (g + 1 < NG && gmt(g + 1) == mt) continue;
          if (g + 1 == NG) C3_ST(1);
          // col2im along the row in registers: da2(x) = acc0(x) + acc1(x-1) + acc2(x-2), the shifted terms
          // by DPP row shifts inside each 16-lane group (= 2 dz3 rows x 8 columns; a term that would cross
          // into the next row is zeroed at its source lane); column 8 = acc1(7) + acc2(6), column 9 =
          // acc2(7) go out from the column-7 lanes.  One plain store per target, no read-add-write.
          f32x4 out, e8;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float a1 = xcol == 7 ? 0.f : acc[1][j], a2 = xcol >= 6 ? 0.f : acc[2][j];
            out[j] = (acc[0][j] + dpp_row_shr<1>(a1)) + dpp_row_shr<2>(a2);
            e8[j] = acc[1][j] + dpp_row_shr<1>(acc[2][j]);
          }
          *reinterpret_cast<f32x4*>(DA + dcol + 20 * mt * 64) = out;
          if (xcol == 7) {
            *reinterpret_cast<f32x4*>(DA + dc8 + 20 * mt * 64) = e8;
            *reinterpret_cast<f32x4*>(DA + dc9 + 20 * mt * 64) = acc[2];
          }
        }
      }
      C3_ST(2);
      lds_barrier();
      C3_ST(3);
    }
  } else {
    // ---- VALU waves: thread vt of 256; wave 7 issues every LDS-DMA: it has the fewest pool2 outputs, and
    // its dz2 stores of a step all follow that step's DMAs, so a vmcnt that leaves exactly those stores out
    // (memory operations of one wave retire in order) waits for the DMAs alone
    const int vt = tid - 256;
    const bool dma = wave == 7;
    C3Pool2Map pmap;
    c3_pool2_map(wave - 4, lane, pmap);
    // The helper waves go first at their SIMD's issue port.  An MFMA wave keeps the port busy with long
    // matrix instructions that it can issue back to back; at equal priority the helper wave beside it got
    // what was left, trailed its MFMA wave by 1200 cycles per image and set the step (stamps:
    // profiles/r07/c3_dgrad/stamps.md).  Ahead of it, both finish together, 5 % sooner.
    __builtin_amdgcn_s_setprio(2);
    auto row_ptr = [&](bf16* P) {
      return [P](int r) {
        const int w = r >> 2, i = r & 3;
        return P + (2 * (w >> 2) + (i >> 1) + 2) * C3_PY + (2 * (w & 3) + (i & 1)) * C3_PX;
      };
    };
    if (dma && n > 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c3s_glds(da3m, idx3, b_first, Sb(0), k, lane);
      if (n > 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) c3s_glds(da3m, idx3, b_first + b_step, Sb(1), k, lane);
      }
      c_dma_wait();
    }
    lds_barrier();  // [B0]
    if (n > 0) {
      C3Pre pre;
      c3s_pre(Sb(0), vt, pre);
      c3_expand(pre, vt, row_ptr(Pb(0)));
    }
    lds_barrier();  // [B1]
    for (int s = 0; s <= n; ++s) {
      if (dma) {
        if (s + 2 < n) {
#pragma unroll
          for (int k = 0; k < 6; ++k) c3s_glds(da3m, idx3, b_first + (s + 2) * b_step, Sb(s & 1), k, lane);
        }
        if (s < n) codes_dma(s, lane);
      }
      if (s + 1 < n) {
        C3Pre pre;
        c3s_pre(Sb((s + 1) & 1), vt, pre);
        c3_expand(pre, vt, row_ptr(Pb((s + 1) & 1)));
      }
      C3_ST(0);
      const bool pool = s >= 1 && !(C3_ABLATE & 1);
      if (pool) {
        // the buffer as a constant: the precomputed offsets then meet it in the reads' immediate fields
        bf16* dz2_img = dz2 + (int64_t)(b_first + (s - 1) * b_step) * (121 * 64);
        if ((s - 1) & 1)
          c3_pool2_bwd(pmap, DAb(1), AMb(1), dz2_img);
        else
          c3_pool2_bwd(pmap, DAb(0), AMb(0), dz2_img);
      }
      C3_ST(1);
      // (issuing image s+1's codes a step earlier and leaving them in flight measured slower)
      if (dma) {
        if (pool)
          c_dma_wait_but<C3_POOL2_DMA_WAVE_STORES>();
        else
          c_dma_wait();
      }
      C3_ST(2);
      lds_barrier();
      C3_ST(3);
    }
    __builtin_amdgcn_s_setprio(0);
  }
}

__device__ __forceinline__ void conv3_wgrad8_role(char* smem, const bf16* __restrict__ a2, const bf16* __restrict__ da3m,
                                                  const uint8_t* __restrict__ idx3, float* __restrict__ slabs, int B,
                                                  int nslices, int slice) {
  // three X image buffers: image i computes from buffer i % 3 while image i+2 is staged into (i+2) % 3; two F
  // buffers: image i+1's A fragments are read into registers (from F[(i+1) & 1]) while image i computes, and
  // image i+2's are built into F[i & 1], which image i left before the barrier that ended image i-1
  auto Xb = [&](int k) { return reinterpret_cast<bf16*>(smem + k * C3V_X); };
  auto Fb = [&](int k) { return smem + 3 * C3V_X + k * C3V_F; };
  auto Sb = [&](int k) { return smem + 3 * C3V_X + 2 * C3V_F + k * C3S_B; };
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wave (wm, wn): m-tiles (co) 4wm..4wm+3 x n-tiles 4j + wn (j < 9), n = tap*64 + ci, i.e. tap j and channels
  // 16wn..16wn+15: the tap part of every X address is then an immediate offset
  const int wm = wave & 1, wn = wave >> 1;
  const int g16 = lane & 15, grp = lane >> 4, q = g16 >> 2, p = g16 & 3;
  f32x4 acc[4][9];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = zero_f32x4();
  // images slice, slice + nslices, ...: the dgrad workgroups stride the batch the same way, so with both counts
  // multiples of 8 an image's two readers of the compact gradient run on one XCD at about the same time
  const int n = slice < B ? (B - slice + nslices - 1) / nslices : 0;
  auto img = [&](int i) { return slice + i * nslices; };
  // this wave's a2 DMA instructions: k = wave, wave + 8; its compact-stage instruction: k = wave (waves 0-5)
  const uint32_t xo0 = a2_rows_off(wave, lane), xo1 = a2_rows_off(wave + 8, lane);
  const uint32_t so = c3w_stage_off(wave < 6 ? wave : 0, lane);
  auto dma_x = [&](int b, bf16* X) {
    a2_glds_rows(a2, b, X, wave, xo0);
    a2_glds_rows(a2, b, X, wave + 8, xo1);
  };
  auto dma_s = [&](int b, char* S) {
    if (wave < 6) c3w_stage_glds(da3m, idx3, b, S, wave, so);
  };
  // A operand of one image, compact stage -> F: thread (m-tile mt = wave, lane) forms the fragment and index word
  // that lane `lane` of the MFMA waves feeds for m-tile mt.  Row co = 16 mt + lane % 16; the lane group g = lane / 16
  // covers dense rows k = 16g..16g+15 of the window-ordered d(conv3), i.e. windows w = 4g + r (k = 4w + argmax):
  // slot 2r = da3m[w][co], slot 2r+1 = 0 (a zero-extended 16-bit read is that pair), index field 2r = argmax[w][co].
  // A dead window (a3 <= 0) has value 0 in both slots.
  const int sv = grp * 1024 + (((2 * wave + (g16 >> 3)) ^ (2 * grp)) * 16) + (g16 & 7) * 2;  // + 256 r
  const int si = 4096 + grp * 512 + ((wave ^ grp) * 16) + g16;                              // + 128 r
  auto expand = [&](const char* S, char* F) {
    uint32_t v[4], a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = *reinterpret_cast<const uint16_t*>(S + sv + 256 * r);
      a[r] = *reinterpret_cast<const uint8_t*>(S + si + 128 * r);
    }
    *reinterpret_cast<uint4*>(F + (wave * 64 + lane) * 16) = make_uint4(v[0], v[1], v[2], v[3]);
    // bits 0-1 of each byte, as c3_rows reads them
    *reinterpret_cast<uint32_t*>(F + C3V_FV + (wave * 64 + lane) * 4) =
        (a[0] | (a[1] << 4) | (a[2] << 8) | (a[3] << 12)) & 0x3333u;
  };
  auto readA = [&](int buf, bf16x8 (&af)[4], int (&ix)[4]) {
    const char* F = Fb(buf) + (4 * wm * 64 + lane) * 16;
    const char* I = Fb(buf) + C3V_FV + (4 * wm * 64 + lane) * 4;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      af[mi] = *reinterpret_cast<const bf16x8*>(F + mi * 1024);
      ix[mi] = *reinterpret_cast<const int*>(I + mi * 256);
    }
  };
  if (n > 0) {  // prologue: images 0 and 1 staged, image 2's compact gradient in S0
    dma_s(img(0), Sb(0));
    if (n > 1) dma_s(img(1), Sb(1));
    dma_x(img(0), Xb(0));
    if (n > 1) dma_x(img(1), Xb(1));
    c_dma_wait();
    lds_barrier();
    expand(Sb(0), Fb(0));
    if (n > 1) expand(Sb(1), Fb(1));
    lds_barrier();  // S0, S1 free
    if (n > 2) dma_s(img(2), Sb(0));
    c_dma_wait();
  }
  lds_barrier();
  bf16x8 afa[4], afb[4];
  int ixa[4], ixb[4];
  if (n > 0) readA(0, afa, ixa);
  lds_barrier();  // every wave holds image 0's fragments: F0 may be rebuilt
  // one image: af / ix are its A fragments, afn / ixn receive the next image's
  auto image = [&](int i, const bf16x8 (&af)[4], const int (&ix)[4], bf16x8 (&afn)[4], int (&ixn)[4]) {
    const int cur = i % 3;
    const int st = (i + 2) % 3;  // staging buffer of image i+2
    if (i + 2 < n) dma_x(img(i + 2), Xb(st));
    if (i + 3 < n) dma_s(img(i + 3), Sb((i + 1) & 1));
    const int xb = (int)(Xb(cur) - reinterpret_cast<const bf16*>(smem)) + 16 * wn + 4 * p;  // element offset
    // B: the lane group's 16 rows are k = 8 grp .. + 7 and 32 + 8 grp .. + 7, the a2 positions of windows 2 grp,
    // 2 grp + 1 and, four image rows (40 positions) below them, 8 + 2 grp, 8 + 2 grp + 1
    int x0 = xb + win_pos(grp * 8 + q, 10) * C3V_XRS, x1 = xb + win_pos(grp * 8 + 4 + q, 10) * C3V_XRS;
    // the whole per-lane part of the address opaque to the optimiser: otherwise it folds the tap offset into
    // a per-tap SGPR or VGPR and pays one VALU add per fragment read instead of the immediate offset
    asm("" : "+v"(x0), "+v"(x1));
    const bf16* S0 = reinterpret_cast<const bf16*>(smem);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int shift = ((j / 3) * 10 + j % 3) * C3V_XRS;  // tap j
      const bf16x4 b0 = lds_read_tr16(S0 + x0 + shift);
      const bf16x4 b1 = lds_read_tr16(S0 + x1 + shift);
      const bf16x4 b2 = lds_read_tr16(S0 + x0 + shift + 40 * C3V_XRS);
      const bf16x4 b3 = lds_read_tr16(S0 + x1 + shift + 40 * C3V_XRS);
      const bf16x16 bf = bf16x16{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3],
                                 b2[0], b2[1], b2[2], b2[3], b3[0], b3[1], b3[2], b3[3]};
      if (j == 2 && i + 2 < n) expand(Sb(i & 1), Fb(i & 1));  // image i+2's A operand
      if (j == 5 && i + 1 < n) readA((i + 1) & 1, afn, ixn);  // image i+1's: its buffer is complete
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) acc[mi][j] = smfmac16x16x64(af[mi], bf, acc[mi][j], ix[mi]);
    }
    // (letting image i+2's a2 copies stay in flight across the barrier measured 50 us slower)
    c_dma_wait();
    lds_barrier();
  };
  for (int i = 0; i < n; i += 2) {  // two images per trip: the fragment registers swap roles without moves
    image(i, afa, ixa, afb, ixb);
    if (i + 1 < n) image(i + 1, afb, ixb, afa, ixa);
  }
  float* slab = slabs + (int64_t)slice * C3_WSLAB;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int co = (4 * wm + mi) * 16 + grp * 4;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int nn = (4 * j + wn) * 16 + g16;
      *reinterpret_cast<f32x4*>(slab + (int64_t)nn * 128 + co) = acc[mi][j];
    }
  }
}

// blocks [0, n_dgrad): dgrad of images [0, b_dgrad) (strided); then n_wgrad wgrad slices, whose workgroups
// go on to the dgrad of images [b_dgrad, B) (static split: deterministic)
__global__ __launch_bounds__(512, 1) void conv3_bwd8_kernel(const bf16* __restrict__ a2, const uint8_t* __restrict__ idx2,
                                                           const bf16* __restrict__ da3m, const uint8_t* __restrict__ idx3,
                                                           const bf16* __restrict__ packed, bf16* __restrict__ dz2,
                                                           int B, float* __restrict__ slabs, int n_wgrad, int n_dgrad,
                                                           int b_dgrad) {
  __shared__ __attribute__((aligned(16))) char smem[C3V_LDS + C3_ST_BYTES];
  const int blk = blockIdx.x;
  if (blk < n_dgrad) {
    conv3_dgrad8_role(smem, da3m, idx3, idx2, packed, dz2, blk, b_dgrad, n_dgrad);
#ifdef RINGDP_C3_STAMPS
    __syncthreads();
    if (blk == C3_ST_BLK && threadIdx.x == 0 && (b_dgrad - blk) / n_dgrad > C3_ST_S0 + 8) {
      const unsigned long long* st = reinterpret_cast<const unsigned long long*>(smem + C3V_LDS);
      for (int w = 0; w < 8; ++w)
        for (int k = 0; k < 8; ++k) {
          const unsigned long long* r = st + (w * 8 + k) * 4;
          const unsigned long long t0 = st[k * 4];  // wave 0's step start
          printf("C3ST w%d s%d %lld %lld %lld %lld\n", w, k, (long long)(r[0] - t0), (long long)(r[1] - t0),
                 (long long)(r[2] - t0), (long long)(r[3] - t0));
        }
    }
#endif
    return;
  }
  const int w = blk - n_dgrad;
  if (!(C3_ABLATE & 4)) conv3_wgrad8_role(smem, a2, da3m, idx3, slabs, B, n_wgrad, w);
  if (dz2 == nullptr || b_dgrad >= B) return;
  __syncthreads();  // LDS changes role
  conv3_dgrad8_role(smem, da3m, idx3, idx2, packed, dz2, b_dgrad + w, B, n_wgrad);
}

}  // namespace

// Work split of the role-fused backward launches.  All blocks of a launch are co-resident (one
// 512-thread block per CU), so dgrad and wgrad blocks are sized to finish together.
// RINGDP_C*_DGRAD_FRAC override the measured fraction of the CUs given to the dgrad role (tuning sweeps),
// RINGDP_C*_WMIN the fewest images per weight-gradient slab (small batches: more slabs = more reduction traffic).
// conv3, 8-wave kernel: a dgrad image is 624 MFMAs plus the pool2 backward, about 5300 cycles of a workgroup; a
// wgrad image is 288 sparse MFMAs, about 2700 (3900 as 576 dense ones), so the dgrad role gets two CUs in three.
// B=65536, conv3 + fc1 backward, two interleaved passes: 1077-1080 us at 0.66, 1164-1173 at the dense role's
// 0.55, 1085-1111 at 0.59-0.63, 1068-1079 at 0.69 without the steal (profiles/r10/c3_wgrad_sparse/README.md).
// conv3, 4-wave kernel: dgrad and wgrad do about the same MFMA work per image (624 / 576 MFMAs); measured best
// split 0.5-0.6 of the workgroup slots (B=32768, when it still served that batch).
static void c3_split(int B, bool dgrad, int& nd, int& ws) {
  if (use_8wave(B)) {  // one 512-thread workgroup per CU; ws = wgrad slices, one workgroup each
    const int cus = num_cus();
    static const double frac = env_real("RINGDP_C3_DGRAD_FRAC", 0.66, split_frac_ok);
    nd = clampi(((int)(frac * cus) + 4) / 8 * 8, 8, cus - 8);  // multiples of 8: see conv3_wgrad8_role
    ws = clampi(cdiv(B, 8), 1, cus - nd);
    // Without a data gradient the same slices, on as many workgroups, and no dgrad workgroups: a slice is a
    // slab and fixes the fp32 order in which dW3 and db3 are summed, so the weight gradients of a call do not
    // depend on whether it also asks for dz2 (byte-equal; one slice per CU would sum in another order).  The
    // CUs the dgrad role would have had stay idle in such a call.
    if (!dgrad) nd = 0;
    return;
  }
  // 256-thread workgroups, two per CU; ws = image slices, each served by a pair of workgroups
  const int slots = 2 * num_cus();
  if (!dgrad) {
    nd = 0;
    ws = clampi(cdiv(B, 8), 1, slots / 2);
    return;
  }
  static const double frac = env_real("RINGDP_C3_DGRAD_FRAC", 0.5, split_frac_ok);
  static const int wmin = env_int("RINGDP_C3_WMIN", 2, slab_images_ok);
  nd = clampi(B, 1, (int)(frac * slots));
  const int per = cdiv(B, nd);
  ws = clampi(cdiv(B, std::max(per, wmin)), 1, std::max(1, (slots - nd) / 2));  // >= wmin images per slab
}

// Images [0, result) of the conv3 data gradient run on the dgrad workgroups, the rest on the wgrad
// workgroups after their weight-gradient slice (RINGDP_C3_STEAL = that share; large batches only, where
// each dgrad workgroup has many images).  The share evens out what the 8-workgroup steps of the split leave:
// with the sparse weight gradient and 0.66 of the CUs on the dgrad role, conv3 + fc1 backward at B=65536 is flat
// within its run-to-run spread (about 13 us) from 0.01 to 0.04: 1083-1089 us at 0.01, 1071-1084 at 0.02, 1077-1080
// at 0.04, 1082-1096 without (profiles/r10/c3_wgrad_sparse/README.md), so 0.04 stays.  It had been fitted to the
// dense role at 0.55 (profiles/r07/c3_dgrad/README.md), and 0.07 / 0.1 to the roles before that
// (profiles/r06/c3_steal_sweep.txt).
static int c3_dgrad_images(int B, int nd) {
  static const double steal = env_real("RINGDP_C3_STEAL", 0.04, [](double f) { return f >= 0.0 && f < 0.9; });
  if (nd <= 0 || B < 32 * nd) return B;
  return B - (int)(steal * B);
}

// images per fc1-backward workgroup (RINGDP_CN_FC_IMGS overrides the table for A/B runs)
static int fc_imgs_host(int B) {
  static const int forced = env_int("RINGDP_CN_FC_IMGS", 0);  // unset, empty, 0 or negative: the table
  return forced > 0 ? std::min(forced, 128) : fc_imgs(B);  // <= 128: the CE logits-gradient LDS block
}
int64_t cn_fc_slab_floats(int B, bool) { return (int64_t)cdiv(B, fc_imgs_host(B)) * FC_SLAB; }
int64_t cn_conv3_slab_floats(int B, bool dgrad) {
  int nd, ws;
  c3_split(B, dgrad, nd, ws);
  return (int64_t)ws * C3_WSLAB;
}

void cn_conv3_fc_bwd(const void* a2, const uint8_t* idx2, const void* a3, const uint8_t* idx3, const float* wfc,
                     const float* dl, const void* packed, void* da3m, void* dz2, int B, float* fc_slabs,
                     float* c3_slabs, float* dw3, float* db3, float* dwfc, float* dbfc, hipStream_t s,
                     const CeFuse* ce, ReduceList* defer) {
  (void)wfc;  // the data gradient uses the packed bf16 copy, like every other dgrad
  int nd, ws;
  c3_split(B, dz2 != nullptr, nd, ws);
  const int fs = cdiv(B, fc_imgs_host(B));
  const bf16 *a3b = static_cast<const bf16*>(a3), *pk = static_cast<const bf16*>(packed);
  const CeFuse cef = ce ? *ce : CeFuse{};
  if (!use_8wave(B)) {  // fc1 backward inside the conv3 backward launch
    const C3Src src{a3b, pk, ce ? nullptr : dl, cef};
    conv3_bwd_kernel<<<fs + nd + 2 * ws, 256, 0, s>>>(static_cast<const bf16*>(a2), idx2, src, idx3, pk,
                                                       static_cast<bf16*>(dz2), B, c3_slabs, ws, nd,
                                                       c3_dgrad_images(B, nd), fs, fc_slabs, fc_imgs_host(B));
  } else {
    // Second pass over a3 after fc1_fwd_kernel, in the same direction.  Opposite directions (this launch by
    // descending image group, or fc1_fwd_kernel descending by workgroup and by group inside it) measured no
    // different at B=65536: both launches are 512 workgroups, all resident at once (2 per CU), so the order of
    // workgroups is no order in time, and the order of images inside a workgroup here is the order of the
    // fp32 sums (profiles/r15/head_bytes/README.md).
    if (ce)
      fc_bwd_kernel<true><<<fs, 256, 0, s>>>(a3b, pk, nullptr, static_cast<bf16*>(da3m), fc_slabs, B, fc_imgs_host(B), cef);
    else
      fc_bwd_kernel<false><<<fs, 256, 0, s>>>(a3b, pk, dl, static_cast<bf16*>(da3m), fc_slabs, B, fc_imgs_host(B), cef);
    conv3_bwd8_kernel<<<nd + ws, 512, 0, s>>>(static_cast<const bf16*>(a2), idx2, static_cast<const bf16*>(da3m), idx3,
                                             pk, static_cast<bf16*>(dz2), B, c3_slabs, ws, nd, c3_dgrad_images(B, nd));
  }
  ReduceList r{seg(c3_slabs, C3_WSLAB, 0, 576 * 128, ws, dw3, 1, 64, 128),
               seg(fc_slabs, FC_SLAB, 20490, 128, fs, db3), seg(fc_slabs, FC_SLAB, 0, 20480, fs, dwfc, 2),
               seg(fc_slabs, FC_SLAB, 20480, 10, fs, dbfc)};
  if (defer)
    defer->insert(defer->end(), r.begin(), r.end());
  else
    launch_reduce(r, s);
}

}  // namespace ringdp::kern
