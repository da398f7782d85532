// Random-resized-crop + bilinear resize for the device loader on gfx950, hipGraph-safe: what feeds a ViT at 224^2 or
// 384^2 from an HBM-resident uint8 dataset of small images (torchvision RandomResizedCrop -> RandomHorizontalFlip ->
// ToTensor -> Normalize -> RandomErasing(value=0)).
//
//  * crop_draw_kernel    one thread per record: the crop box, the flip and the erase box of one sample
//  * resize_crop_kernel  out[b] = the box of x[idx[b]] resized to S x S (bilinear, half-pixel centres, source indices
//                        clamped to the box, no antialiasing), mirrored, normalised, zeroed inside the erase box and
//                        rounded once to fp32 / bf16; yout[b] = labels[idx[b]]
//
// Record (int32 [8]): 0..3 crop box y0 x0 h w in source pixels, 4 flip, 5 erase rows ey0 | ey1 << 16, 6 erase columns
// ex0 | ex1 << 16 (half-open, output coordinates, empty = no erase), 7 zero.
//
// Draws: Philox4x32-10 of the (seed, step) snapshot, key = seed, counter = (record, step lo, step hi, round), uniforms
// (word >> 8) * 2^-24, all arithmetic fp32.  Round t of 0..9 is crop attempt t: w0 area, w1 log-ratio, w2 / w3 the
// position y0 / x0; the first attempt whose box fits is taken, and if none fits, torchvision's centre crop with the
// ratio clamped.  Round 10: w0 flip, w1 erase.  Round 11 + t of 11..20 is erase attempt t with the same word use.
// Both loops are bounded, a record never reads another, and nothing is written but the record.
//
// resize_crop_kernel, per workgroup of 256 threads = one sample and a band of kBandRows output rows (workgroup id =
// sample * bands + band, so one sample's bands run next to each other and share its source in L2):
//   1. stage the source rows the band touches into LDS as uint8.  They are one contiguous byte range of the dataset,
//      copied with 16-byte loads from the 16-byte-aligned address below its start (the first and last chunk fall back
//      to bytes where they would leave the dataset); every later source read is an LDS byte read, and at a 7-12x
//      upscale neighbouring lanes read the same bytes (a broadcast).
//   2. build the column table once: per output column the two source byte offsets and the weight, flip folded in
//      (8 bytes an entry, LDS), and the band's row table (two staged-row offsets and the weight per output row).
//   3. every thread produces packs of 8 consecutive output elements of one row and stores each as one 16-byte vector
//      (bf16) or two (fp32).  NCHW: the thread owns 8 x-positions, reads their 8 column entries, the row pair and the
//      erase test once and walks the channels with them, one pack per channel plane (this halved the time of a
//      pack-per-channel split that re-read the table).  Channels-last: 8 elements of the flattened [S * C] row, the
//      channel and column advancing inside the pack.  A row length that is no multiple of 8 makes rows start off a
//      vector boundary: those shapes take the same kernel with element stores and a bounds test (VEC = false).  A pack
//      that lies inside the erase box is stored as zeros; one that straddles an edge selects per element.
//      Normalisation is one fma per element, v * (inv_std / 255) - mean * inv_std.
// No atomics, no fences: the output is a pure function of (x, idx, rec), bit for bit.  The kernel clamps the record's
// box into the image and the index into the dataset, so records made by hand cannot make it read out of bounds.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"
#include "philox.h"

namespace ringdp {
namespace kern {

using namespace dev;

namespace {

constexpr int kThreads = 256;
constexpr int kBandRows = 16;  // of 32 / 16 / 8 / 4 the fastest at S = 224 and 384 (profiles/r16/resize_crop)
constexpr int kAttempts = 10;

__device__ __forceinline__ float u24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// floor(u * n) for u in [0, 1), kept below n against the rounding of the product
__device__ __forceinline__ int upos(float u, int n) { return clampi((int)(u * (float)n), 0, n - 1); }

__global__ __launch_bounds__(kThreads) void crop_draw_kernel(const uint64_t* __restrict__ snapshot, CropDrawArgs a,
                                                             int32_t* __restrict__ rec) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.R) return;
  const uint64_t seed = snapshot[0], step = snapshot[1];
  const uint32_t s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  int y0 = 0, x0 = 0, h = a.H, w = a.W;
  if (a.crop) {
    const float area = (float)(a.H * a.W), lr0 = logf(a.ratio0), lr1 = logf(a.ratio1);
    bool found = false;
#pragma unroll 1
    for (int t = 0; t < kAttempts && !found; ++t) {
      const philox::U4 q = philox::philox4x32_10((uint32_t)r, s0, s1, (uint32_t)t, k0, k1);
      const float ta = area * (a.scale0 + (a.scale1 - a.scale0) * u24(q.w[0]));
      const float ar = expf(lr0 + (lr1 - lr0) * u24(q.w[1]));
      const float fw = rintf(sqrtf(ta * ar)), fh = rintf(sqrtf(ta / ar));
      if (fw >= 1.f && fw <= (float)a.W && fh >= 1.f && fh <= (float)a.H) {
        found = true;
        w = (int)fw;
        h = (int)fh;
        y0 = upos(u24(q.w[2]), a.H - h + 1);
        x0 = upos(u24(q.w[3]), a.W - w + 1);
      }
    }
    if (!found) {  // the centre crop, ratio clamped to [ratio0, ratio1]
      const float in_ratio = (float)a.W / (float)a.H;
      if (in_ratio < a.ratio0)
        h = clampi((int)rintf((float)a.W / a.ratio0), 1, a.H);
      else if (in_ratio > a.ratio1)
        w = clampi((int)rintf((float)a.H * a.ratio1), 1, a.W);
      y0 = (a.H - h) / 2;
      x0 = (a.W - w) / 2;
    }
  }
  const philox::U4 d = philox::philox4x32_10((uint32_t)r, s0, s1, (uint32_t)kAttempts, k0, k1);
  const int flip = (a.hflip && u24(d.w[0]) < 0.5f) ? 1 : 0;
  int ey0 = 0, ey1 = 0, ex0 = 0, ex1 = 0;
  if (u24(d.w[1]) < a.erase_prob) {
    const float area = (float)(a.S * a.S), lr0 = logf(a.eratio0), lr1 = logf(a.eratio1);
    bool found = false;
#pragma unroll 1
    for (int t = 0; t < kAttempts && !found; ++t) {
      const philox::U4 q = philox::philox4x32_10((uint32_t)r, s0, s1, (uint32_t)(kAttempts + 1 + t), k0, k1);
      const float ta = area * (a.escale0 + (a.escale1 - a.escale0) * u24(q.w[0]));
      const float ar = expf(lr0 + (lr1 - lr0) * u24(q.w[1]));
      const float fh = rintf(sqrtf(ta * ar)), fw = rintf(sqrtf(ta / ar));
      if (fh < (float)a.S && fw < (float)a.S) {
        found = true;
        const int eh = (int)fh, ew = (int)fw;
        if (eh >= 1 && ew >= 1) {  // a box without rows or columns is the empty box
          ey0 = upos(u24(q.w[2]), a.S - eh + 1);
          ex0 = upos(u24(q.w[3]), a.S - ew + 1);
          ey1 = ey0 + eh;
          ex1 = ex0 + ew;
        }
      }
    }
  }
  int32_t* o = rec + (int64_t)r * 8;
  o[0] = y0;
  o[1] = x0;
  o[2] = h;
  o[3] = w;
  o[4] = flip;
  o[5] = ey0 | (ey1 << 16);
  o[6] = ex0 | (ex1 << 16);
  o[7] = 0;
}

struct ResizeCropArgs {
  int B, H, W, C, S;
  int bands;        // ceil(S / kBandRows)
  int rec_words;    // 8: a record per sample, 0: every sample reads record 0
  int col_bytes;    // LDS bytes of the column table (S * 8, rounded up to 16)
  int x_low;        // the low 4 bits of x's address
  int64_t N;        // images in the dataset
  int64_t x_bytes;  // N * H * W * C
  float scale[4];   // per channel: inv_std / 255 and -mean * inv_std, so that the result is fma(v, scale, bias)
  float bias[4];
};

struct ColEntry {
  uint16_t lo, hi;  // byte offsets of the two source pixels within a staged row
  float w;          // weight of hi
};

// Source pair and weight of output coordinate d for a box side of n pixels resized by `scale` = n / S:
// s = scale * (d + 0.5) - 0.5 clamped at 0, i0 = floor(s), i1 = min(i0 + 1, n - 1), lam = s - i0.
__device__ __forceinline__ void src_pair(int d, float scale, int n, int& i0, int& i1, float& lam) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 > n - 1 ? n - 1 : i0;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  lam = s - (float)i0;
}

template <typename T, int E>
struct alignas(sizeof(T) * E) Pack {
  T v[E];
};

__device__ __forceinline__ float pick(const float (&t)[4], int c) {
  return c == 0 ? t[0] : (c == 1 ? t[1] : (c == 2 ? t[2] : t[3]));
}

template <typename T, bool NHWC, bool VEC>
__global__ __launch_bounds__(kThreads) void resize_crop_kernel(const uint8_t* __restrict__ x,
                                                               const int64_t* __restrict__ labels,
                                                               const int64_t* __restrict__ idx,
                                                               const int32_t* __restrict__ rec, ResizeCropArgs a,
                                                               T* __restrict__ out, int64_t* __restrict__ yout) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int row_lo[kBandRows], row_hi[kBandRows];
  __shared__ float row_w[kBandRows];
  ColEntry* col = reinterpret_cast<ColEntry*>(smem);
  uint8_t* src = smem + a.col_bytes;

  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.bands, band = blockIdx.x - b * a.bands;
  const int H = a.H, W = a.W, C = a.C, S = a.S;
  const int32_t* r = rec + (size_t)b * a.rec_words;
  const int y0 = clampi(r[0], 0, H - 1), x0 = clampi(r[1], 0, W - 1);
  const int h = clampi(r[2], 1, H - y0), w = clampi(r[3], 1, W - x0);
  const bool flip = r[4] != 0;
  const int ey0 = r[5] & 0xffff, ey1 = (r[5] >> 16) & 0xffff, ex0 = r[6] & 0xffff, ex1 = (r[6] >> 16) & 0xffff;
  int64_t img = idx[b];
  img = img < 0 ? 0 : (img > a.N - 1 ? a.N - 1 : img);
  if (labels && band == 0 && tid == 0) yout[b] = labels[img];

  const int oy0 = band * kBandRows, rows = min(S - oy0, kBandRows);
  const float sh = (float)h / (float)S, sw = (float)w / (float)S;
  int ilo, ihi, tmp;
  float lam;
  src_pair(oy0, sh, h, ilo, tmp, lam);
  src_pair(oy0 + rows - 1, sh, h, tmp, ihi, lam);
  const int ylo = y0 + ilo, yhi = y0 + ihi;  // the source rows [ylo, yhi] of this band
  const int rowbytes = W * C;

  // 1. stage: dataset bytes [g0, g1) -> src[shift ...], by 16-byte chunks of the aligned range around them
  const int64_t g0 = (img * H + ylo) * rowbytes, g1 = g0 + (int64_t)(yhi - ylo + 1) * rowbytes;
  const int shift = (int)((g0 + a.x_low) & 15);
  const int64_t a0 = g0 - shift;
  const int nchunks = (int)((g1 - a0 + 15) >> 4);
  for (int k = tid; k < nchunks; k += kThreads) {
    const int64_t p = a0 + 16 * (int64_t)k;
    if (p >= 0 && p + 16 <= a.x_bytes) {
      *reinterpret_cast<uint4*>(src + 16 * k) = *reinterpret_cast<const uint4*>(x + p);
    } else {
#pragma unroll 1
      for (int j = 0; j < 16; ++j)
        if (p + j >= 0 && p + j < a.x_bytes) src[16 * k + j] = x[p + j];
    }
  }
  // 2. the tables
  for (int rr = tid; rr < rows; rr += kThreads) {
    int i0, i1;
    src_pair(oy0 + rr, sh, h, i0, i1, lam);
    row_lo[rr] = shift + (y0 + i0 - ylo) * rowbytes;
    row_hi[rr] = shift + (y0 + i1 - ylo) * rowbytes;
    row_w[rr] = lam;
  }
  for (int ox = tid; ox < S; ox += kThreads) {
    int i0, i1;
    src_pair(flip ? S - 1 - ox : ox, sw, w, i0, i1, lam);
    col[ox] = ColEntry{(uint16_t)((x0 + i0) * C), (uint16_t)((x0 + i1) * C), lam};
  }
  __syncthreads();

  // 3. packs of 8 output elements
  if constexpr (!NHWC) {
    // a thread takes 8 x-positions of one row and walks the channels: the column entries, the row weights and the
    // erase test are shared by the C packs it stores
    const int nvec = (S + 7) >> 3, items = rows * nvec;
    for (int i = tid; i < items; i += kThreads) {
      const int rr = i / nvec, j0 = (i - rr * nvec) << 3, oy = oy0 + rr;
      const bool in_rows = oy >= ey0 && oy < ey1;
      const bool all_erased = in_rows && j0 >= ex0 && min(j0 + 7, S - 1) < ex1;
      ColEntry e[8];
      uint32_t erased = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        e[k] = col[min(j0 + k, S - 1)];  // the min only serves the unused tail of a last pack
        erased |= (in_rows && j0 + k >= ex0 && j0 + k < ex1) ? 1u << k : 0u;
      }
      const int tlo = row_lo[rr], blo = row_hi[rr];
      const float lh1 = row_w[rr], lh0 = 1.f - lh1;
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const float scale = pick(a.scale, c), bias = pick(a.bias, c);
        const uint8_t* top = src + tlo + c;
        const uint8_t* bot = src + blo + c;
        Pack<T, 8> o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float f = 0.f;
          if (!all_erased) {
            const float lw1 = e[k].w, lw0 = 1.f - lw1;
            const float p00 = (float)top[e[k].lo], p01 = (float)top[e[k].hi];
            const float p10 = (float)bot[e[k].lo], p11 = (float)bot[e[k].hi];
            const float v = lh0 * (lw0 * p00 + lw1 * p01) + lh1 * (lw0 * p10 + lw1 * p11);
            f = (erased >> k & 1u) ? 0.f : __builtin_fmaf(v, scale, bias);
          }
          o.v[k] = (T)f;
        }
        const int64_t base = (((int64_t)b * C + c) * S + oy) * S + j0;
        if (VEC) {
          *reinterpret_cast<Pack<T, 8>*>(out + base) = o;
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (j0 + k < S) out[base + k] = o.v[k];
        }
      }
    }
  } else {
    // 8 elements of the flattened [S * C] row: the channel and the column advance inside the pack
    const int rowlen = S * C, nvec = (rowlen + 7) >> 3, items = rows * nvec;
    for (int i = tid; i < items; i += kThreads) {
      const int rr = i / nvec, j0 = (i - rr * nvec) << 3, oy = oy0 + rr;
      int ox = j0 / C, c = j0 - ox * C;
      const bool in_rows = oy >= ey0 && oy < ey1;
      const bool all_erased = in_rows && ox >= ex0 && min(j0 + 7, rowlen - 1) / C < ex1;
      const uint8_t* top = src + row_lo[rr];
      const uint8_t* bot = src + row_hi[rr];
      const float lh1 = row_w[rr], lh0 = 1.f - lh1;
      Pack<T, 8> o;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float f = 0.f;
        if (!all_erased) {
          const ColEntry e = col[min(ox, S - 1)];
          const float lw1 = e.w, lw0 = 1.f - lw1;
          const float p00 = (float)top[e.lo + c], p01 = (float)top[e.hi + c];
          const float p10 = (float)bot[e.lo + c], p11 = (float)bot[e.hi + c];
          const float v = lh0 * (lw0 * p00 + lw1 * p01) + lh1 * (lw0 * p10 + lw1 * p11);
          f = (in_rows && ox >= ex0 && ox < ex1) ? 0.f : __builtin_fmaf(v, pick(a.scale, c), pick(a.bias, c));
        }
        o.v[k] = (T)f;
        if (++c == C) {
          c = 0;
          ++ox;
        }
      }
      const int64_t base = ((int64_t)b * S + oy) * rowlen + j0;
      if (VEC) {
        *reinterpret_cast<Pack<T, 8>*>(out + base) = o;
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (j0 + k < rowlen) out[base + k] = o.v[k];
      }
    }
  }
}

template <typename T, bool NHWC>
void launch_resize(bool vec, unsigned grid, size_t lds, const uint8_t* x, const int64_t* labels, const int64_t* idx,
                   const int32_t* rec, const ResizeCropArgs& a, void* out, int64_t* yout, hipStream_t s) {
  if (vec)
    resize_crop_kernel<T, NHWC, true><<<grid, kThreads, lds, s>>>(x, labels, idx, rec, a, static_cast<T*>(out), yout);
  else
    resize_crop_kernel<T, NHWC, false><<<grid, kThreads, lds, s>>>(x, labels, idx, rec, a, static_cast<T*>(out), yout);
}

}  // namespace

void crop_draw(const uint64_t* snapshot, const CropDrawArgs& a, int32_t* rec, hipStream_t s) {
  if (a.R <= 0) return;
  crop_draw_kernel<<<(unsigned)((a.R + kThreads - 1) / kThreads), kThreads, 0, s>>>(snapshot, a, rec);
}

void resize_crop(const uint8_t* x, const int64_t* labels, const int64_t* idx, const int32_t* rec, bool rec_elem,
                 int B, int64_t N, int H, int W, int C, int S, const AugNorm& nrm, bool nhwc, bool out_bf16,
                 void* out, int64_t* yout, hipStream_t s) {
  if (B <= 0) return;
  ResizeCropArgs a{};
  a.B = B;
  a.H = H;
  a.W = W;
  a.C = C;
  a.S = S;
  a.bands = (S + kBandRows - 1) / kBandRows;
  a.rec_words = rec_elem ? 8 : 0;
  a.col_bytes = (S * (int)sizeof(ColEntry) + 15) & ~15;
  a.x_low = (int)(reinterpret_cast<uintptr_t>(x) & 15);
  a.N = N;
  a.x_bytes = N * H * W * C;
  for (int c = 0; c < 4; ++c) {
    a.scale[c] = nrm.inv_std[c] * (1.f / 255.f);
    a.bias[c] = -nrm.mean[c] * nrm.inv_std[c];
  }
  // the staged rows start up to 15 bytes into their first chunk and end up to 15 bytes before the last one's end
  const size_t lds = (size_t)a.col_bytes + (size_t)H * W * C + 32;
  const unsigned grid = (unsigned)B * (unsigned)a.bands;
  const int rowlen = nhwc ? S * C : S;
  const bool vec = rowlen % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 32 == 0;
  if (out_bf16) {
    if (nhwc)
      launch_resize<bf16, true>(vec, grid, lds, x, labels, idx, rec, a, out, yout, s);
    else
      launch_resize<bf16, false>(vec, grid, lds, x, labels, idx, rec, a, out, yout, s);
  } else {
    if (nhwc)
      launch_resize<float, true>(vec, grid, lds, x, labels, idx, rec, a, out, yout, s);
    else
      launch_resize<float, false>(vec, grid, lds, x, labels, idx, rec, a, out, yout, s);
  }
}

}  // namespace kern
}  // namespace ringdp
