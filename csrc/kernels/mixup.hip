// Mixup / CutMix for image batches [B, C, H, W] on gfx950, hipGraph-safe (timm's Mixup, "batch" and "elem" modes).
//
//  * mix_draw_kernel    one thread per record (1 per batch or 1 per sample): decides not applied / mixup / cutmix,
//                       draws lam0 ~ Beta(alpha, alpha) and the cutmix box, writes an 8-word device record
//  * mix_images_kernel  out[b] = mix of x[b] and its partner x[B - 1 - b] as record b (or record 0) says, and
//                       y_b[b] = y[B - 1 - b]
//
// Like the dropout masks (dropout.hip) every draw is Philox4x32-10 of the forward's (seed, step) snapshot, here with
// counter = (record, step lo, step hi, round): lam and the box live in device memory and change with every replay of
// a captured step.  No atomics, fences or counters: draw, mix and the loss are ordered by kernel boundaries.
//
// Record (int32 [8]): 0 lam (fp32 bits, the weight of the sample's own label), 1 kind (0 not applied, 1 mixup,
// 2 cutmix), 2..5 box y0 y1 x0 x1 (half-open, empty unless cutmix), 6 lam0 (fp32 bits, the Beta draw before the box
// correction), 7 zero.
//
// Generator calls of a record, numbered by `round` from 0 in the order they are made:
//   round 0   w0 apply (u < prob), w1 cutmix instead of mixup (u < switch_prob), w2 / w3 the box centre cy / cx
//   alpha == 1: one call, lam0 = the open uniform of w0
//   otherwise:  lam0 = X / (X + Y) from two Gamma(alpha) variates, each by Marsaglia & Tsang's method ("A simple
//               method for generating gamma variables", ACM TOMS 2000), one call per attempt: w0, w1 a Box-Muller
//               normal, w2 the acceptance uniform, w3 the U^(1/alpha) boost that alpha < 1 needs (Gamma(alpha) =
//               Gamma(alpha + 1) * U^(1/alpha)).  X's attempts come first, then Y's.
// An attempt is accepted with probability > 0.95 for every shape >= 1, and the loop is bounded at kGammaRounds = 8
// attempts: all 8 are refused with probability < 0.05^8 = 4e-11 per variate, and then the last positive candidate
// is kept (the shape's own d = a - 1/3 if there was none).  The ratio is formed from the logarithms, so a variate
// that would underflow fp32 (small alpha) still gives a lam0 in [0, 1].
//
// mix_images is a memory-bound stream shaped like dropout_kernel: one 16-byte vector per thread and trip, at most
// 2048 workgroups of 256 threads, a grid-stride loop, no LDS.  It reads x[b] where the output is x[b], the partner
// where it is the partner, and both only for mixup and for a cutmix vector that straddles a box edge.  In batch
// mode the record pointer is wave-uniform.  A sample whose byte size is no multiple of 16 (or an unaligned base)
// takes the same kernel with one element per thread.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"
#include "philox.h"

namespace ringdp {
namespace kern {

using namespace dev;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = 2048;
constexpr int kGammaRounds = 8;

struct Gen {
  uint32_t rec, s0, s1, k0, k1, round;
  __device__ philox::U4 next() { return philox::philox4x32_10(rec, s0, s1, round++, k0, k1); }
};

// 24-bit uniform in [0, 1) for the decisions (prob = 1 always applies, prob = 0 never); 23-bit uniform in (0, 1),
// exact in fp32, where a logarithm is taken
__device__ __forceinline__ float u_half_open(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }
__device__ __forceinline__ float u_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

// log of a Gamma(alpha, 1) variate
__device__ float log_gamma_variate(Gen& g, float alpha) {
  const float a = alpha < 1.f ? alpha + 1.f : alpha;
  const float d = a - 1.f / 3.f, c = 1.f / sqrtf(9.f * d);
  float v = 1.f, boost = 0.f;
#pragma unroll 1
  for (int t = 0; t < kGammaRounds; ++t) {
    const philox::U4 w = g.next();
    const float x = sqrtf(-2.f * logf(u_open(w.w[0]))) * cosf(6.28318530718f * u_half_open(w.w[1]));
    boost = logf(u_open(w.w[3])) / alpha;
    const float cand = 1.f + c * x;
    if (cand <= 0.f) continue;
    v = cand * cand * cand;
    if (logf(u_open(w.w[2])) < 0.5f * x * x + d - d * v + d * logf(v)) break;
  }
  const float lg = logf(d * v);
  return alpha < 1.f ? lg + boost : lg;
}

__device__ float beta_variate(Gen& g, float alpha) {
  if (alpha == 1.f) return u_open(g.next().w[0]);
  const float lx = log_gamma_variate(g, alpha);
  const float ly = log_gamma_variate(g, alpha);
  return 1.f / (1.f + expf(ly - lx));  // X / (X + Y); exp overflow gives 0
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void mix_draw_kernel(const uint64_t* __restrict__ snapshot, MixDrawArgs a,
                                                            int32_t* __restrict__ rec) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.R) return;
  const uint64_t seed = snapshot[0], step = snapshot[1];
  Gen g{(uint32_t)r, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), 0u};
  const philox::U4 w = g.next();
  const bool mix_on = a.mixup_alpha > 0.f, cut_on = a.cutmix_alpha > 0.f;
  int kind = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  float lam = 1.f, lam0 = 1.f;
  if ((mix_on || cut_on) && u_half_open(w.w[0]) < a.prob) {
    const bool cut = cut_on && (!mix_on || u_half_open(w.w[1]) < a.switch_prob);
    lam0 = beta_variate(g, cut ? a.cutmix_alpha : a.mixup_alpha);
    if (cut) {
      kind = 2;
      const float ratio = sqrtf(1.f - lam0);
      const int cut_h = (int)((float)a.H * ratio), cut_w = (int)((float)a.W * ratio);
      const int cy = (int)(w.w[2] % (uint32_t)a.H), cx = (int)(w.w[3] % (uint32_t)a.W);
      y0 = clampi(cy - cut_h / 2, 0, a.H);
      y1 = clampi(cy + cut_h / 2, 0, a.H);
      x0 = clampi(cx - cut_w / 2, 0, a.W);
      x1 = clampi(cx + cut_w / 2, 0, a.W);
      lam = 1.f - (float)((y1 - y0) * (x1 - x0)) / (float)(a.H * a.W);
    } else {
      kind = 1;
      lam = lam0;
    }
  }
  int32_t* o = rec + (int64_t)r * 8;
  o[0] = __builtin_bit_cast(int32_t, lam);
  o[1] = kind;
  o[2] = y0;
  o[3] = y1;
  o[4] = x0;
  o[5] = x1;
  o[6] = __builtin_bit_cast(int32_t, lam0);
  o[7] = 0;
}

struct MixImageArgs {
  uint32_t B;
  uint32_t units;      // packs of E elements per sample
  uint32_t nunits;     // B * units (< 2^31, checked by the caller)
  uint32_t rowlen;     // elements per image row: W * inner
  uint32_t H;
  int inner;           // elements per pixel step in x: 1 (NCHW) or C (channels-last)
  uint32_t rec_words;  // 8 in elem mode, 0 in batch mode (every sample reads record 0)
};

template <typename T, int E>
struct alignas(sizeof(T) * E) Pack {
  T v[E];
};

__device__ __forceinline__ float as_f32(float v) { return v; }
__device__ __forceinline__ float as_f32(bf16 v) { return (float)v; }

// A sample is [outer][H][W][inner] elements; element e of it lies in image row (e / rowlen) % H at e % rowlen of
// that row, and the box covers the row offsets [x0 * inner, x1 * inner) of the rows [y0, y1).
template <typename T, int E>
__global__ __launch_bounds__(kThreads) void mix_images_kernel(const T* __restrict__ x, const int64_t* __restrict__ y,
                                                              const int32_t* __restrict__ rec, MixImageArgs a,
                                                              T* __restrict__ out, int64_t* __restrict__ y_b) {
  typedef Pack<T, E> P;
  const P* xp = reinterpret_cast<const P*>(x);
  P* op = reinterpret_cast<P*>(out);
  const uint32_t gid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  for (uint32_t b = gid; b < a.B; b += stride) y_b[b] = y[a.B - 1 - b];
  for (uint32_t v = gid; v < a.nunits; v += stride) {
    const uint32_t b = v / a.units, j = v - b * a.units;
    const uint32_t pb = a.B - 1 - b, pv = pb * a.units + j;
    const int32_t* r = rec + (size_t)b * a.rec_words;
    const int kind = pb == b ? 0 : r[1];  // the middle sample of an odd batch is its own partner
    P o;
    if (kind == 1) {
      const float lam = __builtin_bit_cast(float, r[0]), rest = 1.f - lam;
      const P va = xp[v], vb = xp[pv];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float fa = as_f32(va.v[k]), fb = as_f32(vb.v[k]);
        // one fp32 rounding of the sum, then the output's; equal inputs are kept exactly
        o.v[k] = fa == fb ? va.v[k] : (T)__builtin_fmaf(lam, fa, rest * fb);
      }
    } else if (kind == 2) {
      const int y0 = r[2], y1 = r[3], c0 = r[4] * a.inner, c1 = r[5] * a.inner;
      const uint32_t e = j * E, row = e / a.rowlen, col = e - row * a.rowlen;
      if (E == 1 || col + E <= a.rowlen) {  // the pack lies in one image row
        const int h = (int)(row % a.H), lo = (int)col;
        int n_in = 0;
        if (h >= y0 && h < y1) n_in = (lo + E < c1 ? lo + E : c1) - (lo > c0 ? lo : c0);
        if (n_in <= 0) {
          o = xp[v];
        } else if (n_in == E) {
          o = xp[pv];
        } else {
          const P va = xp[v], vb = xp[pv];
#pragma unroll
          for (int k = 0; k < E; ++k) o.v[k] = (lo + k >= c0 && lo + k < c1) ? vb.v[k] : va.v[k];
        }
      } else {  // a pack that runs over a row end (rowlen no multiple of E): element by element
        const P va = xp[v], vb = xp[pv];
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const uint32_t rk = (e + k) / a.rowlen;
          const int ck = (int)(e + k - rk * a.rowlen), hk = (int)(rk % a.H);
          o.v[k] = (hk >= y0 && hk < y1 && ck >= c0 && ck < c1) ? vb.v[k] : va.v[k];
        }
      }
    } else {
      o = xp[v];
    }
    op[v] = o;
  }
}

template <typename T, int E>
void launch_images(const void* x, const int64_t* y, const int32_t* rec, MixImageArgs a, int64_t sample_elems,
                   void* out, int64_t* y_b, hipStream_t s) {
  a.units = (uint32_t)(sample_elems / E);
  a.nunits = a.B * a.units;
  int64_t blocks = ((int64_t)a.nunits + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  mix_images_kernel<T, E><<<(unsigned)blocks, kThreads, 0, s>>>(static_cast<const T*>(x), y, rec, a,
                                                               static_cast<T*>(out), y_b);
}

}  // namespace

void mix_draw(const uint64_t* snapshot, const MixDrawArgs& a, int32_t* rec, hipStream_t s) {
  if (a.R <= 0) return;
  mix_draw_kernel<<<(unsigned)((a.R + kThreads - 1) / kThreads), kThreads, 0, s>>>(snapshot, a, rec);
}

void mix_images(const void* x, bool x_bf16, const int64_t* y, const int32_t* rec, bool elem, int64_t B,
                int64_t sample_elems, int H, int W, int inner, bool vec, void* out, int64_t* y_b, hipStream_t s) {
  if (B <= 0 || sample_elems <= 0) return;
  MixImageArgs a{};
  a.B = (uint32_t)B;
  a.rowlen = (uint32_t)(W * inner);
  a.H = (uint32_t)H;
  a.inner = inner;
  a.rec_words = elem ? 8u : 0u;
  if (x_bf16) {
    if (vec)
      launch_images<bf16, 8>(x, y, rec, a, sample_elems, out, y_b, s);
    else
      launch_images<bf16, 1>(x, y, rec, a, sample_elems, out, y_b, s);
  } else {
    if (vec)
      launch_images<float, 4>(x, y, rec, a, sample_elems, out, y_b, s);
    else
      launch_images<float, 1>(x, y, rec, a, sample_elems, out, y_b, s);
  }
}

}  // namespace kern
}  // namespace ringdp
