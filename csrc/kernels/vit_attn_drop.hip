// Fused attention with dropout on the attention probabilities (head dim 64, any sequence length): the
// key-blocked kernels of vit_attn_long.hip with a Philox mask applied to P in registers.
//
//   P = softmax(scale Q K^T) over the T real keys,  Pd = keep ? scale_keep P : 0,  O = Pd V
//   backward: dPd = dO V^T, dP = keep ? scale_keep dPd : 0, D = rowsum(dO * O) (= rowsum(dP * P)),
//             dS = scale P (dP - D), dV = Pd^T dO, dK = dS^T Q, dQ = dS K
//
// Work split, LDS stages, swizzles, lane layouts and the column-sum epilogue are those of vit_attn_long.hip: 64
// query (or key) rows per workgroup, one 16-row tile per wave, the other side in 128-row blocks; P and the mask
// are never stored, every output row and column-sum partial has one writer.  The saved log-sum-exp is that of
// the undropped softmax, so the backward recomputes P as before and regenerates the mask.
//
// Mask (ringdp/ops/dropout.py): one Philox4x32-10 call covers a 4 x 4 tile of (query, key) pairs of one (batch,
// head): counter (g, step lo, step hi, site) with g = ((bh N4 + tq / 4) N4 + tk / 4), N4 = ceil(T / 4); the 8-bit
// draw of (tq, tk) is byte tk & 3 of word tq & 3; keep iff draw >= thr8.  A call is ~70 VALU instructions, so
// no lane makes one per four P elements.  The four lanes of a quad (lane & 3) hold the four query rows (forward,
// dQ) or the four key columns (dK / dV) of the same mask tiles: per four 16-row tiles of the walked side each
// lane of the quad makes the call of one tile, and the quad transposes the 4 x 4 words in registers with DPP
// quad permutes (xor 1, then xor 2; four moves and eight selects) - one call per 16 P elements, no LDS.  On the
// key side a lane needs byte p of each of a tile's four words, so the caller packs those bytes into one word per
// receiver before the same transpose.
//
// scale_keep never touches a P element: dropped elements are zeroed in the bf16 fragment, the running sum takes
// the undropped values and scale_keep folds into the final 1 / l (forward); in the backward it multiplies dP
// under the same select and the dV accumulators once at the end.
#include <algorithm>

#include "device_common.h"
#include "kernels.h"
#include "philox.h"
#include "vit_attn.h"

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

struct AttnDrop {
  const uint64_t* snapshot;  // {seed, step} of the forward's rng_tick
  uint32_t site, thr8, N4;
  float keep_scale;  // 256 / (256 - thr8)
};

struct DropKey {  // the wave-uniform words of a call
  uint32_t k0, k1, s0, s1, site;
  __device__ __forceinline__ explicit DropKey(const AttnDrop& a) {
    const uint64_t seed = a.snapshot[0], step = a.snapshot[1];
    k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32);
    site = a.site;
  }
  __device__ __forceinline__ void words(uint32_t g, uint32_t (&w)[4]) const {
    const philox::U4 r = philox::philox4x32_10(g, s0, s1, site, k0, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = r.w[i];
  }
};

template <int CTL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTL, 0xF, 0xF, false);
}

// 4 x 4 transpose inside a quad: lane p (= lane & 3) comes in with w[u] and leaves with lane u's w[p]
__device__ __forceinline__ void quad_transpose(uint32_t (&w)[4], int p) {
  const bool o1 = p & 1, o2 = p & 2;
#pragma unroll
  for (int m = 0; m < 2; ++m) {  // lanes p ^ 1 swap the off-diagonal words of the 2 x 2 blocks
    const uint32_t a = w[2 * m], b = w[2 * m + 1];
    const uint32_t r = quad_perm<0xB1>(o1 ? a : b);  // quad_perm [1, 0, 3, 2]
    w[2 * m] = o1 ? r : a;
    w[2 * m + 1] = o1 ? b : r;
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {  // lanes p ^ 2 swap the off-diagonal 2 x 2 blocks
    const uint32_t a = w[m], b = w[m + 2];
    const uint32_t r = quad_perm<0x4E>(o2 ? a : b);  // quad_perm [2, 3, 0, 1]
    w[m] = o2 ? r : a;
    w[m + 2] = o2 ? b : r;
  }
}

__device__ __forceinline__ bool drop_keep(uint32_t w, int i, uint32_t thr8) { return ((w >> (8 * i)) & 0xffu) >= thr8; }

// Forward / query side: lane (g, q) holds keys 16t + 4g + i of query row q.  g0 = counter of this lane's row of
// mask tiles at key tile 16j of the block; lane p calls for 16-key tile 4j + p (four mask tiles further per
// 16 keys) and leaves with word p of the tiles 4j .. 4j + 3: byte i of w[u] is the draw of key 16 (4j + u) + 4g + i.
__device__ __forceinline__ void drop_words_q(const DropKey& key, uint32_t g0, int p4, uint32_t (&w)[4]) {
  key.words(g0 + 4u * (uint32_t)p4, w);
  quad_transpose(w, p4);
}

// Key side: lane (g, k) holds queries 16 qp + 4g + r of key column k.  g0 = counter of this lane's column of mask
// tiles at query tile 16j of the block; lane p calls for 16-query tile 4j + p (4 N4 counters further per 16
// queries), packs byte p' of the four words for receiver p', and leaves with its own column's bytes of the tiles
// 4j .. 4j + 3: byte r of w[u] is the draw of query 16 (4j + u) + 4g + r.
__device__ __forceinline__ void drop_words_k(const DropKey& key, uint32_t g0, uint32_t N4, int p4, uint32_t (&w)[4]) {
  uint32_t x[4];
  key.words(g0 + 4u * (uint32_t)p4 * N4, x);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    w[c] = ((x[0] >> (8 * c)) & 0xffu) | (((x[1] >> (8 * c)) & 0xffu) << 8) | (((x[2] >> (8 * c)) & 0xffu) << 16) |
           (((x[3] >> (8 * c)) & 0xffu) << 24);
  quad_transpose(w, p4);
}

// attn_fwd_long_kernel with the mask: the bf16 P fragment is zeroed where dropped, the running sum is not.
__global__ __launch_bounds__(256) void attn_drop_fwd_kernel(AttnIn q, AttnIn k, AttnIn v, int T, int Tp, int H, int NB,
                                                            float scale, AttnDrop drop, AttnOut o,
                                                            float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[ATTL_KB * ATT_D];
  __shared__ __attribute__((aligned(16))) bf16 Vs[ATTL_KB * ATT_D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / NB, q0 = (blockIdx.x % NB) * ATTL_WG + wave * 16;
  const bool live = q0 < Tp;  // wave-uniform: Tp need not be a multiple of 64
  const int g = lane >> 4, qi = lane & 15, qrow = q0 + qi;
  const int q4 = qi >> 2, p4 = qi & 3;  // tr16 lane roles inside the 16-lane group; p4: the lane of the quad
  const bf16x8 qf0 = q.load8(bh, H, qrow, T, 8 * g);
  const bf16x8 qf1 = q.load8(bh, H, qrow, T, 32 + 8 * g);
  const float c2 = scale * 1.4426950408889634f;
  const DropKey key(drop);
  // counter of the mask tile (query rows 4 (q0 / 4 + q4) .., keys 4g ..): + k0 / 4 + 4t per key tile
  const uint32_t grow = ((uint32_t)bh * drop.N4 + (uint32_t)((q0 >> 2) + q4)) * drop.N4 + (uint32_t)g;
  float m = -INFINITY, l = 0.f;  // running maximum of the raw scores; this lane's part of the running sum
  f32x4 ot[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) ot[dt] = zero_f32x4();
  for (int k0 = 0; k0 < Tp; k0 += ATTL_KB) {
    if (k0) __syncthreads();  // every wave is done with the previous block
    attl_stage<true, false>(k, v, Ks, Vs, bh, H, k0, T);
    __syncthreads();
    if (!live) continue;
    const int nt = min(ATTL_NT, (Tp - k0) >> 4);  // tiles of this block below Tp
    f32x4 st[ATTL_NT];
#pragma unroll
    for (int t = 0; t < ATTL_NT; ++t) {
      if (t < nt) {
        const int kr = 16 * t + qi;
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(Ks + att_ksw(kr, 8 * g));
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(Ks + att_ksw(kr, 32 + 8 * g));
        st[t] = mfma16x16x32(a1, qf1, mfma16x16x32(a0, qf0, zero_f32x4()));
      } else {
        st[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    // only the tile that reaches past T is masked (a scalar test per tile)
#pragma unroll
    for (int t = 0; t < ATTL_NT; ++t)
      if (t < nt && k0 + 16 * t + 16 > T)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!(k0 + 16 * t + 4 * g + i < T)) st[t][i] = -INFINITY;
    float bm = -INFINITY;
#pragma unroll
    for (int t = 0; t < ATTL_NT; ++t) bm = fmaxf(bm, fmaxf(fmaxf(st[t][0], st[t][1]), fmaxf(st[t][2], st[t][3])));
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
    m = mn;
    const float mc = mn * c2;
    float sum = 0.f;
    bf16x4 pb[ATTL_NT];
#pragma unroll
    for (int j = 0; j < ATTL_NT / 4; ++j) {
      uint32_t mw[4] = {};
      if (4 * j < nt) drop_words_q(key, grow + (uint32_t)((k0 >> 2) + 16 * j), p4, mw);  // wave-uniform test
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = 4 * j + u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = __builtin_amdgcn_exp2f(fmaf(st[t][i], c2, -mc));  // keys >= T: exp2(-inf) = 0
          sum += e;
          pb[t][i] = drop_keep(mw[u], i, drop.thr8) ? (bf16)e : (bf16)0.f;
        }
      }
    }
    l = fmaf(l, alpha, sum);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ot[dt] *= alpha;
    // O^T[d][q] += sum over key pairs (t0, t0 + 1) of V^T (keys 16t + 4g + j) x Pd^T
#pragma unroll
    for (int ks = 0; ks < ATTL_NT / 2; ++ks) {
      if (2 * ks < nt) {  // a tile >= nt of a started pair has P = 0 and zero V rows
        const int t0 = 2 * ks, t1 = 2 * ks + 1;
        const bf16x8 bfr = bf16x8{pb[t0][0], pb[t0][1], pb[t0][2], pb[t0][3], pb[t1][0], pb[t1][1], pb[t1][2], pb[t1][3]};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x4 lo = lds_read_tr16(Vs + att_vsw(16 * t0 + 4 * g + q4, 16 * dt + 4 * p4));
          const bf16x4 hi = lds_read_tr16(Vs + att_vsw(16 * t1 + 4 * g + q4, 16 * dt + 4 * p4));
          const bf16x8 afr = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          ot[dt] = mfma16x16x32(afr, bfr, ot[dt]);
        }
      }
    }
  }
  if (!live) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (g == 0) lse[(int64_t)bh * Tp + qrow] = qrow < T ? m * scale + __logf(l) : INFINITY;  // of the undropped P
  if (qrow < o.rows) {
    const float inv = drop.keep_scale / l;
    bf16* orow = o.row(bh, H, qrow) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *reinterpret_cast<bf16x4*>(orow + 16 * dt) =
          bf16x4{(bf16)(ot[dt][0] * inv), (bf16)(ot[dt][1] * inv), (bf16)(ot[dt][2] * inv), (bf16)(ot[dt][3] * inv)};
  }
}

// attn_bwd_dq_long_kernel with the mask on dP: dS = scale P ((keep ? scale_keep dP : 0) - D).  The key tiles are
// walked four at a time (two MFMA pairs) so that a quad's four calls cover them.
__global__ __launch_bounds__(256) void attn_drop_bwd_dq_kernel(AttnIn dout, AttnIn q, AttnIn k, AttnIn v, AttnIn out,
                                                               const float* __restrict__ lse, float scale, int T,
                                                               int Tp, int H, int NB, AttnDrop drop,
                                                               float* __restrict__ dsum, AttnOut dq,
                                                               float* __restrict__ cs_out) {
  __shared__ __attribute__((aligned(16))) bf16 Vs[ATTL_KB * ATT_D];
  __shared__ __attribute__((aligned(16))) bf16 Ks[ATTL_KB * ATT_D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / NB, blk = blockIdx.x % NB, q0 = blk * ATTL_WG + wave * 16;
  const bool live = q0 < Tp;
  const int g = lane >> 4, qi = lane & 15, qrow = q0 + qi;
  const int q4 = qi >> 2, p4 = qi & 3;
  const bf16x8 of0 = dout.load8(bh, H, qrow, T, 8 * g);
  const bf16x8 of1 = dout.load8(bh, H, qrow, T, 32 + 8 * g);
  const bf16x8 qf0 = q.load8(bh, H, qrow, T, 8 * g);
  const bf16x8 qf1 = q.load8(bh, H, qrow, T, 32 + 8 * g);
  float dot = 0.f;
  {
    const bf16x8 o0 = out.load8(bh, H, qrow, T, 8 * g);
    const bf16x8 o1 = out.load8(bh, H, qrow, T, 32 + 8 * g);
#pragma unroll
    for (int i = 0; i < 8; ++i) dot = fmaf((float)of0[i], (float)o0[i], fmaf((float)of1[i], (float)o1[i], dot));
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
  }
  const float lq = live ? lse[(int64_t)bh * Tp + qrow] : INFINITY;  // +inf for padded queries: P = 0
  if (live && g == 0) dsum[(int64_t)bh * Tp + qrow] = dot;
  const DropKey key(drop);
  const uint32_t grow = ((uint32_t)bh * drop.N4 + (uint32_t)((q0 >> 2) + q4)) * drop.N4 + (uint32_t)g;
  f32x4 qt4[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) qt4[dt] = zero_f32x4();
  for (int k0 = 0; k0 < Tp; k0 += ATTL_KB) {
    if (k0) __syncthreads();
    attl_stage<true, false>(v, k, Vs, Ks, bh, H, k0, T);
    __syncthreads();
    if (!live) continue;
    const int nt = min(ATTL_NT, (Tp - k0) >> 4);
    auto ds_tile = [&](int t, uint32_t mw) {  // lane (g, q): keys k0 + 16t + 4g + i
      const int kr = 16 * t + qi;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(Ks + att_vsw(kr, 8 * g));
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(Ks + att_vsw(kr, 32 + 8 * g));
      const f32x4 sv = mfma16x16x32(a1, qf1, mfma16x16x32(a0, qf0, zero_f32x4()));
      const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Vs + att_ksw(kr, 8 * g));
      const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(Vs + att_ksw(kr, 32 + 8 * g));
      const f32x4 dpt = mfma16x16x32(b1, of1, mfma16x16x32(b0, of0, zero_f32x4()));
      bf16x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16 pv = (bf16)(k0 + 16 * t + 4 * g + i < T ? __expf(sv[i] * scale - lq) : 0.f);
        const float dp = drop_keep(mw, i, drop.thr8) ? drop.keep_scale * dpt[i] : 0.f;
        r[i] = (bf16)(scale * (float)pv * (dp - dot));
      }
      return r;
    };
#pragma unroll
    for (int j = 0; j < ATTL_NT / 4; ++j) {
      if (4 * j < nt) {
        uint32_t mw[4];
        drop_words_q(key, grow + (uint32_t)((k0 >> 2) + 16 * j), p4, mw);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int t0 = 4 * j + 2 * h, t1 = t0 + 1;
          if (t0 < nt) {  // a tile >= nt of a started pair is all keys >= T: dS = 0
            const bf16x4 d0 = ds_tile(t0, mw[2 * h]), d1 = ds_tile(t1, mw[2 * h + 1]);
            const bf16x8 bfr = bf16x8{d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              const bf16x4 lo = lds_read_tr16(Ks + att_vsw(16 * t0 + 4 * g + q4, 16 * dt + 4 * p4));
              const bf16x4 hi = lds_read_tr16(Ks + att_vsw(16 * t1 + 4 * g + q4, 16 * dt + 4 * p4));
              const bf16x8 afr = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
              qt4[dt] = mfma16x16x32(afr, bfr, qt4[dt]);
            }
          }
        }
      }
    }
  }
  float csum[4][4] = {};
  if (live && qrow < dq.rows) {
    bf16* drow = dq.row(bh, H, qrow) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x4 o = bf16x4{(bf16)qt4[dt][0], (bf16)qt4[dt][1], (bf16)qt4[dt][2], (bf16)qt4[dt][3]};
      *reinterpret_cast<bf16x4*>(drow + 16 * dt) = o;
#pragma unroll
      for (int e = 0; e < 4; ++e) csum[dt][e] = (float)o[e];
    }
  }
  if (cs_out) {  // q part of partial row (batch, block)
    __syncthreads();  // every wave is done with Vs
    attn_colsum_store(csum, reinterpret_cast<float*>(Vs),
                      cs_out + ((int64_t)(bh / H) * NB + blk) * 3 * H * ATT_D + (bh % H) * ATT_D);
  }
}

// attn_bwd_dkdv_long_kernel with the mask: the dV fragment takes P where kept (scale_keep once on the
// accumulators at the end), dS as on the query side.  The query-pair loop of the long kernel becomes a loop over
// groups of four query tiles (two pairs), one call per lane and group.
__global__ __launch_bounds__(256) void attn_drop_bwd_dkdv_kernel(AttnIn dout, AttnIn q, AttnIn k, AttnIn v,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ dsum, float scale, int T,
                                                                 int Tp, int H, int NB, AttnDrop drop, AttnOut dk,
                                                                 AttnOut dv, float* __restrict__ cs_out) {
  __shared__ __attribute__((aligned(16))) bf16 Qs[ATTL_KB * ATT_D];
  __shared__ __attribute__((aligned(16))) bf16 Os[ATTL_KB * ATT_D];  // dO
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / NB, blk = blockIdx.x % NB, key0 = blk * ATTL_WG + wave * 16;
  const bool live = key0 < Tp;
  const int g = lane >> 4, ki = lane & 15, key = key0 + ki;
  const int q4 = ki >> 2, p4 = ki & 3;
  const bf16x8 vf0 = v.load8(bh, H, key, T, 8 * g);
  const bf16x8 vf1 = v.load8(bh, H, key, T, 32 + 8 * g);
  const bf16x8 kf0 = k.load8(bh, H, key, T, 8 * g);
  const bf16x8 kf1 = k.load8(bh, H, key, T, 32 + 8 * g);
  const float* db = dsum + (int64_t)bh * Tp;
  const float* lq = lse + (int64_t)bh * Tp;
  const DropKey rng(drop);
  // counter of the mask tile (queries 4g .., key columns 4 (key0 / 4 + q4) ..): + (q0 / 4 + 4 qp) N4 per query tile
  const uint32_t gcol = ((uint32_t)bh * drop.N4 + (uint32_t)g) * drop.N4 + (uint32_t)((key0 >> 2) + q4);
  f32x4 dva[4], dka[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dva[dt] = dka[dt] = zero_f32x4();
  for (int q0 = 0; q0 < Tp; q0 += ATTL_KB) {
    if (q0) __syncthreads();
    attl_stage<false, false>(q, dout, Qs, Os, bh, H, q0, T);
    __syncthreads();
    if (!live) continue;
    const int nt = min(ATTL_NT, (Tp - q0) >> 4);  // query tiles of this block below Tp
#pragma unroll 1
    for (int j = 0; 4 * j < nt; ++j) {
      uint32_t mw[4];
      drop_words_k(rng, gcol + (uint32_t)((q0 >> 2) + 16 * j) * drop.N4, drop.N4, p4, mw);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ks = 2 * j + h;
        if (2 * ks < nt) {
          const bool has1 = 2 * ks + 1 < nt;
          const int qp[2] = {2 * ks, has1 ? 2 * ks + 1 : 2 * ks};  // tiles inside the block
          bf16x4 pb[2], sb[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            // dP[q][key] and S[q][key] for queries q0 + 16 qp + 4g + r: A = dO / Q rows (LDS), B = V / K rows (registers)
            const int orow = 16 * qp[u] + ki;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(Os + att_vsw(orow, 8 * g));
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(Os + att_vsw(orow, 32 + 8 * g));
            const f32x4 dpv = mfma16x16x32(a1, vf1, mfma16x16x32(a0, vf0, zero_f32x4()));
            const bf16x8 c0 = *reinterpret_cast<const bf16x8*>(Qs + att_vsw(orow, 8 * g));
            const bf16x8 c1 = *reinterpret_cast<const bf16x8*>(Qs + att_vsw(orow, 32 + 8 * g));
            const f32x4 spv = mfma16x16x32(c1, kf1, mfma16x16x32(c0, kf0, zero_f32x4()));
            const f32x4 dq4 = *reinterpret_cast<const f32x4*>(db + q0 + 16 * qp[u] + 4 * g);
            const f32x4 lq4 = *reinterpret_cast<const f32x4*>(lq + q0 + 16 * qp[u] + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              // the bf16 value the query side used; lse = +inf for padded queries
              const float pr = (u == 0 || has1) && key < T ? (float)(bf16)__expf(spv[r] * scale - lq4[r]) : 0.f;
              const bool keep = drop_keep(mw[2 * h + u], r, drop.thr8);
              pb[u][r] = keep ? (bf16)pr : (bf16)0.f;
              sb[u][r] = (bf16)(scale * pr * ((keep ? drop.keep_scale * dpv[r] : 0.f) - dq4[r]));
            }
          }
          const bf16x8 pfr = bf16x8{pb[0][0], pb[0][1], pb[0][2], pb[0][3], pb[1][0], pb[1][1], pb[1][2], pb[1][3]};
          const bf16x8 sfr = bf16x8{sb[0][0], sb[0][1], sb[0][2], sb[0][3], sb[1][0], sb[1][1], sb[1][2], sb[1][3]};
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const bf16x4 olo = lds_read_tr16(Os + att_vsw(16 * qp[0] + 4 * g + q4, 16 * dt + 4 * p4));
            const bf16x4 ohi = lds_read_tr16(Os + att_vsw(16 * qp[1] + 4 * g + q4, 16 * dt + 4 * p4));
            dva[dt] = mfma16x16x32(bf16x8{olo[0], olo[1], olo[2], olo[3], ohi[0], ohi[1], ohi[2], ohi[3]}, pfr, dva[dt]);
            const bf16x4 qlo = lds_read_tr16(Qs + att_vsw(16 * qp[0] + 4 * g + q4, 16 * dt + 4 * p4));
            const bf16x4 qhi = lds_read_tr16(Qs + att_vsw(16 * qp[1] + 4 * g + q4, 16 * dt + 4 * p4));
            dka[dt] = mfma16x16x32(bf16x8{qlo[0], qlo[1], qlo[2], qlo[3], qhi[0], qhi[1], qhi[2], qhi[3]}, sfr, dka[dt]);
          }
        }
      }
    }
  }
  float csk[4][4] = {}, csv[4][4] = {};
  if (live && key < dk.rows) {
    bf16* krow = dk.row(bh, H, key) + 4 * g;
    bf16* vrow = dv.row(bh, H, key) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dva[dt] *= drop.keep_scale;  // dV = Pd^T dO: the kept P were accumulated unscaled
      const bf16x4 ko = bf16x4{(bf16)dka[dt][0], (bf16)dka[dt][1], (bf16)dka[dt][2], (bf16)dka[dt][3]};
      const bf16x4 vo = bf16x4{(bf16)dva[dt][0], (bf16)dva[dt][1], (bf16)dva[dt][2], (bf16)dva[dt][3]};
      *reinterpret_cast<bf16x4*>(krow + 16 * dt) = ko;
      *reinterpret_cast<bf16x4*>(vrow + 16 * dt) = vo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        csk[dt][e] = (float)ko[e];
        csv[dt][e] = (float)vo[e];
      }
    }
  }
  if (cs_out) {  // k part, then v part of partial row (batch, block)
    float* row = cs_out + ((int64_t)(bh / H) * NB + blk) * 3 * H * ATT_D + (bh % H) * ATT_D;
    __syncthreads();  // every wave is done with Qs / Os
    attn_colsum_store(csk, reinterpret_cast<float*>(Qs), row + H * ATT_D);
    attn_colsum_store(csv, reinterpret_cast<float*>(Os), row + 2 * H * ATT_D);
  }
}

// the shapes of the key-blocked kernels, a threshold that drops something, and a 32-bit tile counter
bool attn_drop_ok(int B, int T, int H, int Tp, int Dh, const uint64_t* snapshot, uint32_t thr8) {
  const int64_t N4 = ((int64_t)T + 3) / 4;
  return Dh == ATT_D && B > 0 && H > 0 && T > 0 && Tp == (T + 15) / 16 * 16 && snapshot != nullptr && thr8 >= 1 &&
         thr8 <= 255 && (int64_t)B * H * attn_long_blocks(Tp) < ((int64_t)1 << 31) &&
         (int64_t)B * H * N4 <= ((int64_t)1 << 32) / N4;
}

AttnDrop drop_args(int T, const uint64_t* snapshot, uint32_t site, uint32_t thr8) {
  return AttnDrop{snapshot, site, thr8, (uint32_t)((T + 3) / 4), (float)(256.0 / (double)(256u - thr8))};
}

}  // namespace

bool attn_drop_fwd_rows(const void* qkv, int B, int T, int H, int Tp, int Dh, float scale, const uint64_t* snapshot,
                        uint32_t site, uint32_t thr8, float* lse, void* out, hipStream_t s) {
  if (!attn_drop_ok(B, T, H, Tp, Dh, snapshot, thr8)) return false;
  const int64_t w3 = (int64_t)3 * H * ATT_D, w1 = (int64_t)H * ATT_D;
  const int NB = attn_long_blocks(Tp);
  attn_drop_fwd_kernel<<<B * H * NB, 256, 0, s>>>(token_rows(qkv, T, w3, 0), token_rows(qkv, T, w3, w1),
                                                  token_rows(qkv, T, w3, 2 * w1), T, Tp, H, NB, scale,
                                                  drop_args(T, snapshot, site, thr8), token_rows_out(out, T, w1, 0),
                                                  lse);
  return true;
}

bool attn_drop_bwd_rows(const void* dout_rows, const void* qkv, const float* lse, const void* out_rows, int B, int T,
                        int H, int Tp, int Dh, float scale, const uint64_t* snapshot, uint32_t site, uint32_t thr8,
                        float* dsum, void* dqkv, hipStream_t s, float* colsum_part) {
  if (!attn_drop_ok(B, T, H, Tp, Dh, snapshot, thr8)) return false;
  const int64_t w3 = (int64_t)3 * H * ATT_D, w1 = (int64_t)H * ATT_D;
  const int NB = attn_long_blocks(Tp);
  const AttnDrop drop = drop_args(T, snapshot, site, thr8);
  const AttnIn dout = token_rows(dout_rows, T, w1, 0), q = token_rows(qkv, T, w3, 0), k = token_rows(qkv, T, w3, w1),
               v = token_rows(qkv, T, w3, 2 * w1);
  attn_drop_bwd_dq_kernel<<<B * H * NB, 256, 0, s>>>(dout, q, k, v, token_rows(out_rows, T, w1, 0), lse, scale, T, Tp, H,
                                                     NB, drop, dsum, token_rows_out(dqkv, T, w3, 0), colsum_part);
  attn_drop_bwd_dkdv_kernel<<<B * H * NB, 256, 0, s>>>(dout, q, k, v, lse, dsum, scale, T, Tp, H, NB, drop,
                                                       token_rows_out(dqkv, T, w3, w1),
                                                       token_rows_out(dqkv, T, w3, 2 * w1), colsum_part);
  return true;
}

}  // namespace kern
}  // namespace ringdp
