// Fused attention for any sequence length (head dim 64): the kernels of vit.hip made key-blocked.
//
// vit.hip holds all of K and V of a head in LDS and a query tile's whole score row in registers (Tp <= 256).
// Here a workgroup takes 64 queries (forward, dQ) or 64 keys (dK / dV), one 16-row tile per wave, and walks
// the other side in blocks of ATTL_KB rows staged through LDS with the same swizzles; per block every wave
// does exactly what the short kernels do for a whole head, on the same lane layouts.  The forward carries an
// online softmax (running maximum, sum and O^T accumulator in registers, rescaled every block); the backward
// recomputes P from the forward's log-sum-exp and takes D = rowsum(dO * O) from the saved output rows, so the
// keys are walked once.  Operands are the token rows of the qkv projection; P is never stored; every output
// row and every column-sum partial is written by exactly one wave / workgroup (no atomics: bitwise
// reproducible).  Workgroup ids are bh * NB + block, so the blocks of one head run next to each other and
// share its K / V (or Q / dO) in L2.
#include <algorithm>

#include "device_common.h"
#include "kernels.h"
#include "vit_attn.h"

namespace ringdp {
namespace kern {

using namespace ringdp::dev;

namespace {

constexpr int ATTL_KB = 128;            // rows per staged block: 2 x 16 KiB of LDS, 32 score registers
constexpr int ATTL_NT = ATTL_KB / 16;   // 16-row tiles per block
constexpr int ATTL_WG = 64;             // rows owned by a workgroup: one 16-row tile per wave

// stage rows r0 .. r0 + ATTL_KB of two operands into LDS (rows >= T zero), each with its own swizzle
template <bool A_KSW, bool B_KSW>
__device__ __forceinline__ void attl_stage(const AttnIn& a, const AttnIn& b, bf16* As, bf16* Bs, int bh, int H, int r0,
                                           int T) {
  for (int c = threadIdx.x; c < ATTL_KB * 8; c += 256) {  // 16-B chunks: row c >> 3, columns 8 (c & 7) ..
    const int r = c >> 3, d = (c & 7) * 8;
    *reinterpret_cast<bf16x8*>(As + (A_KSW ? att_ksw(r, d) : att_vsw(r, d))) = a.load8(bh, H, r0 + r, T, d);
    *reinterpret_cast<bf16x8*>(Bs + (B_KSW ? att_ksw(r, d) : att_vsw(r, d))) = b.load8(bh, H, r0 + r, T, d);
  }
}

// Forward.  Per key block: S^T = K Q^T into ATTL_NT f32x4 (lane (g, q): keys k0 + 16t + 4g + i of query
// q = lane & 15), block maximum, m_new = max(m, block max), one per-lane factor exp2((m - m_new) c) on the 16
// accumulator registers and the running sum (every element of a lane belongs to query lane & 15), then
// exp2(s c - m_new c) as bf16 straight into O^T += V^T P^T.  Every block starts below T (Tp - T < 16 and
// ATTL_KB % 16 == 0), so its maximum is finite and the first block's factor is exp2(-inf) = 0, never
// exp2(-inf + inf).  The running sum stays a per-lane partial (the factor is the same for the four lanes of
// a query) and is reduced once at the end.
__global__ __launch_bounds__(256) void attn_fwd_long_kernel(AttnIn q, AttnIn k, AttnIn v, int T, int Tp, int H, int NB,
                                                            float scale, AttnOut o, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[ATTL_KB * ATT_D];
  __shared__ __attribute__((aligned(16))) bf16 Vs[ATTL_KB * ATT_D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / NB, q0 = (blockIdx.x % NB) * ATTL_WG + wave * 16;
  const bool live = q0 < Tp;  // wave-uniform: Tp need not be a multiple of 64
  const int g = lane >> 4, qi = lane & 15, qrow = q0 + qi;
  const int q4 = qi >> 2, p4 = qi & 3;  // tr16 lane roles inside the 16-lane group
  const bf16x8 qf0 = q.load8(bh, H, qrow, T, 8 * g);
  const bf16x8 qf1 = q.load8(bh, H, qrow, T, 32 + 8 * g);
  const float c2 = scale * 1.4426950408889634f;
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
    for (int t = 0; t < ATTL_NT; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float e = __builtin_amdgcn_exp2f(fmaf(st[t][i], c2, -mc));
        sum += e;
        pb[t][i] = (bf16)e;
      }
    }
    l = fmaf(l, alpha, sum);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ot[dt] *= alpha;
    // O^T[d][q] += sum over key pairs (t0, t0 + 1) of V^T (keys 16t + 4g + j) x P^T
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
  if (g == 0) lse[(int64_t)bh * Tp + qrow] = qrow < T ? m * scale + __logf(l) : INFINITY;
  if (qrow < o.rows) {
    const float inv = 1.f / l;
    bf16* orow = o.row(bh, H, qrow) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *reinterpret_cast<bf16x4*>(orow + 16 * dt) =
          bf16x4{(bf16)(ot[dt][0] * inv), (bf16)(ot[dt][1] * inv), (bf16)(ot[dt][2] * inv), (bf16)(ot[dt][3] * inv)};
  }
}

// Backward, query side: per key block P = exp(scale S - lse) recomputed as in attn_bwd_dq_kernel's LSE
// branch, dP^T = V dO^T, dS = scale P (dP - D), dQ^T += K^T dS^T accumulated over the blocks in registers.
// D = rowsum(dO * O) from the saved forward output (equal to rowsum(dP * P), and known before the first key
// block, so the keys are walked once); it is written to dsum for the key-side kernel.
// cs_out: [B * NB][3*H*64] partials, row (batch, query block): column sums of this workgroup's dQ rows.
__global__ __launch_bounds__(256) void attn_bwd_dq_long_kernel(AttnIn dout, AttnIn q, AttnIn k, AttnIn v, AttnIn out,
                                                               const float* __restrict__ lse, float scale, int T,
                                                               int Tp, int H, int NB, float* __restrict__ dsum,
                                                               AttnOut dq, float* __restrict__ cs_out) {
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
  f32x4 qt4[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) qt4[dt] = zero_f32x4();
  for (int k0 = 0; k0 < Tp; k0 += ATTL_KB) {
    if (k0) __syncthreads();
    attl_stage<true, false>(v, k, Vs, Ks, bh, H, k0, T);
    __syncthreads();
    if (!live) continue;
    const int nt = min(ATTL_NT, (Tp - k0) >> 4);
    auto ds_tile = [&](int t) {  // lane (g, q): keys k0 + 16t + 4g + i
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
        r[i] = (bf16)(scale * (float)pv * (dpt[i] - dot));
      }
      return r;
    };
#pragma unroll
    for (int ks = 0; ks < ATTL_NT / 2; ++ks) {
      if (2 * ks < nt) {  // a tile >= nt of a started pair is all keys >= T: dS = 0
        const int t0 = 2 * ks, t1 = 2 * ks + 1;
        const bf16x4 d0 = ds_tile(t0), d1 = ds_tile(t1);
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

// Backward, key side: each wave keeps dV^T and dK^T of its 16-key tile in 32 accumulator registers (K and V
// of the tile in registers as MFMA B operands) while the workgroup streams Q and dO through LDS in blocks of
// ATTL_KB queries; per query pair it does what attn_bwd_dkdv_kernel<NT, true> does.
__global__ __launch_bounds__(256) void attn_bwd_dkdv_long_kernel(AttnIn dout, AttnIn q, AttnIn k, AttnIn v,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ dsum, float scale, int T,
                                                                 int Tp, int H, int NB, AttnOut dk, AttnOut dv,
                                                                 float* __restrict__ cs_out) {
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
    for (int ks = 0; 2 * ks < nt; ++ks) {
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
          pb[u][r] = (bf16)pr;
          sb[u][r] = (bf16)(scale * pr * (dpv[r] - dq4[r]));
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
  float csk[4][4] = {}, csv[4][4] = {};
  if (live && key < dk.rows) {
    bf16* krow = dk.row(bh, H, key) + 4 * g;
    bf16* vrow = dv.row(bh, H, key) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
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

// Tp = T rounded up to 16 (every staged block then starts below T, which the online softmax relies on)
bool attl_shape_ok(int B, int T, int H, int Tp, int Dh) {
  return Dh == ATT_D && B > 0 && H > 0 && T > 0 && Tp == (T + 15) / 16 * 16 &&
         (int64_t)B * H * attn_long_blocks(Tp) < ((int64_t)1 << 31);
}

}  // namespace

int attn_long_blocks(int Tp) { return (Tp + ATTL_WG - 1) / ATTL_WG; }

bool attn_fwd_rows_long(const void* qkv, int B, int T, int H, int Tp, int Dh, float scale, float* lse, void* out,
                        hipStream_t s) {
  if (!attl_shape_ok(B, T, H, Tp, Dh)) return false;
  const int64_t w3 = (int64_t)3 * H * ATT_D, w1 = (int64_t)H * ATT_D;
  const int NB = attn_long_blocks(Tp);
  attn_fwd_long_kernel<<<B * H * NB, 256, 0, s>>>(token_rows(qkv, T, w3, 0), token_rows(qkv, T, w3, w1),
                                                  token_rows(qkv, T, w3, 2 * w1), T, Tp, H, NB, scale,
                                                  token_rows_out(out, T, w1, 0), lse);
  return true;
}

bool attn_bwd_rows_long(const void* dout_rows, const void* qkv, const float* lse, const void* out_rows, int B, int T,
                        int H, int Tp, int Dh, float scale, float* dsum, void* dqkv, hipStream_t s,
                        float* colsum_part) {
  if (!attl_shape_ok(B, T, H, Tp, Dh)) return false;
  const int64_t w3 = (int64_t)3 * H * ATT_D, w1 = (int64_t)H * ATT_D;
  const int NB = attn_long_blocks(Tp);
  const AttnIn dout = token_rows(dout_rows, T, w1, 0), q = token_rows(qkv, T, w3, 0), k = token_rows(qkv, T, w3, w1),
               v = token_rows(qkv, T, w3, 2 * w1);
  attn_bwd_dq_long_kernel<<<B * H * NB, 256, 0, s>>>(dout, q, k, v, token_rows(out_rows, T, w1, 0), lse, scale, T, Tp, H,
                                                     NB, dsum, token_rows_out(dqkv, T, w3, 0), colsum_part);
  attn_bwd_dkdv_long_kernel<<<B * H * NB, 256, 0, s>>>(dout, q, k, v, lse, dsum, scale, T, Tp, H, NB,
                                                       token_rows_out(dqkv, T, w3, w1),
                                                       token_rows_out(dqkv, T, w3, 2 * w1), colsum_part);
  return true;
}

}  // namespace kern
}  // namespace ringdp
