// Operand / index layout and issue rate of gfx950's sparse MFMA v_smfmac_f32_16x16x64_bf16, found on the GPU
// (the ISA manual's tables are not assumed), against v_mfma_f32_16x16x32_bf16 in the same harness.
//
//   layout   one-hot compressed A values against B registers that carry their own (lane group, slot, column)
//            as small integers: which B register element every (A lane, A slot, 2-bit index) multiplies, which
//            bit field of the index VGPR belongs to which A slot, and what the two immediates (cbsz, abid) do.
//            The derived map is then checked on random operands against a CPU product, with index pairs that
//            are ascending, equal and descending.
//   rate     a long stream of 8 independent accumulators, 1 and 2 waves per SIMD, one workgroup and one per CU;
//            s_memtime ticks and event time per instruction.
//
// hipcc --offload-arch=gfx950 -O3 tools/smfmac_probe.hip -o build/smfmac_probe && build/smfmac_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                                \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) {                                                                  \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One experiment per 64-thread workgroup: A [64 lanes][8], B [64][16] (bf16 bits), idx [64], C [64][4].
template <int CBSZ, int ABID>
__global__ __launch_bounds__(64) void one_smfmac(const uint16_t* __restrict__ A, const uint16_t* __restrict__ Bm,
                                                 const uint32_t* __restrict__ idx, float* __restrict__ C) {
  const int e = blockIdx.x, l = threadIdx.x;
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(A + ((size_t)e * 64 + l) * 8);
  const bf16x16 b = *reinterpret_cast<const bf16x16*>(Bm + ((size_t)e * 64 + l) * 16);
  const int ix = (int)idx[(size_t)e * 64 + l];
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, c, ix, CBSZ, ABID);
  *reinterpret_cast<f32x4*>(C + ((size_t)e * 64 + l) * 4) = c;
}

template <bool SPARSE>
__global__ void rate_kernel(float* __restrict__ out, long long* __restrict__ ticks, int iters) {
  const int l = threadIdx.x;
  bf16x16 b;
  bf16x8 a;
  for (int i = 0; i < 16; ++i) b[i] = (__bf16)(float)((l + i) & 3);
  for (int i = 0; i < 8; ++i) a[i] = (__bf16)(float)((l + 2 * i) & 1);
  const bf16x8 b8 = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]};
  int ix = 0x44444444;  // every group: first value at position 0, second at position 1
  asm volatile("" : "+v"(ix));
  f32x4 acc[8];
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const long long t0 = (long long)__builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (SPARSE)
        acc[j] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, acc[j], ix, 0, 0);
      else
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b8, acc[j], 0, 0, 0);
    }
  }
  float s = 0.f;
  for (int j = 0; j < 8; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  asm volatile("" ::"v"(s));
  const long long t1 = (long long)__builtin_amdgcn_s_memtime();
  out[(size_t)blockIdx.x * blockDim.x + l] = s;
  if ((l & 63) == 0) ticks[(size_t)blockIdx.x * (blockDim.x / 64) + (l >> 6)] = t1 - t0;
}

static uint16_t bf(float v) {  // exact for the small integers used here
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return (uint16_t)(u >> 16);
}

struct Batch {
  int n;
  std::vector<uint16_t> A, B;
  std::vector<uint32_t> idx;
  std::vector<float> C;
  explicit Batch(int n_) : n(n_), A((size_t)n_ * 512, 0), B((size_t)n_ * 1024, 0), idx((size_t)n_ * 64, 0),
                           C((size_t)n_ * 256, 0.f) {}
  uint16_t& a(int e, int lane, int slot) { return A[((size_t)e * 64 + lane) * 8 + slot]; }
  uint16_t& b(int e, int lane, int slot) { return B[((size_t)e * 64 + lane) * 16 + slot]; }
  float c(int e, int lane, int r) const { return C[((size_t)e * 64 + lane) * 4 + r]; }
  void run(int cfg) {
    uint16_t *dA, *dB;
    uint32_t* dI;
    float* dC;
    CK(hipMalloc(&dA, A.size() * 2));
    CK(hipMalloc(&dB, B.size() * 2));
    CK(hipMalloc(&dI, idx.size() * 4));
    CK(hipMalloc(&dC, C.size() * 4));
    CK(hipMemcpy(dA, A.data(), A.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), B.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dI, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    if (cfg == 0) one_smfmac<0, 0><<<n, 64>>>(dA, dB, dI, dC);
    if (cfg == 1) one_smfmac<0, 1><<<n, 64>>>(dA, dB, dI, dC);
    if (cfg == 2) one_smfmac<1, 0><<<n, 64>>>(dA, dB, dI, dC);
    if (cfg == 3) one_smfmac<0, 2><<<n, 64>>>(dA, dB, dI, dC);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(C.data(), dC, C.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(dA));
    CK(hipFree(dB));
    CK(hipFree(dI));
    CK(hipFree(dC));
  }
};

// B planes: every B register element holds 1 + one coordinate of itself
enum { PL_SLOT = 0, PL_GROUP = 1, PL_COL = 2, NPL = 3 };
static void fill_plane(Batch& bt, int e, int plane) {
  for (int lane = 0; lane < 64; ++lane)
    for (int f = 0; f < 16; ++f)
      bt.b(e, lane, f) = bf(1.f + (plane == PL_SLOT ? f : plane == PL_GROUP ? (lane >> 4) : (lane & 15)));
}

// What a one-hot A (value 1) produced in the three planes: the output row (C layout assumed the dense one:
// lane = 16 * (row / 4) + column, register = row % 4; checked), the B lane group and the B slot it met.
struct Hit {
  int m = -1, gB = -1, f = -1;
  bool ok = false;
  bool operator==(const Hit& o) const { return m == o.m && gB == o.gB && f == o.f && ok == o.ok; }
};
static Hit decode(const Batch& bt, int e0) {
  Hit h;
  int vals[NPL];
  for (int pl = 0; pl < NPL; ++pl) {
    int row = -1, val = -1;
    bool good = true;
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 4; ++r) {
        const float c = bt.c(e0 + pl, lane, r);
        if (c == 0.f) continue;
        const int m = 4 * (lane >> 4) + r;
        if (row < 0) row = m;
        if (m != row) good = false;
        const int v = (int)c - 1;
        if (pl == PL_COL) {
          if (v != (lane & 15)) good = false;  // column n of C comes from B lanes with lane % 16 == n
        } else {
          if (val < 0) val = v;
          if (v != val) good = false;
        }
      }
    if (row < 0 || !good) return h;
    if (h.m >= 0 && h.m != row) return h;
    h.m = row;
    vals[pl] = val;
  }
  h.f = vals[PL_SLOT];
  h.gB = vals[PL_GROUP];
  h.ok = true;
  return h;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static const char* cfg_name[4] = {"cbsz=0 abid=0", "cbsz=0 abid=1", "cbsz=1 abid=0", "cbsz=0 abid=2"};

static void layout_probe() {
  int field[4][8];  // [cfg][A slot] -> 2-bit field number in the index VGPR
  // ---- phase A: which index field moves A slot e's partner (all lanes carry the same index word)
  for (int cfg = 0; cfg < 4; ++cfg) {
    const int lanes[4] = {0, 21, 42, 63};
    Batch bt(4 * 8 * 17 * NPL);
    auto eid = [&](int li, int e, int bp) { return ((li * 8 + e) * 17 + bp) * NPL; };
    for (int li = 0; li < 4; ++li)
      for (int e = 0; e < 8; ++e)
        for (int bp = 0; bp <= 16; ++bp)
          for (int pl = 0; pl < NPL; ++pl) {
            const int x = eid(li, e, bp) + pl;
            bt.a(x, lanes[li], e) = bf(1.f);
            fill_plane(bt, x, pl);
            for (int lane = 0; lane < 64; ++lane) bt.idx[(size_t)x * 64 + lane] = bp < 16 ? 3u << (2 * bp) : 0u;
          }
    bt.run(cfg);
    std::printf("[%s] index field of A slot e (same for the probed lanes 0, 21, 42, 63 unless noted):", cfg_name[cfg]);
    for (int e = 0; e < 8; ++e) {
      int fe = -2;
      for (int li = 0; li < 4; ++li) {
        const Hit base = decode(bt, eid(li, e, 16));
        int found = -1, nfound = 0;
        for (int bp = 0; bp < 16; ++bp) {
          const Hit h = decode(bt, eid(li, e, bp));
          if (!h.ok || !base.ok) std::printf(" (undecodable lane %d slot %d field %d)", lanes[li], e, bp);
          if (!(h == base)) {
            found = bp;
            ++nfound;
          }
        }
        if (nfound != 1) std::printf(" (lane %d slot %d: %d fields move it)", lanes[li], e, nfound);
        if (fe == -2) fe = found;
        if (fe != found) std::printf(" (lane %d slot %d: field %d)", lanes[li], e, found);
      }
      field[cfg][e] = fe;
      std::printf(" e%d->f%d", e, fe);
    }
    std::printf("\n");
  }
  // ---- phase B (cbsz = abid = 0): every A lane, slot and index value, the index word only in the A lane
  static Hit T[64][8][4];
  {
    Batch bt(64 * 8 * 4 * NPL);
    auto eid = [&](int la, int e, int v) { return ((la * 8 + e) * 4 + v) * NPL; };
    for (int la = 0; la < 64; ++la)
      for (int e = 0; e < 8; ++e)
        for (int v = 0; v < 4; ++v)
          for (int pl = 0; pl < NPL; ++pl) {
            const int x = eid(la, e, v) + pl;
            bt.a(x, la, e) = bf(1.f);
            fill_plane(bt, x, pl);
            if (field[0][e] >= 0) bt.idx[(size_t)x * 64 + la] = (uint32_t)v << (2 * field[0][e]);
          }
    bt.run(0);
    int bad = 0, rowbad = 0, nonuni = 0;
    for (int la = 0; la < 64; ++la)
      for (int e = 0; e < 8; ++e)
        for (int v = 0; v < 4; ++v) {
          T[la][e][v] = decode(bt, eid(la, e, v));
          const Hit& h = T[la][e][v];
          if (!h.ok) ++bad;
          if (h.m != (la & 15)) ++rowbad;
          const Hit& r = T[la & ~15][e][v];
          if (h.gB != r.gB || h.f != r.f) ++nonuni;
        }
    std::printf("[map] undecodable %d, row != A lane %% 16: %d, differs inside a 16-lane group: %d\n", bad, rowbad,
                nonuni);
    std::printf("[map] A lane group gA, slot e, index value v -> B (lane group, slot); B lane = 16 * group + column\n");
    for (int gA = 0; gA < 4; ++gA)
      for (int e = 0; e < 8; ++e) {
        std::printf("  gA%d e%d:", gA, e);
        for (int v = 0; v < 4; ++v) std::printf("  v%d->(g%d,s%2d)", v, T[16 * gA][e][v].gB, T[16 * gA][e][v].f);
        std::printf("\n");
      }
    // dense k named so that A group (gA, pair e/2) covers k = 16 gA + 4 (e/2) + v: print B's k per (group, slot)
    int kB[4][16];
    for (int g = 0; g < 4; ++g)
      for (int f = 0; f < 16; ++f) kB[g][f] = -1;
    int clash = 0;
    for (int gA = 0; gA < 4; ++gA)
      for (int e = 0; e < 8; ++e)
        for (int v = 0; v < 4; ++v) {
          const Hit& h = T[16 * gA][e][v];
          if (!h.ok) continue;
          const int k = 16 * gA + 4 * (e / 2) + v;
          if (kB[h.gB][h.f] >= 0 && kB[h.gB][h.f] != k) ++clash;
          kB[h.gB][h.f] = k;
        }
    std::printf("[map] dense k of B (lane group g, slot s), with A pair (gA, e/2) named k = 16 gA + 4 (e/2) + v; "
                "clashes %d\n", clash);
    for (int g = 0; g < 4; ++g) {
      std::printf("  g%d:", g);
      for (int f = 0; f < 16; ++f) std::printf(" %2d", kB[g][f]);
      std::printf("\n");
    }
  }
  // ---- phase C: the map on random operands, index pairs ascending / equal / descending / any
  for (int mode = 0; mode < 4; ++mode) {
    const int N = 64;
    Batch bt(N);
    for (int x = 0; x < N; ++x)
      for (int lane = 0; lane < 64; ++lane) {
        for (int e = 0; e < 8; ++e) bt.a(x, lane, e) = bf((float)((int)(rnd() % 9) - 4));
        for (int f = 0; f < 16; ++f) bt.b(x, lane, f) = bf((float)((int)(rnd() % 9) - 4));
        uint32_t w = 0;
        for (int pr = 0; pr < 4; ++pr) {
          int i0 = rnd() & 3, i1 = rnd() & 3;
          if (mode == 0) {  // ascending, distinct
            while (i0 == i1) i1 = rnd() & 3;
            if (i0 > i1) std::swap(i0, i1);
          } else if (mode == 1) {
            i1 = i0;
          } else if (mode == 2) {  // descending, distinct
            while (i0 == i1) i1 = rnd() & 3;
            if (i0 < i1) std::swap(i0, i1);
          }
          if (field[0][2 * pr] >= 0 && field[0][2 * pr + 1] >= 0)
            w |= (uint32_t)i0 << (2 * field[0][2 * pr]) | (uint32_t)i1 << (2 * field[0][2 * pr + 1]);
        }
        w |= (rnd() & 0xffffu) << 16;  // the half that abid = 0 should ignore
        bt.idx[(size_t)x * 64 + lane] = w;
      }
    bt.run(0);
    int wrong = 0;
    for (int x = 0; x < N; ++x) {
      float ref[16][16] = {};
      for (int la = 0; la < 64; ++la)
        for (int e = 0; e < 8; ++e) {
          if (field[0][e] < 0) continue;
          const int v = (bt.idx[(size_t)x * 64 + la] >> (2 * field[0][e])) & 3;
          const Hit& h = T[la][e][v];
          if (!h.ok) continue;
          uint32_t au = (uint32_t)bt.a(x, la, e) << 16;
          float av;
          std::memcpy(&av, &au, 4);
          for (int n = 0; n < 16; ++n) {
            uint32_t bu = (uint32_t)bt.b(x, 16 * h.gB + n, h.f) << 16;
            float bv;
            std::memcpy(&bv, &bu, 4);
            ref[h.m][n] += av * bv;
          }
        }
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r)
          if (bt.c(x, lane, r) != ref[4 * (lane >> 4) + r][lane & 15]) ++wrong;
    }
    const char* mn[4] = {"ascending distinct", "equal", "descending distinct", "any"};
    std::printf("[check] random operands, index pairs %s: %d of %d outputs differ from the CPU product\n", mn[mode],
                wrong, N * 256);
  }
}

template <bool SPARSE>
static void rate_case(int grid, int block, int iters, double mhz) {
  float* out;
  long long* tk;
  const int waves = grid * block / 64;
  CK(hipMalloc(&out, (size_t)grid * block * 4));
  CK(hipMalloc(&tk, (size_t)waves * 8));
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  rate_kernel<SPARSE><<<grid, block>>>(out, tk, iters);  // warm-up
  CK(hipDeviceSynchronize());
  double best_ms = 1e30;
  std::vector<long long> h(waves);
  long long tmin = 0, tmax = 0;
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipEventRecord(a));
    rate_kernel<SPARSE><<<grid, block>>>(out, tk, iters);
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    if (ms < best_ms) {
      best_ms = ms;
      CK(hipMemcpy(h.data(), tk, (size_t)waves * 8, hipMemcpyDeviceToHost));
      tmin = tmax = h[0];
      for (long long v : h) {
        tmin = v < tmin ? v : tmin;
        tmax = v > tmax ? v : tmax;
      }
    }
  }
  const double n = 8.0 * iters;
  std::printf("[rate] %-6s grid %3d block %3d (%d wave/SIMD): s_memtime ticks per instruction and wave %.2f .. %.2f; "
              "event %.3f ms = %.2f ns per instruction and wave = %.1f cycles at %.0f MHz\n",
              SPARSE ? "sparse" : "dense", grid, block, block / 256, tmin / n, tmax / n, best_ms,
              best_ms * 1e6 / n, best_ms * 1e3 * mhz / n, mhz);
  CK(hipFree(out));
  CK(hipFree(tk));
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 20000;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const double mhz = prop.clockRate / 1000.0;
  std::printf("device %s, %d CUs, %.0f MHz\n", prop.gcnArchName, prop.multiProcessorCount, mhz);
  layout_probe();
  const int cus = prop.multiProcessorCount;
  for (int rep = 0; rep < 2; ++rep)
    for (int grid : {1, cus})
      for (int block : {256, 512}) {
        rate_case<false>(grid, block, iters, mhz);
        rate_case<true>(grid, block, iters, mhz);
      }
  return 0;
}
