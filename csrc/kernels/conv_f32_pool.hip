// fp32 ConvNet: the ReLU + max-pool kernels, the fused head backward, and the host helpers of conv_f32_host.h
// (design: conv_f32_gemm.h, included here for FastDiv).
#include "conv_f32_gemm.h"

namespace ringdp::kern {

int f32_num_cus() {
  static const int n = [] {
    int dev = 0, v = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      v = 256;
    return v;
  }();
  return n;
}

bool is_convnet_conv2(const ConvF32Geom& g) {
  return g.Kout == 64 && g.C == 32 && g.R == 3 && g.pad == 0 && g.H == 13 && g.W == 13;
}
bool is_convnet_conv3(const ConvF32Geom& g) {
  return g.Kout == 128 && g.C == 64 && g.R == 3 && g.pad == 0 && g.H == 10 && g.W == 10;
}

int grid_1d(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return static_cast<int>(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// One element per thread for the pool kernels: their per-element loads are dependent (code, then
// gradient), so a grid-stride loop over a capped grid runs at one load round trip per iteration.
int grid_elems(int64_t n) { return static_cast<int>(std::max<int64_t>(1, (n + 255) / 256)); }

// Largest batch chunk whose per-chunk element counts (each listed per-image size) stay < 2^29, so
// every fp32 operand chunk is < 2^31 bytes: 32-bit buffer offsets, and kBadOff is out of range
// (RINGDP_F32_CHUNK_LIMIT lowers the bound: the tests run the chunked path at small batches).
int64_t batch_chunk(int64_t B, std::initializer_list<int64_t> per_image) {
  int64_t worst = 1;
  for (int64_t v : per_image) worst = std::max(worst, v);
  int64_t limit = (int64_t{1} << 29) - 1;
  if (const char* e = std::getenv("RINGDP_F32_CHUNK_LIMIT")) limit = std::max<int64_t>(1, std::min<int64_t>(limit, std::atoll(e)));
  const int64_t cap = limit / worst;
  return std::max<int64_t>(1, std::min(B, cap));
}

namespace {

// ---------------------------------------------------------------- pooling (+ReLU)
// a[bc, py, px] = relu(max over the k x k window at (py*st, px*st)); code = argmax offset
// (first maximum in row-major order, as max_pool2d); code 255 where the result is 0 (no gradient).
__global__ __launch_bounds__(256) void pool_relu_fwd_kernel(const float* __restrict__ z, float* __restrict__ a,
                                                            unsigned char* __restrict__ code, int total, int H,
                                                            int W, FastDiv fphw, FastDiv fpw, int k, int st) {
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < total;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    const int bc = fdiv(i, fphw), r = i - bc * static_cast<int>(fphw.d);
    const int py = fdiv(r, fpw), px = r - py * static_cast<int>(fpw.d);
    const float* zp = z + bc * H * W + (py * st) * W + px * st;
    float best = zp[0];
    int arg = 0;
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) {
        const float v = zp[dy * W + dx];
        if (v > best) { best = v; arg = dy * k + dx; }
      }
    const bool live = best > 0.f;
    a[i] = live ? best : 0.f;
    code[i] = live ? static_cast<unsigned char>(arg) : 255;
  }
}

// 2x2/s2 windows with an even input width: two 8-B row loads per window.
__global__ __launch_bounds__(256) void pool2s2_fwd_kernel(const float* __restrict__ z, float* __restrict__ a,
                                                          unsigned char* __restrict__ code, int total, int H,
                                                          int W, FastDiv fphw, FastDiv fpw) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= total) return;
  const int bc = fdiv(i, fphw), r = i - bc * static_cast<int>(fphw.d);
  const int py = fdiv(r, fpw), px = r - py * static_cast<int>(fpw.d);
  const float* zp = z + bc * H * W + (2 * py) * W + 2 * px;
  const float2 t = *reinterpret_cast<const float2*>(zp), b = *reinterpret_cast<const float2*>(zp + W);
  float best = t.x;
  int arg = 0;
  if (t.y > best) { best = t.y; arg = 1; }
  if (b.x > best) { best = b.x; arg = 2; }
  if (b.y > best) { best = b.y; arg = 3; }
  const bool live = best > 0.f;
  a[i] = live ? best : 0.f;
  code[i] = live ? static_cast<unsigned char>(arg) : 255;
}

// 2x2/s1 windows: the four loads issued together.
__global__ __launch_bounds__(256) void pool2s1_fwd_kernel(const float* __restrict__ z, float* __restrict__ a,
                                                          unsigned char* __restrict__ code, int total, int H,
                                                          int W, FastDiv fphw, FastDiv fpw) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= total) return;
  const int bc = fdiv(i, fphw), r = i - bc * static_cast<int>(fphw.d);
  const int py = fdiv(r, fpw), px = r - py * static_cast<int>(fpw.d);
  const float* zp = z + bc * H * W + py * W + px;
  const float v0 = zp[0], v1 = zp[1], v2 = zp[W], v3 = zp[W + 1];
  float best = v0;
  int arg = 0;
  if (v1 > best) { best = v1; arg = 1; }
  if (v2 > best) { best = v2; arg = 2; }
  if (v3 > best) { best = v3; arg = 3; }
  const bool live = best > 0.f;
  a[i] = live ? best : 0.f;
  code[i] = live ? static_cast<unsigned char>(arg) : 255;
}

// dz[bc, y, x] = sum over windows (py, px) covering (y, x) whose code points at (y, x) of da[bc, py, px]
__global__ __launch_bounds__(256) void pool_relu_bwd_kernel(const float* __restrict__ da,
                                                            const unsigned char* __restrict__ code,
                                                            float* __restrict__ dz, int total, FastDiv fhw,
                                                            FastDiv fw, int PH, int PW, int k, int st) {
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < total;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    const int bc = fdiv(i, fhw), r = i - bc * static_cast<int>(fhw.d);
    const int y = fdiv(r, fw), x = r - y * static_cast<int>(fw.d);
    float g = 0.f;
    for (int dy = 0; dy < k; ++dy) {
      const int ty = y - dy;
      if (ty < 0) break;
      const int py = ty / st;
      if (py * st != ty || py >= PH) continue;
      for (int dx = 0; dx < k; ++dx) {
        const int tx = x - dx;
        if (tx < 0) break;
        const int px = tx / st;
        if (px * st != tx || px >= PW) continue;
        const int o = bc * PH * PW + py * PW + px;
        if (code[o] == dy * k + dx) g += da[o];
      }
    }
    dz[i] = g;
  }
}

// Non-overlapping 2x2/s2 windows: one thread per window writes its 2x2 block (the gradient at the
// coded position, zeros elsewhere); a trailing odd row / column (no window covers it) is zeroed by
// the last window of the row / column.
__global__ __launch_bounds__(256) void pool2s2_bwd_kernel(const float* __restrict__ da,
                                                          const unsigned char* __restrict__ code,
                                                          float* __restrict__ dz, int total, FastDiv fphw,
                                                          FastDiv fpw, int H, int W) {
  const int PH = H / 2, PW = W / 2;
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < total;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    const int bc = fdiv(i, fphw), r = i - bc * static_cast<int>(fphw.d);
    const int py = fdiv(r, fpw), px = r - py * PW;
    const int c = code[i];
    const float g = da[i];
    float* o = dz + bc * H * W + 2 * py * W + 2 * px;
    const float2 top = make_float2(c == 0 ? g : 0.f, c == 1 ? g : 0.f);
    const float2 bot = make_float2(c == 2 ? g : 0.f, c == 3 ? g : 0.f);
    if ((W & 1) == 0) {
      *reinterpret_cast<float2*>(o) = top;
      *reinterpret_cast<float2*>(o + W) = bot;
    } else {
      o[0] = top.x; o[1] = top.y; o[W] = bot.x; o[W + 1] = bot.y;
      if (px == PW - 1) { o[2] = 0.f; o[W + 2] = 0.f; }
    }
    if ((H & 1) && py == PH - 1) {
      o[2 * W] = 0.f;
      o[2 * W + 1] = 0.f;
      if ((W & 1) && px == PW - 1) o[2 * W + 2] = 0.f;
    }
  }
}

// Overlapping 2x2/s1 windows: one thread per input position gathers the (up to) 4 windows covering it.
__global__ __launch_bounds__(256) void pool2s1_bwd_kernel(const float* __restrict__ da,
                                                          const unsigned char* __restrict__ code,
                                                          float* __restrict__ dz, int total, FastDiv fhw,
                                                          FastDiv fw, int PH, int PW) {
  for (int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); i < total;
       i += static_cast<int>(gridDim.x * blockDim.x)) {
    const int bc = fdiv(i, fhw), r = i - bc * static_cast<int>(fhw.d);
    const int y = fdiv(r, fw), x = r - y * static_cast<int>(fw.d);
    const int base = bc * PH * PW;
    // all 8 loads issued together (clamped in-plane addresses), then masked: one memory round trip
    int o[4];
    bool in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int py = y - (q >> 1), px = x - (q & 1);
      in[q] = static_cast<unsigned>(py) < static_cast<unsigned>(PH) && static_cast<unsigned>(px) < static_cast<unsigned>(PW);
      o[q] = base + min(max(py, 0), PH - 1) * PW + min(max(px, 0), PW - 1);
    }
    int c[4];
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c[q] = code[o[q]];
      v[q] = da[o[q]];
    }
    float g = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (in[q] && c[q] == q) g += v[q];
    dz[i] = g;
  }
}

// The same over tiles of 16 planes staged in LDS (16-B loads of da and the codes, coalesced stores of dz): the
// per-element form issues 8 scalar loads per output and ran at ~2.6 TB/s (conv2's pool2 backward at B=65536:
// 1.58 ms).  Needs PH * PW <= 128, PH * PW % 4 == 0 and a multiple of 16 planes (kP2Tile).
// CPH / CPW > 0: compile-time window grid (the ConvNet's 10 x 10: the output index divisions become multiplies)
template <int CPH, int CPW>
// slices > 1: da is the data-gradient GEMM's split-K planes (slices x plane floats), summed in slice order while the
// tile is staged - the same sums as slab_sum_kernel, without its launch and the da round trip
__global__ __launch_bounds__(256) void pool2s1_bwd_tile_kernel(const float* __restrict__ da,
                                                               const unsigned char* __restrict__ code,
                                                               float* __restrict__ dz, int ntiles, int PH_, int PW_,
                                                               int slices, int64_t plane) {
  const int PH = CPH > 0 ? CPH : PH_, PW = CPW > 0 ? CPW : PW_;
  __shared__ __attribute__((aligned(16))) float D[kP2Tile * 128];
  __shared__ __attribute__((aligned(16))) unsigned char Cd[kP2Tile * 128];
  const int tid = threadIdx.x, W = PW + 1, hw = (PH + 1) * W, phw = PH * PW;
  const int n4 = kP2Tile * phw / 4, n16 = kP2Tile * phw / 16, nout = kP2Tile * hw;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = (int64_t)t * kP2Tile;
    const float4* src = reinterpret_cast<const float4*>(da + p0 * phw);
    for (int e = tid; e < n4; e += 256) {
      float4 acc = src[e];
      for (int z = 1; z < slices; ++z) {
        const float4 v = reinterpret_cast<const float4*>(da + z * plane + p0 * phw)[e];
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
      reinterpret_cast<float4*>(D)[e] = acc;
    }
    const uint4* cs = reinterpret_cast<const uint4*>(code + p0 * phw);
    for (int e = tid; e < n16; e += 256) reinterpret_cast<uint4*>(Cd)[e] = cs[e];
    __syncthreads();
    float* out = dz + p0 * hw;
    for (int o = tid; o < nout; o += 256) {
      const int pl = o / hw, r = o - pl * hw, y = r / W, x = r - y * W;
      float g = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int py = y - (q >> 1), px = x - (q & 1);
        if (static_cast<unsigned>(py) < static_cast<unsigned>(PH) && static_cast<unsigned>(px) < static_cast<unsigned>(PW)) {
          const int i = pl * phw + py * PW + px;
          if (Cd[i] == q) g += D[i];
        }
      }
      out[o] = g;
    }
    __syncthreads();  // the tile is consumed before the next one is staged
  }
}

}  // namespace

void pool2s1_bwd_tile(const float* da, const unsigned char* code, float* dz, int ntiles, int PH, int PW, int slices,
                      int64_t plane, hipStream_t s) {
  const auto kernel = PH == 10 && PW == 10 ? pool2s1_bwd_tile_kernel<10, 10> : pool2s1_bwd_tile_kernel<0, 0>;
  hipLaunchKernelGGL(kernel, dim3(std::min(ntiles, 8 * f32_num_cus())), dim3(256), 0, s, da, code, dz, ntiles, PH, PW,
                     slices, plane);
}

void pool_relu_f32_fwd(const float* z, float* a, unsigned char* code, int64_t BC, int H, int W, int k, int st,
                       hipStream_t s) {
  const int PH = (H - k) / st + 1, PW = (W - k) / st + 1;
  const int64_t chunk = batch_chunk(BC, {static_cast<int64_t>(H) * W});
  for (int64_t c0 = 0; c0 < BC; c0 += chunk) {
    const int64_t nbc = std::min(chunk, BC - c0);
    const int total = static_cast<int>(nbc * PH * PW);
    if (k == 2 && (st == 1 || (st == 2 && (W & 1) == 0))) {
      hipLaunchKernelGGL(st == 2 ? pool2s2_fwd_kernel : pool2s1_fwd_kernel, dim3(grid_elems(total)), dim3(256), 0, s,
                         z + c0 * H * W, a + c0 * PH * PW, code + c0 * PH * PW, total, H, W, make_fdiv(PH * PW),
                         make_fdiv(PW));
      continue;
    }
    hipLaunchKernelGGL(pool_relu_fwd_kernel, dim3(grid_elems(total)), dim3(256), 0, s, z + c0 * H * W,
                       a + c0 * PH * PW, code + c0 * PH * PW, total, H, W, make_fdiv(PH * PW), make_fdiv(PW), k, st);
  }
}

// The fp32 ConvNet head backward at small batches (the whole-network cross-entropy node): the logits gradient
// (ce_bwd_kernel's expression, same bits) -> dl for fc1's weight gradient, fc1's data gradient
// da3[f] = sum_j dl[j] W[j][f] (an fmaf chain in j order) and pool3's backward (2x2/s2, code = dy*2+dx, 255 =
// no gradient) straight into dz3 [128][8][8] - one launch for the cross-entropy backward, fc1 data gradient and
// pool3 backward launches.  Workgroup = 256 features of one image; 8 per image.
__global__ __launch_bounds__(256) void fc_ce_pool3_bwd_f32_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ grad_out,
                                                                  const float* __restrict__ denom, int ignore_index,
                                                                  float eps, int reduction,
                                                                  const float* __restrict__ wfc,
                                                                  const unsigned char* __restrict__ code3,
                                                                  float* __restrict__ dl, float* __restrict__ dz3) {
  __shared__ float g[10];
  const int n = blockIdx.x >> 3, f = (blockIdx.x & 7) * 256 + threadIdx.x;
  if (threadIdx.x < 10) {
    const int c = threadIdx.x;
    const int64_t y = labels[n];
    float v = 0.f;
    if (y != ignore_index) {
      const float p = __expf(logits[n * 10 + c] - lse[n]);
      const float q = (c == y ? (1.f - eps) : 0.f) + eps / 10.f;
      v = (p - q) * (reduction == 0 ? grad_out[n] : grad_out[0] / denom[0]);
    }
    g[c] = v;
    if ((blockIdx.x & 7) == 0) dl[n * 10 + c] = v;
  }
  __syncthreads();
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 10; ++j) a = fmaf(g[j], wfc[j * 2048 + f], a);
  const int code = code3[n * 2048 + f];
  const int c = f >> 4, py = (f >> 2) & 3, px = f & 3;
  float* o = dz3 + (int64_t)n * 8192 + c * 64 + 2 * py * 8 + 2 * px;
  *reinterpret_cast<float2*>(o) = make_float2(code == 0 ? a : 0.f, code == 1 ? a : 0.f);
  *reinterpret_cast<float2*>(o + 8) = make_float2(code == 2 ? a : 0.f, code == 3 ? a : 0.f);
}

void fc_ce_pool3_bwd_f32(const float* logits, const int64_t* labels, const float* lse, const float* grad_out,
                         const float* denom, int ignore_index, float eps, int reduction, const float* wfc,
                         const unsigned char* code3, int B, float* dl, float* dz3, hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(fc_ce_pool3_bwd_f32_kernel, dim3(8 * B), dim3(256), 0, s, logits, labels, lse, grad_out, denom,
                     ignore_index, eps, reduction, wfc, code3, dl, dz3);
}

void pool_relu_f32_bwd(const float* da, const unsigned char* code, float* dz, int64_t BC, int H, int W, int k,
                       int st, hipStream_t s) {
  const int PH = (H - k) / st + 1, PW = (W - k) / st + 1;
  const int64_t chunk = batch_chunk(BC, {static_cast<int64_t>(H) * W});
  for (int64_t c0 = 0; c0 < BC; c0 += chunk) {
    const int64_t nbc = std::min(chunk, BC - c0);
    const int total = static_cast<int>(nbc * H * W);
    if (k == 2 && st == 2) {
      const int wins = static_cast<int>(nbc * PH * PW);
      hipLaunchKernelGGL(pool2s2_bwd_kernel, dim3(grid_elems(wins)), dim3(256), 0, s, da + c0 * PH * PW,
                         code + c0 * PH * PW, dz + c0 * H * W, wins, make_fdiv(PH * PW), make_fdiv(PW), H, W);
      continue;
    }
    if (k == 2 && st == 1 && PH * PW <= 128 && (PH * PW) % 4 == 0 && nbc % kP2Tile == 0) {
      pool2s1_bwd_tile(da + c0 * PH * PW, code + c0 * PH * PW, dz + c0 * H * W, static_cast<int>(nbc / kP2Tile), PH, PW,
                       1, 0, s);
      continue;
    }
    if (k == 2 && st == 1) {
      hipLaunchKernelGGL(pool2s1_bwd_kernel, dim3(grid_elems(total)), dim3(256), 0, s, da + c0 * PH * PW,
                         code + c0 * PH * PW, dz + c0 * H * W, total, make_fdiv(H * W), make_fdiv(W), PH, PW);
      continue;
    }
    hipLaunchKernelGGL(pool_relu_bwd_kernel, dim3(grid_elems(total)), dim3(256), 0, s, da + c0 * PH * PW,
                       code + c0 * PH * PW, dz + c0 * H * W, total, make_fdiv(H * W), make_fdiv(W), PH, PW, k, st);
  }
}

}  // namespace ringdp::kern
