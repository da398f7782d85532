// Tensor-level wrappers for the MXFP8 quantiser, GEMM and LayerNorms (csrc/kernels/mxfp8.hip, gemm_mxfp8_256.hip,
// layernorm_mx.hip, layernorm_bwd_mx.hip).
#include <c10/core/DeviceGuard.h>

#include <algorithm>

#include "../kernels/kernels.h"
#include "nn_ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

namespace {

void mx_source(const at::Tensor& x, const char* name) {
  gpu(x, name);
  RINGDP_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, name,
               ": expected bf16 or fp32, got ", c10::toString(x.scalar_type()));
  RINGDP_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 32 && x.size(1) % 32 == 0, name,
               ": expected [rows >= 1, cols % 32 == 0], got ", x.sizes());
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name, ": expected a 16-B aligned tensor");
}

uint8_t* u8(const at::Tensor& t) { return static_cast<uint8_t*>(t.data_ptr()); }

// e4m3 operand [rows][K] and its E8M0 scales [rows][K / 32]
void mx_operand(const at::Tensor& a, const at::Tensor& s, int64_t rows, int64_t K, const char* name) {
  gpu(a, name);
  gpu(s, name);
  dtype(a, at::kByte, name);
  dtype(s, at::kByte, name);
  RINGDP_CHECK(a.numel() >= rows * K && s.numel() >= rows * (K / 32), name, ": operand or scales smaller than [",
               rows, ", ", K, "] describes");
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(s.data_ptr()) % 4 == 0,
               name, ": expected 16-B aligned elements and 4-B aligned scales");
}

void mx_gemm_dims(int64_t M, int64_t N, int64_t K, const char* name) {
  RINGDP_CHECK(M >= 1 && N >= 4 && N % 4 == 0 && K >= 128 && K % 128 == 0, name,
               ": expected M >= 1, N % 4 == 0 and the padded K % 128 == 0, got ", M, ", ", N, ", ", K);
  // (the kernel addresses a tile's 256 rows x K bytes with 32-bit lane offsets)
  RINGDP_CHECK(M < (int64_t(1) << 31) - 256 && N < (int64_t(1) << 31) - 256 && K < (int64_t(1) << 24), name,
               ": dimension too large");
}

}  // namespace

std::tuple<c10::optional<at::Tensor>, c10::optional<at::Tensor>, c10::optional<at::Tensor>, c10::optional<at::Tensor>>
mx_quantize(const at::Tensor& x, bool rowwise, bool colwise) {
  mx_source(x, "mx_quantize input");
  RINGDP_CHECK(rowwise || colwise, "mx_quantize: neither orientation requested");
  c10::DeviceGuard guard(x.device());
  const int64_t R = x.size(0), Cc = x.size(1), Rp = kern::mx_pad(R), Cp = kern::mx_pad(Cc);
  const auto o = x.options().dtype(at::kByte);
  c10::optional<at::Tensor> q, s, qt, st;
  if (rowwise) {
    q = at::empty({R, Cp}, o);
    s = at::empty({R, Cp / 32}, o);
  }
  if (colwise) {
    qt = at::empty({Cc, Rp}, o);
    st = at::empty({Cc, Rp / 32}, o);
  }
  kern::mx_quantize(x.data_ptr(), x.scalar_type() == at::kFloat, R, Cc, rowwise ? u8(*q) : nullptr,
                    rowwise ? u8(*s) : nullptr, colwise ? u8(*qt) : nullptr, colwise ? u8(*st) : nullptr, stream_of(x));
  return {q, s, qt, st};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>, c10::optional<at::Tensor>> layernorm_fwd_mx(
    const at::Tensor& x, const at::Tensor& w, const at::Tensor& b, double eps, bool colwise) {
  gpu(x, "layernorm_fwd_mx input");
  dtype(x, at::kBFloat16, "layernorm_fwd_mx input");
  RINGDP_CHECK(x.dim() == 2 && x.is_contiguous() && x.size(0) >= 1, "layernorm_fwd_mx input: expected contiguous [rows >= 1, D], got ",
               x.sizes());
  const int64_t rows = x.size(0), D = x.size(1);
  RINGDP_CHECK(D % 32 == 0 && D >= 32 && D <= 2048, "layernorm_fwd_mx: expected D % 32 == 0 and 32 <= D <= 2048, got ", D);
  RINGDP_CHECK(rows < (int64_t(1) << 31) - 128, "layernorm_fwd_mx: too many rows");
  f32_gpu(w, "layernorm_fwd_mx weight");
  f32_gpu(b, "layernorm_fwd_mx bias");
  RINGDP_CHECK(w.numel() == D && b.numel() == D && w.is_contiguous() && b.is_contiguous() &&
                   w.get_device() == x.get_device() && b.get_device() == x.get_device(),
               "layernorm_fwd_mx: weight and bias must be contiguous [D] on the input's device");
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "layernorm_fwd_mx input: expected a 16-B aligned tensor");
  c10::DeviceGuard guard(x.device());
  const int64_t Rp = kern::mx_pad(rows), Cp = kern::mx_pad(D);
  const auto o = x.options().dtype(at::kByte);
  at::Tensor stats = at::empty({rows, 2}, w.options());
  // (at::empty: the kernel writes every byte, padding included)
  at::Tensor q = at::empty({rows, Cp}, o), s = at::empty({rows, Cp / 32}, o);
  c10::optional<at::Tensor> qt, st;
  if (colwise) {
    qt = at::empty({D, Rp}, o);
    st = at::empty({D, Rp / 32}, o);
  }
  kern::layernorm_fwd_mx(x.data_ptr(), w.data_ptr<float>(), b.data_ptr<float>(), rows, (int)D, (float)eps,
                         stats.data_ptr<float>(), u8(q), u8(s), colwise ? u8(*qt) : nullptr, colwise ? u8(*st) : nullptr,
                         stream_of(x));
  // with colwise the kernel takes 64 * D bytes of dynamic LDS (128 KiB at D = 2048): a launch the runtime refuses
  // must not leave the outputs unwritten without a word
  RINGDP_HIP_CHECK(hipGetLastError());
  return {stats, q, s, qt, st};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>, c10::optional<at::Tensor>,
           c10::optional<at::Tensor>>
layernorm_bwd_mx(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& stats, const at::Tensor& w,
                 const c10::optional<at::Tensor>& dres, at::Tensor dw, at::Tensor db, bool colwise) {
  bf16_gpu(dy, "layernorm_bwd_mx output grad");
  bf16_gpu(x, "layernorm_bwd_mx input");
  f32_gpu(stats, "layernorm_bwd_mx stats");
  f32_gpu(w, "layernorm_bwd_mx weight");
  f32_gpu(dw, "layernorm_bwd_mx dweight");
  f32_gpu(db, "layernorm_bwd_mx dbias");
  RINGDP_CHECK(x.dim() >= 1 && x.numel() >= 1, "layernorm_bwd_mx input: expected [rows >= 1, D], got ", x.sizes());
  const int64_t D = x.size(-1), rows = x.numel() / D;
  RINGDP_CHECK(dy.sizes() == x.sizes(), "layernorm_bwd_mx: shape mismatch");
  RINGDP_CHECK(D % 32 == 0 && D >= 32 && D <= 2048, "layernorm_bwd_mx: expected D % 32 == 0 and 32 <= D <= 2048, got ", D);
  RINGDP_CHECK(rows < (int64_t(1) << 31) - 128, "layernorm_bwd_mx: too many rows");
  RINGDP_CHECK(w.numel() == D && dw.numel() == D && db.numel() == D, "layernorm_bwd_mx: w / dw / db must hold D floats");
  RINGDP_CHECK(stats.numel() == 2 * rows, "layernorm_bwd_mx: stats must hold (mean, rstd) per row");
  const int dev = x.get_device();
  RINGDP_CHECK(dy.get_device() == dev && stats.get_device() == dev && w.get_device() == dev &&
                   dw.get_device() == dev && db.get_device() == dev,
               "layernorm_bwd_mx: tensors on different devices");
  const void* dr = nullptr;
  if (dres.has_value() && dres->defined()) {
    bf16_gpu(*dres, "layernorm_bwd_mx residual grad");
    RINGDP_CHECK(dres->sizes() == x.sizes() && dres->get_device() == dev, "layernorm_bwd_mx residual grad: shape mismatch");
    dr = dres->data_ptr();
  }
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(dr) % 16 == 0,
               "layernorm_bwd_mx: expected 16-B aligned tensors");
  c10::DeviceGuard guard(x.device());
  const int64_t Rp = kern::mx_pad(rows), Cp = kern::mx_pad(D);
  const auto o = x.options().dtype(at::kByte);
  at::Tensor dx = at::empty_like(x);
  // (at::empty: the kernel writes every byte, padding included)
  at::Tensor q = at::empty({rows, Cp}, o), s = at::empty({rows, Cp / 32}, o);
  c10::optional<at::Tensor> qt, st, cs;
  if (colwise) {
    qt = at::empty({D, Rp}, o);
    st = at::empty({D, Rp / 32}, o);
    cs = at::empty({kern::layernorm_bwd_mx_bands(rows), D}, w.options());
  }
  at::Tensor scratch = at::empty({kern::layernorm_bwd_mx_scratch_floats(rows, (int)D)}, w.options());
  kern::layernorm_bwd_mx(dy.data_ptr(), x.data_ptr(), stats.data_ptr<float>(), w.data_ptr<float>(), dr, rows, (int)D,
                         dx.data_ptr(), u8(q), u8(s), colwise ? u8(*qt) : nullptr, colwise ? u8(*st) : nullptr,
                         colwise ? cs->data_ptr<float>() : nullptr, scratch.data_ptr<float>(), dw.data_ptr<float>(),
                         db.data_ptr<float>(), stream_of(x));
  // 64 * D bytes of dynamic LDS (128 KiB at D = 2048): a launch the runtime refuses must not leave the outputs
  // unwritten without a word
  RINGDP_HIP_CHECK(hipGetLastError());
  return {dx, q, s, qt, st, cs};
}

std::vector<at::Tensor> mx_quantize_weights(const std::vector<at::Tensor>& ws) {
  RINGDP_CHECK(!ws.empty(), "mx_quantize_weights: no weights");
  c10::DeviceGuard guard(ws[0].device());
  std::vector<at::Tensor> out;
  kern::MxQuantTable t{};
  auto flush = [&] {
    kern::mx_quantize_multi(t, stream_of(ws[0]));
    t = kern::MxQuantTable{};
  };
  for (const at::Tensor& w : ws) {
    mx_source(w, "mx_quantize_weights weight");
    dtype(w, at::kFloat, "mx_quantize_weights weight");
    RINGDP_CHECK(w.get_device() == ws[0].get_device(), "mx_quantize_weights: weights on different devices");
    const int64_t R = w.size(0), Cc = w.size(1), Rp = kern::mx_pad(R), Cp = kern::mx_pad(Cc);
    const auto o = w.options().dtype(at::kByte);
    at::Tensor q = at::empty({R, Cp}, o), s = at::empty({R, Cp / 32}, o);
    at::Tensor qt = at::empty({Cc, Rp}, o), st = at::empty({Cc, Rp / 32}, o);
    out.insert(out.end(), {q, s, qt, st});
    if (t.n == kern::kMxQuantMax) flush();
    kern::MxQuantEntry& e = t.e[t.n++];
    e.src = w.data_ptr<float>();
    e.rows = R;
    e.cols = Cc;
    e.q = u8(q);
    e.s = u8(s);
    e.qt = u8(qt);
    e.st = u8(st);
    e.tile0 = t.total_tiles;
    t.total_tiles += (int)kern::mx_quant_tiles(R, Cc);
  }
  flush();
  return out;
}

at::Tensor gemm_mxfp8(const at::Tensor& a, const at::Tensor& sa, const at::Tensor& b, const at::Tensor& sb, int64_t M,
                      int64_t N, int64_t K, bool out_bf16, const c10::optional<at::Tensor>& bias, int64_t act,
                      const c10::optional<at::Tensor>& residual, const c10::optional<at::Tensor>& preact) {
  mx_gemm_dims(M, N, K, "gemm_mxfp8");
  mx_operand(a, sa, M, K, "gemm_mxfp8 A");
  mx_operand(b, sb, N, K, "gemm_mxfp8 B");
  RINGDP_CHECK(act == 0 || act == 1 || act == 2, "gemm_mxfp8: act must be 0, 1 (ReLU) or 2 (GELU)");
  c10::DeviceGuard guard(a.device());
  at::Tensor c = at::empty({M, N}, a.options().dtype(out_bf16 ? at::kBFloat16 : at::kFloat));
  kern::GemmEpilogue e{};
  e.mode = kern::GemmEpilogue::kStore;
  e.C = c.data_ptr();
  e.ldc = N;
  e.out_bf16 = out_bf16;
  e.alpha = 1.f;
  e.act = static_cast<int>(act);
  if (bias.has_value() && bias->defined()) {
    f32_gpu(*bias, "gemm_mxfp8 bias");
    RINGDP_CHECK(bias->numel() == N && reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0,
                 "gemm_mxfp8 bias: expected [N] floats, 16-B aligned");
    e.bias = bias->data_ptr<float>();
  }
  if (residual.has_value() && residual->defined()) {
    bf16_gpu(*residual, "gemm_mxfp8 residual");
    RINGDP_CHECK(residual->numel() == M * N, "gemm_mxfp8 residual: expected [M][N]");
    e.residual = residual->data_ptr();
  }
  if (preact.has_value() && preact->defined()) {
    bf16_gpu(*preact, "gemm_mxfp8 preact");
    RINGDP_CHECK(preact->numel() == M * N, "gemm_mxfp8 preact: expected [M][N]");
    e.preact = preact->data_ptr();
  }
  kern::gemm_mxfp8_256(u8(a), u8(sa), u8(b), u8(sb), (int)M, (int)N, (int)K, e, 1, stream_of(a));
  return c;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> gemm_mxfp8_quant_out(
    const at::Tensor& a, const at::Tensor& sa, const at::Tensor& b, const at::Tensor& sb, int64_t M, int64_t N,
    int64_t K, const c10::optional<at::Tensor>& bias, int64_t act, const c10::optional<at::Tensor>& preact,
    const c10::optional<at::Tensor>& colsum) {
  mx_gemm_dims(M, N, K, "gemm_mxfp8_quant_out");
  RINGDP_CHECK(N % 32 == 0, "gemm_mxfp8_quant_out: N must hold whole blocks of 32, got ", N);
  mx_operand(a, sa, M, K, "gemm_mxfp8_quant_out A");
  mx_operand(b, sb, N, K, "gemm_mxfp8_quant_out B");
  RINGDP_CHECK(act == 0 || act == 2 || act == 3,
               "gemm_mxfp8_quant_out: act must be 0, 2 (GELU) or 3 (GELU backward)");
  c10::DeviceGuard guard(a.device());
  kern::GemmEpilogue e{};
  e.mode = kern::GemmEpilogue::kStore;
  e.ldc = N;  // of preact: the values themselves never reach memory
  e.out_bf16 = true;
  e.alpha = 1.f;
  e.act = static_cast<int>(act);
  if (bias.has_value() && bias->defined()) {
    f32_gpu(*bias, "gemm_mxfp8_quant_out bias");
    RINGDP_CHECK(bias->numel() == N && reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0,
                 "gemm_mxfp8_quant_out bias: expected [N] floats, 16-B aligned");
    e.bias = bias->data_ptr<float>();
  }
  const bool has_pre = preact.has_value() && preact->defined();
  RINGDP_CHECK(has_pre == (act != 0), "gemm_mxfp8_quant_out: act 2 writes and act 3 reads preact; act 0 takes none");
  if (has_pre) {
    bf16_gpu(*preact, "gemm_mxfp8_quant_out preact");
    RINGDP_CHECK(preact->numel() == M * N && preact->is_contiguous() &&
                     reinterpret_cast<uintptr_t>(preact->data_ptr()) % 8 == 0,
                 "gemm_mxfp8_quant_out preact: expected contiguous [M][N], 8-B aligned");
    e.preact = preact->data_ptr();
  }
  const int64_t Mp = kern::mx_pad(M), Np = kern::mx_pad(N);
  // (torch.empty: the kernel writes every byte, padding included)
  at::Tensor q = at::empty({M, Np}, a.options()), s = at::empty({M, Np / 32}, a.options());
  at::Tensor qt = at::empty({N, Mp}, a.options()), st = at::empty({N, Mp / 32}, a.options());
  e.mx_q = u8(q);
  e.mx_s = u8(s);
  e.mx_qt = u8(qt);
  e.mx_st = u8(st);
  at::Tensor part;
  if (colsum.has_value() && colsum->defined()) {
    f32_gpu(*colsum, "gemm_mxfp8_quant_out colsum");
    RINGDP_CHECK(colsum->numel() == N && colsum->is_contiguous(), "gemm_mxfp8_quant_out colsum: expected [N] floats");
    part = at::empty({Mp / 128, N}, colsum->options());  // one partial row per 128-row wave tile
    e.colsum_part = part.data_ptr<float>();
  }
  const int used = kern::gemm_mxfp8_256(u8(a), u8(sa), u8(b), u8(sb), (int)M, (int)N, (int)K, e, 1, stream_of(a));
  RINGDP_CHECK(used == 1, "gemm_mxfp8_quant_out: the MXFP8-output kernel was not launched");
  if (part.defined())
    kern::rowsum_f32(part.data_ptr<float>(), (int)part.size(0), N, colsum->data_ptr<float>(), stream_of(a));
  return {q, s, qt, st};
}

void gemm_mxfp8_splitk_f32(const at::Tensor& a, const at::Tensor& sa, const at::Tensor& b, const at::Tensor& sb,
                           int64_t M, int64_t N, int64_t K, int64_t splits, at::Tensor out) {
  mx_gemm_dims(M, N, K, "gemm_mxfp8_splitk_f32");
  mx_operand(a, sa, M, K, "gemm_mxfp8_splitk_f32 A");
  mx_operand(b, sb, N, K, "gemm_mxfp8_splitk_f32 B");
  f32_gpu(out, "gemm_mxfp8_splitk_f32 out");
  RINGDP_CHECK(out.numel() == M * N, "gemm_mxfp8_splitk_f32 out: expected M * N floats");
  c10::DeviceGuard guard(a.device());
  splits = std::max<int64_t>(1, std::min<int64_t>(splits, K / 128));
  splits = kern::gemm_fp8_pick_splits((int)M, (int)N, (int)K, (int)splits);  // whole CU rounds of 256 x 256 tiles
  at::Tensor part = at::empty({splits, M, N}, out.options());
  kern::GemmEpilogue e{};
  e.mode = kern::GemmEpilogue::kSplitK;
  e.partial = part.data_ptr<float>();
  const int used = kern::gemm_mxfp8_256(u8(a), u8(sa), u8(b), u8(sb), (int)M, (int)N, (int)K, e, (int)splits, stream_of(a));
  kern::splitk_sum(part.data_ptr<float>(), used, M * N, out.data_ptr<float>(), stream_of(a));
}

}  // namespace ops
}  // namespace ringdp
