// Tensor-level wrappers for the depthwise convolution kernels (csrc/kernels/dwconv.hip).
#include <c10/core/DeviceGuard.h>

#include "../kernels/kernels.h"
#include "nn_ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

namespace {

// x: contiguous bf16 [N, H, W, C] with C % 8 == 0 on a 16-byte boundary (the kernels load 8 channels at a time)
void check_nhwc(const at::Tensor& x, const char* name) {
  bf16_gpu(x, name);
  RINGDP_CHECK(x.dim() == 4, name, ": expected NHWC bf16 [N, H, W, C], got ", x.sizes());
  RINGDP_CHECK(x.size(3) % 8 == 0, name, ": the channel count must be a multiple of 8, got ", x.size(3));
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name, ": expected 16-byte aligned data");
  // every tile holds at least one element, so the grids fit an int as well
  RINGDP_CHECK(x.numel() < (int64_t(1) << 31), name, ": tensor too large, ", x.sizes());
}

void check_k(int64_t K) { RINGDP_CHECK(kern::dwconv_ok((int)K), "dwconv: the kernel size must be 3, 5 or 7, got ", K); }

}  // namespace

at::Tensor dwconv_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, bool flip) {
  check_nhwc(x, "dwconv_fwd x");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  f32_gpu(w, "dwconv_fwd weight");
  RINGDP_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 1 && w.size(2) == w.size(3),
               "dwconv_fwd weight: expected fp32 [", C, ", 1, K, K], got ", w.sizes());
  const int64_t K = w.size(2);
  check_k(K);
  RINGDP_CHECK(w.get_device() == x.get_device(), "dwconv_fwd: tensors on different devices");
  const float* b = nullptr;
  if (bias.has_value() && bias->defined()) {
    f32_gpu(*bias, "dwconv_fwd bias");
    RINGDP_CHECK(bias->dim() == 1 && bias->size(0) == C && bias->get_device() == x.get_device(),
                 "dwconv_fwd bias: expected fp32 [", C, "] on the input's device, got ", bias->sizes());
    RINGDP_CHECK(reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0, "dwconv_fwd bias: expected 16-byte "
                 "aligned data");
    b = bias->data_ptr<float>();
  }
  c10::DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  kern::dwconv_fwd(x.data_ptr(), w.data_ptr<float>(), b, y.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)K, flip,
                   stream_of(x));
  // up to 70 KiB of LDS a workgroup: a launch the runtime refuses must not leave y unwritten without a word
  RINGDP_HIP_CHECK(hipGetLastError());
  return y;
}

std::tuple<at::Tensor, c10::optional<at::Tensor>> dwconv_wgrad(const at::Tensor& x, const at::Tensor& dy, int64_t K,
                                                               bool need_bias) {
  check_nhwc(x, "dwconv_wgrad x");
  check_nhwc(dy, "dwconv_wgrad dy");
  check_k(K);
  RINGDP_CHECK(dy.sizes() == x.sizes(), "dwconv_wgrad: dy ", dy.sizes(), " does not match x ", x.sizes());
  RINGDP_CHECK(dy.get_device() == x.get_device(), "dwconv_wgrad: tensors on different devices");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  c10::DeviceGuard guard(x.device());
  const auto f32 = x.options().dtype(at::kFloat);
  at::Tensor dw = at::empty({C, 1, K, K}, f32);
  c10::optional<at::Tensor> db;
  if (need_bias) db = at::empty({C}, f32);
  if (x.numel() == 0) {
    dw.zero_();
    if (need_bias) db->zero_();
    return {dw, db};
  }
  const int cus = num_cus(x);
  // scratch from the caching allocator (capturable); every element is written by the first launch
  at::Tensor partial = at::empty({kern::dwconv_wgrad_partial_floats((int)N, (int)H, (int)W, (int)C, (int)K, cus)}, f32);
  kern::dwconv_wgrad(x.data_ptr(), dy.data_ptr(), partial.data_ptr<float>(), dw.data_ptr<float>(),
                     need_bias ? db->data_ptr<float>() : nullptr, (int)N, (int)H, (int)W, (int)C, (int)K, cus,
                     stream_of(x));
  RINGDP_HIP_CHECK(hipGetLastError());
  return {dw, db};
}

}  // namespace ops
}  // namespace ringdp
