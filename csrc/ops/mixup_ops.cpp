// Tensor-level wrappers for the mixup / cutmix kernels (csrc/kernels/mixup.hip).
#include <c10/core/DeviceGuard.h>

#include "../kernels/kernels.h"
#include "nn_ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

at::Tensor mix_draw(const at::Tensor& snapshot, int64_t R, int64_t H, int64_t W, double mixup_alpha,
                    double cutmix_alpha, double prob, double switch_prob) {
  gpu(snapshot, "mix_draw snapshot");
  dtype(snapshot, at::kLong, "mix_draw snapshot");
  RINGDP_CHECK(snapshot.numel() == 2, "mix_draw snapshot: expected the two int64 values of rng_tick");
  RINGDP_CHECK(R >= 1 && R < (int64_t(1) << 24), "mix_draw: the number of records must be in [1, 2^24), got ", R);
  RINGDP_CHECK(H >= 1 && W >= 1 && H * W < (int64_t(1) << 31), "mix_draw: bad image size ", H, " x ", W);
  RINGDP_CHECK(mixup_alpha >= 0.0 && cutmix_alpha >= 0.0, "mix_draw: alphas must not be negative");
  RINGDP_CHECK(prob >= 0.0 && prob <= 1.0 && switch_prob >= 0.0 && switch_prob <= 1.0,
               "mix_draw: prob and switch_prob must be in [0, 1]");
  c10::DeviceGuard guard(snapshot.device());
  at::Tensor rec = at::empty({R, 8}, snapshot.options().dtype(at::kInt));
  kern::MixDrawArgs a{};
  a.mixup_alpha = static_cast<float>(mixup_alpha);
  a.cutmix_alpha = static_cast<float>(cutmix_alpha);
  a.prob = static_cast<float>(prob);
  a.switch_prob = static_cast<float>(switch_prob);
  a.H = static_cast<int>(H);
  a.W = static_cast<int>(W);
  a.R = static_cast<int>(R);
  kern::mix_draw(reinterpret_cast<const uint64_t*>(snapshot.data_ptr<int64_t>()), a, rec.data_ptr<int32_t>(),
                 stream_of(snapshot));
  return rec;
}

std::tuple<at::Tensor, at::Tensor> mix_images(const at::Tensor& x, const at::Tensor& y, const at::Tensor& rec) {
  RINGDP_CHECK(x.defined() && x.is_cuda(), "mix_images x: expected a GPU tensor (ringdp HIP kernel)");
  RINGDP_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat,
               "mix_images x: expected bf16 or fp32, got ", c10::toString(x.scalar_type()));
  RINGDP_CHECK(x.dim() == 4, "mix_images x: expected [B, C, H, W], got ", x.sizes());
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const bool nchw = x.is_contiguous();
  RINGDP_CHECK(nchw || x.is_contiguous(at::MemoryFormat::ChannelsLast),
               "mix_images x: expected a contiguous NCHW or channels-last tensor");
  RINGDP_CHECK(B >= 1 && x.numel() > 0 && x.numel() < (int64_t(1) << 31),
               "mix_images x: between 1 and 2^31 - 1 elements, got ", x.numel());
  gpu(y, "mix_images y");
  dtype(y, at::kLong, "mix_images y");
  RINGDP_CHECK(y.dim() == 1 && y.size(0) == B, "mix_images y: expected ", B, " labels, got ", y.sizes());
  gpu(rec, "mix_images records");
  dtype(rec, at::kInt, "mix_images records");
  RINGDP_CHECK(rec.dim() == 2 && rec.size(1) == 8 && (rec.size(0) == 1 || rec.size(0) == B),
               "mix_images records: expected int32 [1, 8] or [", B, ", 8], got ", rec.sizes());
  RINGDP_CHECK(y.get_device() == x.get_device() && rec.get_device() == x.get_device(),
               "mix_images: tensors on different devices");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = at::empty_like(x);  // keeps the memory format; never in place
  at::Tensor y_b = at::empty_like(y);
  const int64_t sample = C * H * W, bytes = sample * x.element_size();
  const bool vec = bytes % 16 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0;
  // elem mode only when there is a record per sample and more than one sample; [1, 8] serves the whole batch
  kern::mix_images(x.data_ptr(), x.scalar_type() == at::kBFloat16, y.data_ptr<int64_t>(), rec.data_ptr<int32_t>(),
                   rec.size(0) > 1, B, sample, static_cast<int>(H), static_cast<int>(W),
                   nchw ? 1 : static_cast<int>(C), vec, out.data_ptr(), y_b.data_ptr<int64_t>(), stream_of(x));
  return {out, y_b};
}

}  // namespace ops
}  // namespace ringdp
