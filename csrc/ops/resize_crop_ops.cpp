// Tensor-level wrappers for the random-resized-crop / resize kernels (csrc/kernels/resize_crop.hip).
#include <c10/core/DeviceGuard.h>

#include <cmath>

#include "../kernels/kernels.h"
#include "nn_ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

namespace {

void check_range(const Range& r, const char* name) {
  RINGDP_CHECK(std::isfinite(r.first) && std::isfinite(r.second) && r.first > 0.0 && r.first <= r.second, name,
               ": expected 0 < lo <= hi, got (", r.first, ", ", r.second, ")");
}

}  // namespace

at::Tensor crop_draw(const at::Tensor& snapshot, int64_t R, int64_t H, int64_t W, int64_t S,
                     const c10::optional<Range>& scale, Range ratio, bool hflip, double erase_prob, Range erase_scale,
                     Range erase_ratio) {
  gpu(snapshot, "crop_draw snapshot");
  dtype(snapshot, at::kLong, "crop_draw snapshot");
  RINGDP_CHECK(snapshot.numel() == 2, "crop_draw snapshot: expected the two int64 values of rng_tick");
  RINGDP_CHECK(R >= 1 && R < (int64_t(1) << 24), "crop_draw: the number of records must be in [1, 2^24), got ", R);
  RINGDP_CHECK(H >= 1 && W >= 1 && H * W <= kern::kResizeMaxSourceBytes, "crop_draw: bad source size ", H, " x ", W);
  RINGDP_CHECK(S >= 1 && S <= kern::kResizeMaxSize, "crop_draw: the output size must be in [1, ",
               kern::kResizeMaxSize, "], got ", S);
  if (scale.has_value()) {
    check_range(*scale, "crop_draw scale");
    RINGDP_CHECK(scale->second <= 1.0, "crop_draw scale: an area fraction cannot exceed 1, got ", scale->second);
  }
  check_range(ratio, "crop_draw ratio");
  RINGDP_CHECK(erase_prob >= 0.0 && erase_prob <= 1.0, "crop_draw: erase_prob must be in [0, 1], got ", erase_prob);
  check_range(erase_scale, "crop_draw erase_scale");
  RINGDP_CHECK(erase_scale.second <= 1.0, "crop_draw erase_scale: an area fraction cannot exceed 1");
  check_range(erase_ratio, "crop_draw erase_ratio");
  c10::DeviceGuard guard(snapshot.device());
  at::Tensor rec = at::empty({R, 8}, snapshot.options().dtype(at::kInt));
  kern::CropDrawArgs a{};
  a.R = static_cast<int>(R);
  a.H = static_cast<int>(H);
  a.W = static_cast<int>(W);
  a.S = static_cast<int>(S);
  a.crop = scale.has_value() ? 1 : 0;
  a.hflip = hflip ? 1 : 0;
  a.scale0 = static_cast<float>(scale.has_value() ? scale->first : 1.0);
  a.scale1 = static_cast<float>(scale.has_value() ? scale->second : 1.0);
  a.ratio0 = static_cast<float>(ratio.first);
  a.ratio1 = static_cast<float>(ratio.second);
  a.erase_prob = static_cast<float>(erase_prob);
  a.escale0 = static_cast<float>(erase_scale.first);
  a.escale1 = static_cast<float>(erase_scale.second);
  a.eratio0 = static_cast<float>(erase_ratio.first);
  a.eratio1 = static_cast<float>(erase_ratio.second);
  kern::crop_draw(reinterpret_cast<const uint64_t*>(snapshot.data_ptr<int64_t>()), a, rec.data_ptr<int32_t>(),
                  stream_of(snapshot));
  return rec;
}

std::tuple<at::Tensor, at::Tensor> resize_crop(const at::Tensor& x, const c10::optional<at::Tensor>& labels,
                                               const at::Tensor& idx, const at::Tensor& rec, int64_t S,
                                               std::vector<double> mean, std::vector<double> std, bool channels_last,
                                               at::ScalarType out_dtype) {
  gpu(x, "resize_crop dataset images");
  dtype(x, at::kByte, "resize_crop dataset images");
  RINGDP_CHECK(x.dim() == 3 || x.dim() == 4, "resize_crop dataset images: expected uint8 [N, H, W] or [N, H, W, C], "
               "got ", x.sizes());
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.dim() == 4 ? x.size(3) : 1;
  RINGDP_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= 4, "resize_crop dataset images: at least one image of "
               "1 to 4 channels, got ", x.sizes());
  RINGDP_CHECK(H * W * C <= kern::kResizeMaxSourceBytes, "resize_crop: a source image of ", H, " x ", W, " x ", C,
               " bytes does not fit the kernel's LDS stage (at most ", kern::kResizeMaxSourceBytes, ")");
  RINGDP_CHECK(S >= 1 && S <= kern::kResizeMaxSize, "resize_crop: the output size must be in [1, ",
               kern::kResizeMaxSize, "], got ", S);
  gpu(idx, "resize_crop batch indices");
  dtype(idx, at::kLong, "resize_crop batch indices");
  RINGDP_CHECK(idx.dim() == 1, "resize_crop batch indices: expected 1-D int64, got ", idx.sizes());
  const int64_t B = idx.size(0);
  RINGDP_CHECK(B * ((S + 31) / 32) < (int64_t(1) << 31), "resize_crop: batch too large, ", B);
  gpu(rec, "resize_crop records");
  dtype(rec, at::kInt, "resize_crop records");
  RINGDP_CHECK(rec.dim() == 2 && rec.size(1) == 8 && (rec.size(0) == 1 || rec.size(0) == B),
               "resize_crop records: expected int32 [1, 8] or [", B, ", 8], got ", rec.sizes());
  RINGDP_CHECK(idx.get_device() == x.get_device() && rec.get_device() == x.get_device(),
               "resize_crop: tensors on different devices");
  RINGDP_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16,
               "resize_crop: out dtype must be float32 or bfloat16, got ", c10::toString(out_dtype));
  RINGDP_CHECK(mean.size() <= 4 && std.size() <= 4, "resize_crop: at most 4 mean / std values");
  kern::AugNorm nrm{};
  for (int c = 0; c < 4; ++c) {
    const double m = mean.empty() ? 0.0 : mean[std::min<size_t>(c, mean.size() - 1)];
    const double sd = std.empty() ? 1.0 : std[std::min<size_t>(c, std.size() - 1)];
    RINGDP_CHECK(sd != 0.0, "resize_crop: std must be non-zero");
    nrm.mean[c] = static_cast<float>(m);
    nrm.inv_std[c] = static_cast<float>(1.0 / sd);
  }
  const int64_t* lab = nullptr;
  if (labels.has_value() && labels->defined()) {
    gpu(*labels, "resize_crop dataset labels");
    dtype(*labels, at::kLong, "resize_crop dataset labels");
    RINGDP_CHECK(labels->dim() == 1 && labels->size(0) == N && labels->get_device() == x.get_device(),
                 "resize_crop dataset labels: expected ", N, " labels on the images' device, got ", labels->sizes());
    lab = labels->data_ptr<int64_t>();
  }
  c10::DeviceGuard guard(x.device());
  auto opt = x.options().dtype(out_dtype);
  at::Tensor out = at::empty({B, C, S, S}, channels_last ? opt.memory_format(at::MemoryFormat::ChannelsLast) : opt);
  at::Tensor y;
  if (lab) y = at::empty({B}, labels->options());
  if (B == 0) return {out, y};
  kern::resize_crop(x.data_ptr<uint8_t>(), lab, idx.data_ptr<int64_t>(), rec.data_ptr<int32_t>(), rec.size(0) > 1,
                    static_cast<int>(B), N, static_cast<int>(H), static_cast<int>(W), static_cast<int>(C),
                    static_cast<int>(S), nrm, channels_last, out_dtype == at::kBFloat16, out.data_ptr(),
                    lab ? y.data_ptr<int64_t>() : nullptr, stream_of(x));
  return {out, y};
}

}  // namespace ops
}  // namespace ringdp
