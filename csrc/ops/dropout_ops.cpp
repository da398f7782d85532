// Tensor-level wrappers for the dropout / stochastic-depth kernels (csrc/kernels/dropout.hip).
#include <c10/core/DeviceGuard.h>

#include "../kernels/kernels.h"
#include "nn_ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

namespace {

void check_rng_pair(const at::Tensor& t, const char* name) {
  RINGDP_CHECK(t.defined(), name, ": undefined tensor");
  RINGDP_CHECK(t.is_cuda(), name, ": expected a GPU tensor (ringdp HIP kernel), got ", t.device());
  dtype(t, at::kLong, name);
  RINGDP_CHECK(t.numel() == 2 && t.is_contiguous(), name, ": expected two contiguous int64 values");
}

// Element mode walks the flat tensor in groups of 8 (one 16-byte vector, one Philox call): rows must be whole
// vectors and every row 16-byte aligned.
void check_stream(const at::Tensor& t, const char* name) {
  bf16_gpu(t, name);
  RINGDP_CHECK(t.dim() >= 1 && t.size(-1) % 8 == 0, name, ": the last dimension must be a multiple of 8, got ",
               t.dim() >= 1 ? t.size(-1) : 0);
  RINGDP_CHECK(t.numel() < (int64_t(1) << 35), name, ": at most 2^35 - 1 elements (32-bit group counter), got ",
               t.numel());
  RINGDP_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, ": rows must be 16-byte aligned");
}

void check_site(int64_t site, int64_t thr, const char* name) {
  RINGDP_CHECK(site >= 0 && site <= 0xffffffffLL, name, ": site id out of range: ", site);
  RINGDP_CHECK(thr >= 0 && thr <= 65535, name, ": threshold must be in [0, 65535], got ", thr);
}

at::Tensor run(const at::Tensor& x, const at::Tensor* res, const c10::optional<at::Tensor>& snap, int64_t site_e,
               int64_t thr_e, int64_t site_r, int64_t thr_r, int64_t T, const char* name) {
  check_stream(x, name);
  check_site(site_e, thr_e, name);
  check_site(site_r, thr_r, name);
  if (res != nullptr) {
    check_stream(*res, "dropout_add residual");
    RINGDP_CHECK(res->sizes() == x.sizes() && res->get_device() == x.get_device(), name,
                 ": x and the residual must have one shape and device");
  }
  if (thr_e == 0 && thr_r == 0) return res != nullptr ? add_bf16(x, *res) : x;  // identity: nothing is drawn
  RINGDP_CHECK(snap.has_value(), name, ": a snapshot (rng_tick) is needed when a threshold is non-zero");
  const at::Tensor& snapshot = *snap;
  check_rng_pair(snapshot, "dropout snapshot");
  RINGDP_CHECK(snapshot.get_device() == x.get_device(), name, ": snapshot on another device");
  int64_t row_elems = 0;
  if (thr_r != 0) {
    const int64_t cols = x.size(-1), rows = x.numel() / std::max<int64_t>(cols, 1);
    RINGDP_CHECK(T > 0 && rows % T == 0, name, ": row mode needs T > 0 rows per sample dividing the ", rows,
                 " rows, got ", T);
    row_elems = T * cols;
  }
  at::Tensor y = at::empty_like(x);
  c10::DeviceGuard guard(x.device());
  kern::dropout_bf16(x.data_ptr(), res != nullptr ? res->data_ptr() : nullptr,
                     reinterpret_cast<const uint64_t*>(snapshot.data_ptr<int64_t>()), (uint32_t)site_e,
                     (uint32_t)thr_e, (uint32_t)site_r, (uint32_t)thr_r, row_elems, x.numel(), y.data_ptr(),
                     stream_of(x));
  return y;
}

}  // namespace

at::Tensor rng_tick(at::Tensor state) {
  check_rng_pair(state, "rng state");
  c10::DeviceGuard guard(state.device());
  at::Tensor snapshot = at::empty({2}, state.options());
  kern::rng_tick(reinterpret_cast<uint64_t*>(state.data_ptr<int64_t>()),
                 reinterpret_cast<uint64_t*>(snapshot.data_ptr<int64_t>()), stream_of(state));
  return snapshot;
}

at::Tensor dropout_bf16(const at::Tensor& x, const c10::optional<at::Tensor>& snapshot, int64_t site, int64_t thr,
                        int64_t site_r, int64_t thr_r, int64_t T) {
  return run(x, nullptr, snapshot, site, thr, site_r, thr_r, T, "dropout");
}

at::Tensor dropout_add_bf16(const at::Tensor& x, const at::Tensor& res, const c10::optional<at::Tensor>& snapshot,
                            int64_t site_e, int64_t thr_e, int64_t site_r, int64_t thr_r, int64_t T) {
  return run(x, &res, snapshot, site_e, thr_e, site_r, thr_r, T, "dropout_add");
}

}  // namespace ops
}  // namespace ringdp
