// Tensor-level wrappers for the LR-schedule and model-EMA kernels (csrc/kernels/sched_ema.hip).
#include <c10/core/DeviceGuard.h>

#include "../kernels/kernels.h"
#include "ops.h"
#include "util.h"

namespace ringdp {
namespace ops {

using namespace util;

namespace {

bool aligned16(const at::Tensor& t) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0; }

// A one-element device scalar of the given dtype.
void scalar_gpu(const at::Tensor& t, at::ScalarType d, const char* name) {
  gpu(t, name);
  dtype(t, d, name);
  RINGDP_CHECK(t.numel() == 1, name, ": expected one element, got ", t.numel());
}

}  // namespace

void lr_sched_run(at::Tensor counter, const LrSchedSpec& spec, const std::vector<double>& base_lrs,
                  std::vector<at::Tensor> lr_tensors, bool advance) {
  scalar_gpu(counter, at::kLong, "lr_sched counter");
  const size_t G = lr_tensors.size();
  RINGDP_CHECK(G >= 1 && G <= static_cast<size_t>(kern::kAdamMaxGroups), "lr_sched: between 1 and ",
               kern::kAdamMaxGroups, " parameter groups per launch, got ", G);
  RINGDP_CHECK(base_lrs.size() == G, "lr_sched: one base lr per lr tensor");
  RINGDP_CHECK(spec.kind >= kern::kSchedConstant && spec.kind <= kern::kSchedMultiStep, "lr_sched: unknown kind ",
               spec.kind);
  RINGDP_CHECK(spec.period >= 1, "lr_sched: period must be at least 1, got ", spec.period);
  RINGDP_CHECK(spec.warmup_steps >= 0, "lr_sched: warmup_steps must not be negative, got ", spec.warmup_steps);
  RINGDP_CHECK(spec.total_steps > spec.warmup_steps, "lr_sched: total_steps (", spec.total_steps,
               ") must exceed warmup_steps (", spec.warmup_steps, ")");
  RINGDP_CHECK(spec.milestones.size() <= static_cast<size_t>(kern::kSchedMaxMilestones), "lr_sched: at most ",
               kern::kSchedMaxMilestones, " milestones, got ", spec.milestones.size());
  for (size_t i = 1; i < spec.milestones.size(); ++i)
    RINGDP_CHECK(spec.milestones[i - 1] <= spec.milestones[i], "lr_sched: milestones must be sorted");
  kern::LrSchedArgs a{};
  a.counter = counter.data_ptr<int64_t>();
  a.ngroups = static_cast<int>(G);
  a.advance = advance ? 1 : 0;
  a.spec.kind = static_cast<int>(spec.kind);
  a.spec.nmilestones = static_cast<int>(spec.milestones.size());
  a.spec.period = spec.period;
  a.spec.warmup_steps = spec.warmup_steps;
  a.spec.total_steps = spec.total_steps;
  a.spec.warmup_start_factor = spec.warmup_start_factor;
  a.spec.min_factor = spec.min_factor;
  a.spec.power = spec.power;
  a.spec.gamma = spec.gamma;
  for (size_t i = 0; i < spec.milestones.size(); ++i) a.spec.milestones[i] = spec.milestones[i];
  for (size_t g = 0; g < G; ++g) {
    const at::Tensor& lr = lr_tensors[g];
    scalar_gpu(lr, at::kFloat, "lr tensor");
    RINGDP_CHECK(lr.dim() == 0, "lr tensor: expected a 0-dim tensor, got ", lr.sizes());
    RINGDP_CHECK(lr.get_device() == counter.get_device(), "lr tensor on another device than the counter");
    for (size_t k = 0; k < g; ++k)
      RINGDP_CHECK(lr_tensors[k].data_ptr() != lr.data_ptr(), "lr_sched: groups ", k, " and ", g,
                   " share one lr tensor");
    a.group[g].base_lr = base_lrs[g];
    a.group[g].lr_ptr = lr.data_ptr<float>();
  }
  c10::DeviceGuard guard(counter.device());
  kern::lr_sched(a, stream_of(counter));
}

void ema_tick_run(at::Tensor num_updates, at::Tensor w, double decay, bool warmup) {
  scalar_gpu(num_updates, at::kLong, "ema num_updates");
  scalar_gpu(w, at::kFloat, "ema weight");
  RINGDP_CHECK(w.get_device() == num_updates.get_device(), "ema_tick: tensors on different devices");
  RINGDP_CHECK(decay >= 0.0 && decay <= 1.0, "ema_tick: decay must be in [0, 1], got ", decay);
  c10::DeviceGuard guard(w.device());
  kern::ema_tick(num_updates.data_ptr<int64_t>(), w.data_ptr<float>(), decay, warmup, stream_of(w));
}

void ema_update_run(const AdamTable& table, const at::Tensor& w) {
  RINGDP_CHECK(table.dev.defined() && table.table_bytes > 0, "ema_update: the table is not built");
  RINGDP_CHECK(table.pair, "ema_update: expected a table of {shadow, source} pairs (no moments)");
  RINGDP_CHECK(table.chunk_starts.size() == 2, "ema_update: expected a table of one group, got ",
               table.chunk_starts.size() - 1);
  scalar_gpu(w, at::kFloat, "ema weight");
  RINGDP_CHECK(w.get_device() == table.dev.get_device(), "ema_update: weight on another device");
  const auto* entries = reinterpret_cast<const kern::AdamTensor*>(table.dev.data_ptr());
  const auto* chunks =
      reinterpret_cast<const int64_t*>(static_cast<const char*>(table.dev.data_ptr()) + table.table_bytes);
  c10::DeviceGuard guard(table.dev.device());
  kern::ema_update_multi(entries, chunks, table.nchunks(), w.data_ptr<float>(), table.all_aligned[0],
                         stream_of(table.dev));
}

void ema_update_flat(at::Tensor shadow, const at::Tensor& source, const at::Tensor& w) {
  f32_gpu(shadow, "ema shadow");
  f32_gpu(source, "ema source");
  scalar_gpu(w, at::kFloat, "ema weight");
  RINGDP_CHECK(source.numel() == shadow.numel(), "ema_update_flat: ", source.numel(), " source elements for ",
               shadow.numel(), " shadow elements");
  RINGDP_CHECK(source.get_device() == shadow.get_device() && w.get_device() == shadow.get_device(),
               "ema_update_flat: tensors on different devices");
  RINGDP_CHECK(aligned16(shadow) && aligned16(source), "ema_update_flat: buffers must be 16-byte aligned");
  RINGDP_CHECK(shadow.data_ptr() != source.data_ptr(), "ema_update_flat: the shadow is the source");
  c10::DeviceGuard guard(shadow.device());
  kern::ema_update_flat(shadow.data_ptr<float>(), source.data_ptr<float>(), shadow.numel(), w.data_ptr<float>(),
                        stream_of(shadow));
}

}  // namespace ops
}  // namespace ringdp
