// Host helpers shared by the bf16 ConvNet units; defined in convnet_reduce.hip unless inline.
#pragma once

#include <algorithm>
#include <type_traits>
#include <vector>

#include "kernels.h"

namespace ringdp::kern {

__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
int num_cus();

// fixed-order slab reduction: one segment of it, and its launch (one per 8 segments)
ReduceSeg seg(const float* slabs, int64_t stride, int64_t off, int64_t n, int nslices, float* out, int mode = 0,
              int cin = 0, int cout = 0);
void launch_reduce(const std::vector<ReduceSeg>& v, hipStream_t s);

// Environment knob `name`: atoi / atof of its value when it is set and `ok` (if given) accepts that, else dflt.
// Callers keep the result in a function-local static: every knob is read once per process.
int env_int(const char* name, int dflt, bool (*ok)(int) = nullptr);
double env_real(const char* name, double dflt, bool (*ok)(double));
inline bool split_frac_ok(double f) { return f > 0.05 && f < 0.95; }  // the RINGDP_*_DGRAD_FRAC knobs
inline bool slab_images_ok(int n) { return n >= 1 && n <= 64; }       // the RINGDP_*_WMIN knobs

// The 8-wave backward kernels (fc_bwd_kernel + conv3_bwd8_kernel, conv12_bwd8_kernel) run batches above
// RINGDP_CN_FC_IN_C3_MAX (2048); up to it the 4-wave kernels, fc1's backward inside the conv3 backward launch.
int fc_in_c3_max_batch();
inline bool use_8wave(int B) { return B > fc_in_c3_max_batch(); }

// f(std::true_type{}) or f(std::false_type{}): a run-time flag (uint8 / float input) as a template argument
template <class F>
void dispatch_bool(bool flag, F&& f) {
  flag ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace ringdp::kern
