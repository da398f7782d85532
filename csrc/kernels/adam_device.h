// Adam / AdamW element math shared by the optimizer kernels (optim.hip: flat / multi-tensor).
// Parity: torch/optim/adam.py, torch/optim/adamw.py (_single_tensor_adam, amsgrad off).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace ringdp {
namespace kern {

struct AdamDev {
  double weight_decay;
  double clip;         // global-norm clip coefficient (1 when clipping is off), negated for maximize
  float decay;         // 1 - lr * weight_decay (decoupled form)
  float step_size;     // lr / (1 - beta1^t)
  float inv_sqrt_bc2;  // 1 / sqrt(1 - beta2^t)
  float beta2, w1, w2, eps;
};

// The per-group record adam_prepare wrote earlier on this stream: {lr, step_size, 1/sqrt(bc2), clip_coef}.
__device__ __forceinline__ AdamDev load_adam(const AdamArgs& a) {
  const float4 r = *reinterpret_cast<const float4*>(a.rec);
  AdamDev d;
  d.weight_decay = a.weight_decay;
  d.clip = a.maximize ? -(double)r.w : (double)r.w;
  d.decay = (float)(1.0 - (double)r.x * a.weight_decay);
  d.step_size = r.y;
  d.inv_sqrt_bc2 = r.z;
  d.beta2 = a.beta2;
  d.w1 = a.one_minus_beta1;
  d.w2 = a.one_minus_beta2;
  d.eps = a.eps;
  return d;
}

template <bool kDecoupled>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamDev& d) {
  // The effective gradient +-clip * g (+ weight_decay * p, coupled form) is formed in fp64 and rounded once: where
  // the decay term nearly cancels the gradient, Adam's first steps (update ~ lr * g / |g|) amplify an fp32
  // rounding of either term far beyond the optimizer tolerance.  The kernel is bandwidth-bound; fp64 is free here.
  if (kDecoupled) {
    g = (float)(d.clip * (double)g);
    p *= d.decay;
  } else {
    g = (float)fma(d.weight_decay, (double)p, d.clip * (double)g);
  }
  m = fmaf(d.w1, g - m, m);
  v = fmaf(d.w2 * g, g, d.beta2 * v);
  const float denom = sqrtf(v) * d.inv_sqrt_bc2 + d.eps;
  p -= d.step_size * (m / denom);
}

}  // namespace kern
}  // namespace ringdp
