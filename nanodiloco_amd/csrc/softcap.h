// Final-logit soft-capping, y = C * tanh(x / C) (docs/DESIGN.md "Logit soft-capping"): what the capped
// instantiations of the lm-head kernels (cross_entropy.hip, ce_loss.hip) take on top of the plain kernels' arguments,
// and the one formulation of tanh and its derivative that all of them share.
#pragma once
#include "common.h"

namespace nd {

struct CapArgs {
  float cap;  // C
  float inv;  // 1 / C, rounded once on the host
};

// a cap a launcher accepts: finite and > 0 (refuses NaN too)
inline bool cap_ok(float c) { return c > 0.f && c <= 3.0e38f; }
inline CapArgs cap_args(float c) { return CapArgs{c, 1.f / c}; }

// t = tanh(u) and d = 1 - t^2 from one v_exp_f32 and one v_rcp_f32: with e = exp(-2|u|) in [0, 1],
//   t = sign(u) (1 - e) / (1 + e)        d = 4 e / (1 + e)^2
// Nothing can overflow: |u| -> inf gives e = 0, t = +-1 and d = 0 exactly (from |u| > 9 on t is +-1, from |u| > 44
// d is 0), never inf / inf.  d has no cancellation anywhere.  1 - e cancels towards u = 0 (absolute error 2^-24,
// relative 2^-24 / 2|u|), so below |u| = 1/4 t is the odd series u - u^3/3 + 2u^5/15 - 17u^7/315 + 62u^9/2835
// (next term < 2^-26 relative there; at the border 1 - e = 0.39 carries the exponential's ulp 1.5 times).
// NaN stays NaN in both results (every comparison with it is false: the e form, which propagates it).
__device__ __forceinline__ float cap_tanh(float u, float& d) {
  const float a = fabsf(u);
  const float e = __builtin_amdgcn_exp2f(a * -2.8853900817779268f);  // -2 log2(e)
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  d = 4.f * e * r * r;
  const float u2 = u * u;
  float p = fmaf(u2, 0.021869488536155203f, -0.053968253968253971f);
  p = fmaf(u2, p, 0.13333333333333333f);
  p = fmaf(u2, p, -0.33333333333333333f);
  const float small = fmaf(u * u2, p, u);
  const float big = copysignf((1.f - e) * r, u);
  return a < 0.25f ? small : big;
}

__device__ __forceinline__ float cap_tanh(float u) {
  float d;
  return cap_tanh(u, d);
}

}  // namespace nd
