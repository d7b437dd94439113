// The outer SGD-Nesterov update of one element, shared by the fp32 / bf16 transport (optim.hip
// outer_kernel), the block-quantised transport (qcomm.hip outer_q_kernel) and the Streaming DiLoCo fragment
// update (stream_outer.hip frag_outer_mix_kernel): ONE definition, so they cannot drift apart.
//   d = delta_sum * inv_world (formed by the caller)
//   buf = first ? d : mu*buf + d ;  theta = sync - lr*(d + mu*buf) ;  sync = theta
//   has_drift: p = theta + (p - (sync_old - drift)) (overlapped mode) ; else p = theta.  Returns the new p.
// The three multiply-adds are written as explicit fused operations: they are the contractions the compiler
// formed for outer_kernel when the expressions stood inline (v_fma / v_fmac / v_fma with a negated lr), and
// pinning them keeps the rounding independent of the code around the call -- every caller gets the same bits.
#pragma once
#include "common.h"

namespace nd {

__device__ __forceinline__ float outer_update(float d, float& b, float& so, float pv, bool has_drift, float drift,
                                              float lr, float mu, int first) {
  b = first ? d : __fmaf_rn(mu, b, d);
  const float th = __fmaf_rn(-lr, __fmaf_rn(mu, b, d), so);
  const float np = has_drift ? th + (pv - (so - drift)) : th;
  so = th;
  return np;
}

// Streaming DiLoCo merge of the new outer weights th into the local weights p that kept drifting while the
// fragment's all-reduce was in flight: (1 - alpha) * th + alpha * p, as ONE fused rounding.  alpha == 0 (the
// local progress is dropped, p is not needed) returns th itself, so that case is bitwise outer_update's.
__device__ __forceinline__ float outer_mix(float th, float p, float alpha) {
  return alpha == 0.f ? th : __fmaf_rn(alpha, p - th, th);
}

}  // namespace nd
