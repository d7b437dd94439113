// The inner optimizer's shared device code: the clip coefficient from the global sum-of-squares partials and the
// per-element AdamW update.  nd_adamw_step (optim.hip, the whole flat vector) and nd_adamw_step_spans (muon.hip,
// the non-Muon spans of it) run exactly this code, so on the same element they produce the same bits; the Muon
// kernels take the same clip coefficient and the same skip decision from clip_from_partials.
#pragma once
#include "common.h"

namespace nd {

struct ClipState {
  float coef;  // min(1, max_norm / (norm + 1e-6)); 1 without clipping
  bool skip;   // skip_nonfinite and the global norm is NaN / Inf: the caller writes no state
};

// Every block re-reduces the <= 1024 partials of nd_sumsq_partial (4 KB, L2-resident): the same order in every
// block, so every block of every kernel of one step sees the same norm.  Contains barriers: all 256 threads call
// it.  part == nullptr: no norm (coef 1, never skipped).  Block 0 writes norm_out and counts a skipped step when
// the caller passes the pointers (ONE kernel per step does).
__device__ __forceinline__ ClipState clip_from_partials(const float* __restrict__ part, int nparts, float max_norm,
                                                        int skip_nonfinite, float* __restrict__ norm_out,
                                                        int* __restrict__ skipped, float* red) {
  ClipState c{1.f, false};
  if (!part) return c;
  float t = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) t += part[i];
  t = block_sum<256>(t, red);
  const float norm = sqrtf(t);
  if (max_norm > 0.f) c.coef = fminf(1.f, max_norm / (norm + 1e-6f));
  const bool first = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
  if (norm_out && first) norm_out[0] = norm;
  // device-side guard: every block sees the same norm, so a NaN/Inf step is skipped everywhere
  // (no host sync); the step counter on the host still advances, like torch's GradScaler skip.
  if (skip_nonfinite && !isfinite(norm)) {
    if (skipped && first) skipped[0] += 1;
    c.skip = true;
  }
  return c;
}

struct AdamWCoef {
  float coef, decay, step, rbc2, omb1, b2, omb2, eps;
  __device__ __forceinline__ AdamWCoef(float coef_, float lr, float wd, float bc1, float bc2, float omb1_, float b2_,
                                       float omb2_, float eps_)
      : coef(coef_), decay(1.f - lr * wd), step(lr / bc1), rbc2(1.f / sqrtf(bc2)), omb1(omb1_), b2(b2_), omb2(omb2_),
        eps(eps_) {}
};

// torch.optim.AdamW's single-tensor order: decoupled decay, m / v update, bias-corrected step
__device__ __forceinline__ void adamw_update(const AdamWCoef& c, float& pp, float gg, float& mm, float& vv) {
  gg *= c.coef;
  pp *= c.decay;
  mm = mm + c.omb1 * (gg - mm);
  vv = vv * c.b2 + c.omb2 * gg * gg;
  const float den = sqrtf(vv) * c.rbc2 + c.eps;
  pp = pp - c.step * (mm / den);
}

}  // namespace nd
