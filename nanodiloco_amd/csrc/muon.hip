// Device side of the Muon inner optimizer (ops/muon.py, docs/DESIGN.md "Muon inner optimizer"): AdamW over a span
// table, for everything Muon does not own (embedding, lm head, norms).
//
//   nd_adamw_step_spans  adamw_update (adamw_update.h) over a span table, one launch: inside the spans the bits of
//                        nd_adamw_step (optim.hip) on the same element, outside nothing is written
//
// The clip coefficient comes from the partials of the WHOLE gradient (clip_from_partials), as in nd_adamw_step.
#include "adamw_update.h"

using namespace nd;

// Span table (device, int64): S rows (start, end), then S + 1 prefix sums pre[] of the spans' lengths in 4-element
// vectors, each rounded UP (a span of 5 elements takes 2 vector slots).  Starts are multiples of 4 elements,
// lengths are arbitrary: vector slot j of a span is a 16-B access when all four elements exist and a scalar tail
// otherwise.  A lane's slot index only grows, so it walks the table forwards.
template <int SDT>
__global__ void __launch_bounds__(256) adamw_spans_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          void* __restrict__ sh, const int64_t* __restrict__ table,
                                                          int S, int64_t total4, const float* __restrict__ part,
                                                          int nparts, float lr, float omb1, float b2, float omb2,
                                                          float eps, float wd, float bc1, float bc2, float max_norm,
                                                          float* __restrict__ norm_out, int skip_nonfinite,
                                                          int* __restrict__ skipped) {
  __shared__ float red[4];
  const ClipState clip = clip_from_partials(part, nparts, max_norm, skip_nonfinite, norm_out, skipped, red);
  if (clip.skip) return;
  const AdamWCoef c(clip.coef, lr, wd, bc1, bc2, omb1, b2, omb2, eps);
  const int64_t* pre = table + 2 * S;
  int s = 0;
  int64_t hi = pre[1];
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total4; k += (int64_t)gridDim.x * 256) {
    while (k >= hi && s + 1 < S) {
      ++s;
      hi = pre[s + 1];
    }
    const int64_t i = table[2 * s] + (k - pre[s]) * 4, end = table[2 * s + 1];
    if (i + 4 <= end) {
      float4 P = *reinterpret_cast<float4*>(p + i);
      const float4 G = *reinterpret_cast<const float4*>(g + i);
      float4 Mv = *reinterpret_cast<float4*>(m + i);
      float4 Vv = *reinterpret_cast<float4*>(v + i);
      adamw_update(c, P.x, G.x, Mv.x, Vv.x);
      adamw_update(c, P.y, G.y, Mv.y, Vv.y);
      adamw_update(c, P.z, G.z, Mv.z, Vv.z);
      adamw_update(c, P.w, G.w, Mv.w, Vv.w);
      *reinterpret_cast<float4*>(p + i) = P;
      *reinterpret_cast<float4*>(m + i) = Mv;
      *reinterpret_cast<float4*>(v + i) = Vv;
      if (SDT == BF16)
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(sh) + i) = make_uint2(pack2(P.x, P.y), pack2(P.z, P.w));
    } else {
      for (int64_t j = i; j < end; ++j) {
        float pp = p[j], mm = m[j], vv = v[j];
        adamw_update(c, pp, g[j], mm, vv);
        p[j] = pp; m[j] = mm; v[j] = vv;
        if (SDT == BF16) reinterpret_cast<bf16_t*>(sh)[j] = f2bf(pp);
      }
    }
  }
}

ND_API int nd_adamw_step_spans(float* p, const float* g, float* m, float* v, void* sh, int shdt, const int64_t* table,
                               int S, int64_t total4, const float* part, int nparts, float lr, double b1, double b2,
                               float eps, float wd, float bc1, float bc2, float max_norm, float* norm_out,
                               int skip_nonfinite, int* skipped, hipStream_t s) {
  if (S <= 0 || total4 <= 0) return 0;
  const int64_t b = (total4 + 255) / 256;
  const unsigned grid = (unsigned)(b > 2048 ? 2048 : b);
  const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2), b2f = (float)b2;
  if (sh && shdt == BF16)
    hipLaunchKernelGGL(adamw_spans_kernel<BF16>, dim3(grid), dim3(256), 0, s, p, g, m, v, sh, table, S, total4, part,
                       nparts, lr, omb1, b2f, omb2, eps, wd, bc1, bc2, max_norm, norm_out, skip_nonfinite, skipped);
  else
    hipLaunchKernelGGL(adamw_spans_kernel<F32>, dim3(grid), dim3(256), 0, s, p, g, m, v, nullptr, table, S, total4,
                       part, nparts, lr, omb1, b2f, omb2, eps, wd, bc1, bc2, max_norm, norm_out, skip_nonfinite,
                       skipped);
  ND_LAUNCH_CHECK();
}
