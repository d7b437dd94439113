// Attention logit soft-capping for the decode step (docs/DESIGN.md "Attention soft-capping"): nd_attn_decode with the
// scores z = C tanh(scale q.k / C) over the same keys.  The kernel is attn_decode.hip's attn_decode_kernel with one
// trailing CapArgs -- the cap is applied to a key's fp32 dot product before it joins the wave's scores, so the
// two-pass softmax, the wave merge, the key-indexed partition and the combine kernel are the uncapped ones, and so
// are the append to slot pos[b] and the launch shape (HIP-graph capturable).  This file includes that source for
// everything but its library entries, so the capped kernels are objects of their own.
#define ND_DECODE_KERNELS_ONLY 1
#include "attn_decode.hip"

// window: 0 = none, W >= 1 = sliding window (as nd_attn_decode_win); cap: C, finite and > 0.
ND_API int nd_attn_decode_cap(const void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                              void* kcache, void* vcache, float* part_o, float* part_ml, void* o, int B, int nh,
                              int nkv, int hd, int S_max, int64_t ld, float scale, int window, float cap,
                              hipStream_t st) {
  if (window < 0 || !cap_ok(cap)) return (int)hipErrorInvalidValue;
  return decode_impl(qkv, cosT, sinT, pos, kstart, kcache, vcache, part_o, part_ml, o, B, nh, nkv, hd, S_max, ld, scale,
                     window, st, cap_args(cap));
}
