// Attention logit soft-capping (docs/DESIGN.md "Attention soft-capping"): the launchers of the capped instantiations
// of the flash-attention kernels.  Scores become z = C tanh(scale q.k / C) before the mask and the softmax (HF Gemma 2
// `attn_logit_softcapping`: scale, cap, then mask); the backward carries the factor 1 - tanh^2.
//
// The kernels are the templates of attention.hip, instantiated with one trailing CapArgs: this file includes that
// source for the templates alone, so the capped kernels are objects of their own (built with their own flags) and
// the uncapped library entries launch the instantiations they always did.  One entry per direction takes every mask
// mode the kernels have -- kstart (left padding), doc_start / doc_end (packed documents), window -- plus the cap:
//   forward   T % 64 == 0: the LDS-DMA kernel; any other T: the register-staged kernel (not with documents)
//   backward  the fused LDS-DMA pair only (T % 64 == 0): dQ (writes -delta and -lse for the next kernel), then dK/dV
// q|k are already rotated (the backward un-rotates dq / dk with rope_mode 2, as the other fused entries).  Always the
// default block shape and the plain softmax variant; of the A/B switches only the grid orders and the deferred-max
// threshold apply.  No host synchronisation: capturable in a HIP graph like the uncapped launches.
#undef ND_ATTN_STAMP  // the stamp buffer exists once, in attention.hip's own object
#define ND_ATTN_KERNELS_ONLY 1
#include "attention.hip"

namespace nd {
float attn_env_thr();
int attn_env_order();
int attn_env_dkdv_order(int nh, int nkv);
}  // namespace nd

namespace {

// which mask a call asks for (documents and a window do not combine, as in the uncapped entries)
int mask_of(const int* ks, const int* doc_start, const int* doc_end, int window) {
  if (doc_start || doc_end) return (doc_start && doc_end && !ks && window < 1) ? MASK_DOC : -1;
  if (window >= 1) return MASK_WIN;
  return ks ? MASK_PAD : MASK_NONE;
}

template <int HD, int MASK>
int fwd_cap_launch(const void* q, const void* k, const void* v, void* o, float* lse, int B, int nh, int nkv, int T,
                   int64_t ld, int64_t ldo, float scale, const int* mk, int window, CapArgs cp, hipStream_t s) {
  const dim3 g((T + 127) / 128 * B * nh), b(256);
  if (T % 64 == 0)
    hipLaunchKernelGGL((attn_fwd_kernel<HD, false, true, MASK, 0, 4, CapArgs>), g, b, 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, B, nh, nkv, T, ld, ldo, scale, nullptr,
                       nullptr, mk, attn_env_thr(), attn_env_order(), window, cp);
  else if constexpr (MASK != MASK_DOC)
    hipLaunchKernelGGL((attn_fwd_kernel<HD, false, false, MASK, 0, 4, CapArgs>), g, b, 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, B, nh, nkv, T, ld, ldo, scale, nullptr,
                       nullptr, mk, attn_env_thr(), attn_env_order(), window, cp);
  else
    return (int)hipErrorInvalidValue;
  ND_LAUNCH_CHECK();
}

template <int HD, int MASK, bool ROPE_OUT>
int bwd_cap_launch(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   void* dq, void* dk, void* dv, float* ws, int B, int nh, int nkv, int T, int64_t ld, int64_t ldo,
                   const float* cosT, const float* sinT, float scale, const int* mq, const int* mkv, int window,
                   CapArgs cp, hipStream_t s) {
  const int nb = (T + 127) / 128;
  const int64_t n = (int64_t)B * nh * T;
  float *nl = ws, *nd = ws + n;  // -lse (log2 domain, as it is: the capped form) and -delta
  hipLaunchKernelGGL((attn_bwd_dq_kernel<HD, false, ROPE_OUT, true, true, MASK, 4, CapArgs>), dim3(nb * B * nh),
                     dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse,
                     nullptr, (bf16_t*)dq, B, nh, nkv, T, ld, ldo, scale, cosT, sinT, (const bf16_t*)o, nl, nd, mq,
                     attn_env_order(), window, cp);
  // 128-query tiles when T allows, but for head_dim 64 with a window: that one instantiation needs 5-6 registers more
  // than the 256 of two waves per SIMD and would spill; its 64-query form (234 VGPRs) serves every T
  constexpr bool BQ128 = !(HD == 64 && MASK == MASK_WIN);
  if (BQ128 && T % 128 == 0)
    hipLaunchKernelGGL((attn_bwd_dkdv_dma_kernel<HD, ROPE_OUT, BQ128 ? 128 : 64, MASK, 4, 0, 2, CapArgs>), dim3(nb * B * nkv),
                       dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, nl,
                       nd, (bf16_t*)dk, (bf16_t*)dv, B, nh, nkv, T, ld, ldo, scale, cosT, sinT, mkv,
                       attn_env_dkdv_order(nh, nkv), window, cp);
  else
    hipLaunchKernelGGL((attn_bwd_dkdv_dma_kernel<HD, ROPE_OUT, 64, MASK, 4, 0, 2, CapArgs>), dim3(nb * B * nkv),
                       dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, nl,
                       nd, (bf16_t*)dk, (bf16_t*)dv, B, nh, nkv, T, ld, ldo, scale, cosT, sinT, mkv,
                       attn_env_dkdv_order(nh, nkv), window, cp);
  ND_LAUNCH_CHECK();
}

}  // namespace

// Capped forward.  ks: per-sequence key start [B] or null; doc_start / doc_end: per-token document bounds [B, T], both
// or neither (then T % 64 == 0, no ks, no window); window: 0 = none, W >= 1 = sliding window (composes with ks);
// cap: C, finite and > 0.  lse: log2 domain, of the capped scores.  A row with no visible key gives o = 0, lse = -inf.
ND_API int nd_attn_fwd_cap(const void* q, const void* k, const void* v, void* o, float* lse, int B, int nh, int nkv,
                           int T, int hd, int64_t ld, int64_t ldo, float scale, const int* ks, const int* doc_start,
                           const int* doc_end, int window, float cap, hipStream_t s) {
  const int mask = mask_of(ks, doc_start, doc_end, window);
  if (nh % nkv || (ld % 8) || (ldo % 8) || T < 1 || window < 0 || mask < 0 || !cap_ok(cap))
    return (int)hipErrorInvalidValue;
  const CapArgs cp = cap_args(cap);
  const int w = window < T ? window : T;  // a window of T or more keys is the whole prefix
#define ND_FC(H)                                                                                                       \
  case H:                                                                                                              \
    switch (mask) {                                                                                                    \
      case MASK_DOC: return fwd_cap_launch<H, MASK_DOC>(q, k, v, o, lse, B, nh, nkv, T, ld, ldo, scale, doc_start, 0, cp, s); \
      case MASK_WIN: return fwd_cap_launch<H, MASK_WIN>(q, k, v, o, lse, B, nh, nkv, T, ld, ldo, scale, ks, w, cp, s);  \
      case MASK_PAD: return fwd_cap_launch<H, MASK_PAD>(q, k, v, o, lse, B, nh, nkv, T, ld, ldo, scale, ks, 0, cp, s);  \
      default: return fwd_cap_launch<H, MASK_NONE>(q, k, v, o, lse, B, nh, nkv, T, ld, ldo, scale, nullptr, 0, cp, s);  \
    }
  switch (hd) {
    ND_FC(32)
    ND_FC(64)
    ND_FC(128)
    default: return (int)hipErrorInvalidValue;
  }
#undef ND_FC
}

// Capped fused backward (see nd_attn_bwd_fused_ks / _doc / _win for the uncapped forms): T % 64 == 0, rope_mode 0 or
// 2, ws: 2 * B * nh * T floats; dq / dk / dv may point into one packed buffer (row stride ld).  The mask arguments
// are nd_attn_fwd_cap's.  No atomics: bitwise reproducible like every other mode.
ND_API int nd_attn_bwd_fused_cap(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                 const float* lse, void* dq, void* dk, void* dv, float* ws, int B, int nh, int nkv,
                                 int T, int hd, int64_t ld, int64_t ldo, const float* cosT, const float* sinT,
                                 float scale, int rope_mode, const int* ks, const int* doc_start, const int* doc_end,
                                 int window, float cap, hipStream_t s) {
  const int mask = mask_of(ks, doc_start, doc_end, window);
  if (nh % nkv || (ld % 8) || (ldo % 8) || T < 1 || T % 64 || ws == nullptr || window < 0 || mask < 0 || !cap_ok(cap))
    return (int)hipErrorInvalidValue;
  if ((rope_mode != 0 && rope_mode != 2) || (rope_mode == 2 && !(cosT && sinT))) return (int)hipErrorInvalidValue;
  const CapArgs cp = cap_args(cap);
  const int w = window < T ? window : T;
#define ND_BC(H, R)                                                                                                    \
  switch (mask) {                                                                                                      \
    case MASK_DOC: return bwd_cap_launch<H, MASK_DOC, R>(q, k, v, o, dout, lse, dq, dk, dv, ws, B, nh, nkv, T, ld, ldo, cosT, sinT, scale, doc_start, doc_end, 0, cp, s); \
    case MASK_WIN: return bwd_cap_launch<H, MASK_WIN, R>(q, k, v, o, dout, lse, dq, dk, dv, ws, B, nh, nkv, T, ld, ldo, cosT, sinT, scale, ks, ks, w, cp, s); \
    case MASK_PAD: return bwd_cap_launch<H, MASK_PAD, R>(q, k, v, o, dout, lse, dq, dk, dv, ws, B, nh, nkv, T, ld, ldo, cosT, sinT, scale, ks, ks, 0, cp, s); \
    default: return bwd_cap_launch<H, MASK_NONE, R>(q, k, v, o, dout, lse, dq, dk, dv, ws, B, nh, nkv, T, ld, ldo, cosT, sinT, scale, nullptr, nullptr, 0, cp, s); \
  }
#define ND_BCH(H)          \
  case H:                  \
    if (rope_mode == 2) {  \
      ND_BC(H, true)       \
    } else {               \
      ND_BC(H, false)      \
    }
  switch (hd) {
    ND_BCH(32)
    ND_BCH(64)
    ND_BCH(128)
    default: return (int)hipErrorInvalidValue;
  }
#undef ND_BCH
#undef ND_BC
}
