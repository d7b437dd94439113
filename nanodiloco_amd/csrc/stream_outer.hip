// Streaming DiLoCo outer step on one FRAGMENT of the flat vector (parallel/fragments.py): a fragment is a short
// list of spans [start, end) of the flat fp32 buffers, and its wire buffer is the concatenation of the spans
// ("packed" order).  Two kernels, one launch each per fragment sync instead of one per span:
//
//   nd_frag_pseudograd   out[k] = sync[g(k)] - master[g(k)]            packed fp32 / bf16 wire buffer
//   nd_frag_outer_mix    the outer Nesterov update of outer_update.h scattered back through g, then the local
//                        weights merged as master = outer_mix(theta, master, alpha), shadow = bf16(master)
//
// Span table (device, int64, built once per fragment by ops/optim.py SpanTable): S rows (start, end) followed by
// the S+1 packed offsets pre[0] = 0 .. pre[S] = total.  Every start, end and packed offset is a multiple of 64
// elements (ParamStore aligns every layer to 64), so a 16-B vector of 4 elements never straddles two spans and
// every vector access is aligned.  g(k) = start[s] + (k - pre[s]) for pre[s] <= k < pre[s+1].
//
// Both are pure HBM streams like the kernels of optim.hip: 4 elements per lane, grid-stride, grid capped at
// 2048 blocks (optim.hip stream_grid's cap; 4096 blocks, nd_outer_nesterov's cap for its 4-byte lanes, measured
// 2-8 % slower here on the whole 150M vector, profiles/stream_outer_bench.md).  A lane's packed index only grows,
// so it walks the table forwards and keeps the current span's bounds in registers: the lookup costs one compare
// per vector.
#include "common.h"
#include "outer_update.h"

using namespace nd;

namespace {

constexpr int64_t MAX_BLOCKS = 2048;

unsigned frag_grid(int64_t n4) {
  const int64_t b = (n4 + 255) / 256;
  return (unsigned)(b > MAX_BLOCKS ? MAX_BLOCKS : (b < 1 ? 1 : b));
}

struct SpanCursor {
  const int64_t* __restrict__ span;  // [S][2]
  const int64_t* __restrict__ pre;   // [S + 1]
  int S, s;
  int64_t hi, off;  // current span: packed end, start - packed begin
  __device__ __forceinline__ SpanCursor(const int64_t* table, int S_) : span(table), pre(table + 2 * S_), S(S_), s(0) {
    load();
  }
  __device__ __forceinline__ void load() {
    hi = pre[s + 1];
    off = span[2 * s] - pre[s];
  }
  // flat index of packed index k (k must not decrease between calls); never reads past row S - 1
  __device__ __forceinline__ int64_t flat(int64_t k) {
    while (k >= hi && s + 1 < S) {
      ++s;
      load();
    }
    return k + off;
  }
};

}  // namespace

template <int DDT>
__global__ void __launch_bounds__(256) frag_pseudograd_kernel(const float* __restrict__ sync,
                                                              const float* __restrict__ p,
                                                              const int64_t* __restrict__ table, int S, int64_t total,
                                                              void* __restrict__ d) {
  SpanCursor cur(table, S);
  const int64_t n4 = total >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t g = cur.flat(i * 4);
    const float4 Sv = *reinterpret_cast<const float4*>(sync + g);
    const float4 P = *reinterpret_cast<const float4*>(p + g);
    const float4 D = make_float4(Sv.x - P.x, Sv.y - P.y, Sv.z - P.z, Sv.w - P.w);
    if (DDT == BF16) reinterpret_cast<uint2*>(d)[i] = make_uint2(pack2(D.x, D.y), pack2(D.z, D.w));
    else reinterpret_cast<float4*>(d)[i] = D;
  }
}

ND_API int nd_frag_pseudograd(const float* sync, const float* master, const int64_t* spans, int S, int64_t total,
                              void* out, int out_dt, hipStream_t s) {
  if (S <= 0 || total <= 0) return 0;
  const unsigned grid = frag_grid(total >> 2);
  if (out_dt == BF16)
    hipLaunchKernelGGL(frag_pseudograd_kernel<BF16>, dim3(grid), dim3(256), 0, s, sync, master, spans, S, total, out);
  else
    hipLaunchKernelGGL(frag_pseudograd_kernel<F32>, dim3(grid), dim3(256), 0, s, sync, master, spans, S, total, out);
  ND_LAUNCH_CHECK();
}

// Per element: d = delta * inv_w ; (theta, buf) = outer_update(...) ; sync = theta ; master = outer_mix(theta,
// master, alpha) ; shadow = bf16(master).  alpha is a kernel argument, so `mix` is uniform over the grid: with
// alpha == 0 the master is never read and the kernel moves nd_outer_nesterov's 26 B / element (30 B otherwise).
template <int DDT, int SDT>
__global__ void __launch_bounds__(256) frag_outer_mix_kernel(float* __restrict__ p, float* __restrict__ sync,
                                                             const void* __restrict__ dsum, float* __restrict__ buf,
                                                             void* __restrict__ sh, const int64_t* __restrict__ table,
                                                             int S, int64_t total, float inv_w, float lr, float mu,
                                                             int first, float alpha) {
  SpanCursor cur(table, S);
  const bool mix = alpha != 0.f;
  const int64_t n4 = total >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t g = cur.flat(i * 4);
    float d[4];
    if (DDT == BF16) {
      const uint2 w = reinterpret_cast<const uint2*>(dsum)[i];
      d[0] = lo_bf(w.x); d[1] = hi_bf(w.x); d[2] = lo_bf(w.y); d[3] = hi_bf(w.y);
    } else {
      const float4 w = reinterpret_cast<const float4*>(dsum)[i];
      d[0] = w.x; d[1] = w.y; d[2] = w.z; d[3] = w.w;
    }
    const float4 B = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(buf + g);
    const float4 So = *reinterpret_cast<const float4*>(sync + g);
    const float4 P = mix ? *reinterpret_cast<const float4*>(p + g) : make_float4(0.f, 0.f, 0.f, 0.f);
    float b[4] = {B.x, B.y, B.z, B.w}, so[4] = {So.x, So.y, So.z, So.w}, np[4] = {P.x, P.y, P.z, P.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float th = outer_update(d[j] * inv_w, b[j], so[j], 0.f, false, 0.f, lr, mu, first);
      np[j] = outer_mix(th, np[j], alpha);
    }
    *reinterpret_cast<float4*>(buf + g) = make_float4(b[0], b[1], b[2], b[3]);
    *reinterpret_cast<float4*>(sync + g) = make_float4(so[0], so[1], so[2], so[3]);
    *reinterpret_cast<float4*>(p + g) = make_float4(np[0], np[1], np[2], np[3]);
    if (SDT == BF16)
      *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(sh) + g) = make_uint2(pack2(np[0], np[1]), pack2(np[2], np[3]));
  }
}

ND_API int nd_frag_outer_mix(float* master, float* sync, const void* delta_packed, int dt, float* mom, void* shadow,
                             int sh_dt, const int64_t* spans, int S, int64_t total, float inv_w, float lr, float mu,
                             int first, float alpha, hipStream_t s) {
  if (S <= 0 || total <= 0) return 0;
  const unsigned grid = frag_grid(total >> 2);
  const bool bsh = shadow && sh_dt == BF16;
#define ND_FM(D, SH) hipLaunchKernelGGL((frag_outer_mix_kernel<D, SH>), dim3(grid), dim3(256), 0, s, master, sync, \
                                        delta_packed, mom, shadow, spans, S, total, inv_w, lr, mu, first, alpha)
  if (dt == BF16) { if (bsh) ND_FM(BF16, BF16); else ND_FM(BF16, F32); }
  else { if (bsh) ND_FM(F32, BF16); else ND_FM(F32, F32); }
#undef ND_FM
  ND_LAUNCH_CHECK();
}
