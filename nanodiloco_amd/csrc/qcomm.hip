// Block-quantised transport of the DiLoCo pseudo-gradient (int8 / int4 codes + one fp32 scale per 256
// elements; wire format: docs/DESIGN.md "Quantised outer transport").
//
//   nd_pseudograd_q      d = sync - master in registers -> codes + scales, laid out as W wire chunks
//   nd_qreduce           W received chunks -> one requantised chunk holding their sum (rank order)
//   nd_outer_nesterov_q  the outer Nesterov update with d = (code * scale) * inv_w from the gathered chunks
//
// Error feedback (docs/DESIGN.md "Error feedback"): nd_pseudograd_q_ef / nd_qreduce_ef are the same kernels with
// an fp32 residual added to the value before it is quantised and rewritten, in place, as what the codes did
// not deliver: x = v + e, e = x - code * scale.  A lane reads and writes only its own four residual elements.
//
// One wave64 owns one quantisation block: lane l holds elements 4l..4l+3 (one float4), the block amax is a
// wave reduction (no LDS, no barrier).  A 256-thread workgroup therefore covers four blocks per pass; the
// grid is capped at 2048 workgroups like the other flat kernels and strides over the rest.
//
// A wire chunk of c elements is [codes: c*BITS/8 bytes][scales: c/256 fp32], W chunks back to back.  The
// chunk stride is a multiple of 4 bytes but not always of 16, so the wire side is accessed with dword (or
// narrower) instructions only: one dword of codes per lane (int8), one dword per lane PAIR (int4).  The
// fp32 side (sync, master, momentum) uses 16-byte accesses and is never touched past its logical length.
#include "common.h"
#include "outer_update.h"

using namespace nd;

namespace {

constexpr int QB = 256;  // elements per quantisation block

template <int BITS> struct Q;
template <> struct Q<8> { static constexpr float QMAX = 127.f; static constexpr int BLOCK_BYTES = 256; };
template <> struct Q<4> { static constexpr float QMAX = 7.f; static constexpr int BLOCK_BYTES = 128; };

struct Wire {         // geometry of W chunks of `bpc` blocks each
  int64_t bpc;        // quantisation blocks per chunk (c / 256)
  int64_t stride;     // bytes from one chunk to the next
  int64_t code_bytes; // bytes of one chunk's codes (= offset of its scales)
};

template <int BITS>
__device__ __forceinline__ Wire wire_of(int64_t bpc) {
  Wire w;
  w.bpc = bpc;
  w.code_bytes = bpc * Q<BITS>::BLOCK_BYTES;
  w.stride = w.code_bytes + bpc * 4;
  return w;
}

unsigned q_grid(int64_t nblk) {
  const int64_t b = (nblk + 3) / 4;
  return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// Quantise the wave's block (x: this lane's 4 values) and store codes + scale.  fmaxf drops NaNs, so
// non-finite values are tracked apart: such a block gets a NaN scale (and zero codes), and the update
// that consumes it becomes NaN as it would with fp32 transport.  Hands back the lane's codes (q) and returns
// the block scale (wave-uniform) for the error-feedback residual.
template <int BITS>
__device__ __forceinline__ float quant_store(const float (&x)[4], uint8_t* __restrict__ codes,
                                             float* __restrict__ scale, int lane, int (&q)[4]) {
  constexpr float QMAX = Q<BITS>::QMAX;
  const float m = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
  const bool bad = __any(!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(x[3])));
  const float amax = wave_max(m);
  // IEEE division; kept finite: below amax ~ 3.7e-37 the quotient overflows, and a zero element times inf
  // would be NaN (with the clamp such a block only loses resolution, at a scale of ~1e-39)
  const float inv = (!bad && amax > 0.f) ? fminf(QMAX / amax, 3.402823466e+38f) : 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    q[k] = bad ? 0 : (int)fminf(fmaxf(rintf(x[k] * inv), -QMAX), QMAX);
  if (BITS == 8) {
    const uint32_t w = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) |
                       ((uint32_t)(q[3] & 0xff) << 24);
    reinterpret_cast<uint32_t*>(codes)[lane] = w;
  } else {
    const uint32_t h = (uint32_t)(q[0] & 0xf) | ((uint32_t)(q[1] & 0xf) << 4) | ((uint32_t)(q[2] & 0xf) << 8) |
                       ((uint32_t)(q[3] & 0xf) << 12);
    const uint32_t up = __shfl_xor(h, 1, 64);  // the pair's other half: even lanes store one dword
    if ((lane & 1) == 0) reinterpret_cast<uint32_t*>(codes)[lane >> 1] = h | (up << 16);
  }
  const float sc = bad ? __builtin_nanf("") : amax / QMAX;
  if (lane == 0) scale[0] = sc;
  return sc;
}

// what the codes did not deliver: r = x - code * scale, product and difference rounded separately (the
// receivers compute fl(code * scale)); a non-finite block (scale NaN) gives NaN
__device__ __forceinline__ void residual_of(const float (&x)[4], const int (&q)[4], float sc, float (&r)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = x[k] - (float)q[k] * sc;
}

// this lane's 4 codes of a block, as floats
template <int BITS>
__device__ __forceinline__ void load_codes(const uint8_t* __restrict__ codes, int lane, float (&v)[4]) {
  if (BITS == 8) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(codes)[lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)(int8_t)(w >> (8 * k));
  } else {
    const uint32_t w = reinterpret_cast<const uint32_t*>(codes)[lane >> 1] >> ((lane & 1) * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)(((int32_t)(w << (28 - 4 * k))) >> 28);  // sign-extended nibble
  }
}

// EF: resid (n elements) is added to sync - master before the quantiser and rewritten with the new residual
template <int BITS, bool EF>
__global__ void __launch_bounds__(256) pseudograd_q_kernel(const float* __restrict__ sync, const float* __restrict__ p,
                                                           float* __restrict__ resid, int64_t n,
                                                           uint8_t* __restrict__ out, int64_t nblk, int64_t bpc) {
  const Wire w = wire_of<BITS>(bpc);
  const int lane = threadIdx.x & 63;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblk; blk += (int64_t)gridDim.x * 4) {
    const int64_t e = blk * QB + lane * 4;
    float x[4] = {0.f, 0.f, 0.f, 0.f};  // elements past n count as zero
    if (e + 4 <= n) {
      const float4 S = *reinterpret_cast<const float4*>(sync + e);
      const float4 P = *reinterpret_cast<const float4*>(p + e);
      x[0] = S.x - P.x; x[1] = S.y - P.y; x[2] = S.z - P.z; x[3] = S.w - P.w;
      if (EF) {
        const float4 E = *reinterpret_cast<const float4*>(resid + e);
        x[0] = x[0] + E.x; x[1] = x[1] + E.y; x[2] = x[2] + E.z; x[3] = x[3] + E.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) {
          x[k] = sync[e + k] - p[e + k];
          if (EF) x[k] = x[k] + resid[e + k];
        }
    }
    const int64_t ch = blk / bpc, j = blk - ch * bpc;
    uint8_t* base = out + ch * w.stride;
    int q[4];
    const float sc = quant_store<BITS>(x, base + j * Q<BITS>::BLOCK_BYTES,
                                       reinterpret_cast<float*>(base + w.code_bytes) + j, lane, q);
    if (EF) {  // no residual past n: nothing is read or written there
      float r[4];
      residual_of(x, q, sc, r);
      if (e + 4 <= n) {
        *reinterpret_cast<float4*>(resid + e) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < n) resid[e + k] = r[k];
      }
    }
  }
}

// EF: resid (one chunk, bpc * 256 elements) is added after the rank-order sum and rewritten
template <int BITS, bool EF>
__global__ void __launch_bounds__(256) qreduce_kernel(const uint8_t* __restrict__ in, int nw, int64_t bpc,
                                                      float* __restrict__ resid, uint8_t* __restrict__ out) {
  const Wire w = wire_of<BITS>(bpc);
  const int lane = threadIdx.x & 63;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < bpc; j += (int64_t)gridDim.x * 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = 0; r < nw; ++r) {  // rank order: deterministic
      const uint8_t* base = in + r * w.stride;
      const float sc = reinterpret_cast<const float*>(base + w.code_bytes)[j];
      float v[4];
      load_codes<BITS>(base + j * Q<BITS>::BLOCK_BYTES, lane, v);
      {
#pragma clang fp contract(off)  // product and sum round separately, like the PyTorch path: no fused multiply-add
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = acc[k] + v[k] * sc;
      }
    }
    float4* E = EF ? reinterpret_cast<float4*>(resid + j * QB + lane * 4) : nullptr;
    if (EF) {
      const float4 e = *E;
      acc[0] = acc[0] + e.x; acc[1] = acc[1] + e.y; acc[2] = acc[2] + e.z; acc[3] = acc[3] + e.w;
    }
    int q[4];
    const float sc = quant_store<BITS>(acc, out + j * Q<BITS>::BLOCK_BYTES,
                                       reinterpret_cast<float*>(out + w.code_bytes) + j, lane, q);
    if (EF) {
      float r[4];
      residual_of(acc, q, sc, r);
      *E = make_float4(r[0], r[1], r[2], r[3]);
    }
  }
}

template <int BITS, int SDT>
__global__ void __launch_bounds__(256) outer_q_kernel(float* __restrict__ p, float* __restrict__ sync,
                                                      const uint8_t* __restrict__ q, float* __restrict__ buf,
                                                      void* __restrict__ sh, int64_t n, int64_t bpc, float inv_w,
                                                      float lr, float mu, int first) {
  const Wire w = wire_of<BITS>(bpc);
  const int lane = threadIdx.x & 63;
  const int64_t nblk = (n + QB - 1) / QB;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblk; blk += (int64_t)gridDim.x * 4) {
    const int64_t e = blk * QB + lane * 4;
    if (e >= n) continue;
    const int64_t ch = blk / bpc, j = blk - ch * bpc;
    const uint8_t* base = q + ch * w.stride;
    const float sc = reinterpret_cast<const float*>(base + w.code_bytes)[j];
    float v[4];
    load_codes<BITS>(base + j * Q<BITS>::BLOCK_BYTES, lane, v);
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = (v[k] * sc) * inv_w;
    if (e + 4 <= n) {
      float4 B = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(buf + e);
      float4 S = *reinterpret_cast<const float4*>(sync + e);
      float4 P;
      P.x = outer_update(d[0], B.x, S.x, 0.f, false, 0.f, lr, mu, first);
      P.y = outer_update(d[1], B.y, S.y, 0.f, false, 0.f, lr, mu, first);
      P.z = outer_update(d[2], B.z, S.z, 0.f, false, 0.f, lr, mu, first);
      P.w = outer_update(d[3], B.w, S.w, 0.f, false, 0.f, lr, mu, first);
      *reinterpret_cast<float4*>(buf + e) = B;
      *reinterpret_cast<float4*>(sync + e) = S;
      *reinterpret_cast<float4*>(p + e) = P;
      if (SDT == BF16) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(sh) + e) = make_uint2(pack2(P.x, P.y), pack2(P.z, P.w));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e + k < n) {
          float b = first ? 0.f : buf[e + k];
          float so = sync[e + k];
          const float np = outer_update(d[k], b, so, 0.f, false, 0.f, lr, mu, first);
          buf[e + k] = b;
          sync[e + k] = so;
          p[e + k] = np;
          if (SDT == BF16) reinterpret_cast<bf16_t*>(sh)[e + k] = f2bf(np);
        }
      }
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// out: nchunks wire chunks of bpc blocks each; block i of the span (elements [256 i, 256 i + 256) of
// sync - master, zero past n) goes to chunk i / bpc.  sync / master: 16-byte aligned; out: 4-byte aligned.
ND_API int nd_pseudograd_q(const float* sync, const float* p, int64_t n, void* out, int64_t nchunks, int64_t bpc,
                           int bits, hipStream_t s) {
  if ((bits != 8 && bits != 4) || n < 0 || nchunks < 1 || bpc < 1 || n > nchunks * bpc * QB) return (int)hipErrorInvalidValue;
  if (!aligned(sync, 16) || !aligned(p, 16) || !aligned(out, 4)) return (int)hipErrorInvalidValue;
  const int64_t nblk = nchunks * bpc;
  uint8_t* o = static_cast<uint8_t*>(out);
  float* none = nullptr;
  if (bits == 8) hipLaunchKernelGGL((pseudograd_q_kernel<8, false>), dim3(q_grid(nblk)), dim3(256), 0, s, sync, p, none, n, o, nblk, bpc);
  else hipLaunchKernelGGL((pseudograd_q_kernel<4, false>), dim3(q_grid(nblk)), dim3(256), 0, s, sync, p, none, n, o, nblk, bpc);
  ND_LAUNCH_CHECK();
}

// nd_pseudograd_q of fl(fl(sync - master) + resid); resid (n fp32, 16-byte aligned) becomes x - code * scale
ND_API int nd_pseudograd_q_ef(const float* sync, const float* p, float* resid, int64_t n, void* out, int64_t nchunks,
                              int64_t bpc, int bits, hipStream_t s) {
  if ((bits != 8 && bits != 4) || n < 0 || nchunks < 1 || bpc < 1 || n > nchunks * bpc * QB) return (int)hipErrorInvalidValue;
  if (!resid || !aligned(resid, 16) || !aligned(sync, 16) || !aligned(p, 16) || !aligned(out, 4)) return (int)hipErrorInvalidValue;
  const int64_t nblk = nchunks * bpc;
  uint8_t* o = static_cast<uint8_t*>(out);
  if (bits == 8) hipLaunchKernelGGL((pseudograd_q_kernel<8, true>), dim3(q_grid(nblk)), dim3(256), 0, s, sync, p, resid, n, o, nblk, bpc);
  else hipLaunchKernelGGL((pseudograd_q_kernel<4, true>), dim3(q_grid(nblk)), dim3(256), 0, s, sync, p, resid, n, o, nblk, bpc);
  ND_LAUNCH_CHECK();
}

// in: nw chunks (worker-rank order) of bpc blocks; out: one chunk = quantise(sum_r dequantise(chunk r))
ND_API int nd_qreduce(const void* in, int nw, int64_t bpc, int bits, void* out, hipStream_t s) {
  if ((bits != 8 && bits != 4) || nw < 1 || nw > 64 || bpc < 1) return (int)hipErrorInvalidValue;
  if (!aligned(in, 4) || !aligned(out, 4)) return (int)hipErrorInvalidValue;
  const uint8_t* i = static_cast<const uint8_t*>(in);
  uint8_t* o = static_cast<uint8_t*>(out);
  float* none = nullptr;
  if (bits == 8) hipLaunchKernelGGL((qreduce_kernel<8, false>), dim3(q_grid(bpc)), dim3(256), 0, s, i, nw, bpc, none, o);
  else hipLaunchKernelGGL((qreduce_kernel<4, false>), dim3(q_grid(bpc)), dim3(256), 0, s, i, nw, bpc, none, o);
  ND_LAUNCH_CHECK();
}

// nd_qreduce of fl(sum + resid); resid (one chunk: bpc * 256 fp32, 16-byte aligned) becomes x - code * scale
ND_API int nd_qreduce_ef(const void* in, int nw, int64_t bpc, int bits, float* resid, void* out, hipStream_t s) {
  if ((bits != 8 && bits != 4) || nw < 1 || nw > 64 || bpc < 1) return (int)hipErrorInvalidValue;
  if (!resid || !aligned(resid, 16) || !aligned(in, 4) || !aligned(out, 4)) return (int)hipErrorInvalidValue;
  const uint8_t* i = static_cast<const uint8_t*>(in);
  uint8_t* o = static_cast<uint8_t*>(out);
  if (bits == 8) hipLaunchKernelGGL((qreduce_kernel<8, true>), dim3(q_grid(bpc)), dim3(256), 0, s, i, nw, bpc, resid, o);
  else hipLaunchKernelGGL((qreduce_kernel<4, true>), dim3(q_grid(bpc)), dim3(256), 0, s, i, nw, bpc, resid, o);
  ND_LAUNCH_CHECK();
}

// nd_outer_nesterov with the pseudo-gradient sum read from gathered wire chunks (q: chunks of bpc blocks,
// element i of the span in block i / 256).  p / sync / buf: 16-byte aligned; sh (bf16): 8-byte aligned.
ND_API int nd_outer_nesterov_q(float* p, float* sync, const void* q, int bits, int64_t bpc, float* buf, void* sh,
                               int shdt, int64_t n, float inv_w, float lr, float mu, int first, hipStream_t s) {
  if ((bits != 8 && bits != 4) || bpc < 1 || n < 0) return (int)hipErrorInvalidValue;
  if (!aligned(p, 16) || !aligned(sync, 16) || !aligned(buf, 16) || !aligned(q, 4) || !aligned(sh, 8))
    return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  const uint8_t* qq = static_cast<const uint8_t*>(q);
  const unsigned grid = q_grid((n + QB - 1) / QB);
  const bool bsh = sh && shdt == BF16;
#define ND_OQ(B, S) hipLaunchKernelGGL((outer_q_kernel<B, S>), dim3(grid), dim3(256), 0, s, p, sync, qq, buf, sh, n, bpc, inv_w, lr, mu, first)
  if (bits == 8) { if (bsh) ND_OQ(8, BF16); else ND_OQ(8, F32); }
  else { if (bsh) ND_OQ(4, BF16); else ND_OQ(4, F32); }
#undef ND_OQ
  ND_LAUNCH_CHECK();
}
