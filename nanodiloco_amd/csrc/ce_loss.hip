// Loss-only cross-entropy over one chunk of lm_head logits (held-out evaluation): per row
//   lse      = logsumexp(x)                                    (fp32)
//   row_loss = valid ? lse - x[target] : 0
//   row_hit  = valid && x[target] == max_j x[j]                (top-1 on the stored values, ties count)
// The logits are const: read once, never written (cross_entropy.hip overwrites them with the gradient and
// therefore holds the row in registers; nothing here needs the row twice).  One 256-thread workgroup per
// row streams it with 16-B loads into a per-thread online (max, sum): m' = max(m, x), s' = s e^(m - m') +
// sum e^(x - m').  At most 64 VGPRs with four loads in flight per thread, so 8 waves fit per SIMD.  The four
// waves' pairs are merged in wave order by one thread: no atomics, no loss_sum -- the result is per-row
// stores only and bitwise repeatable.
// NaN: fmaxf skips it, the sum keeps it (e^(NaN - m) = NaN), so a NaN anywhere in a valid row gives
// lse = row_loss = NaN and row_hit = 0.  A target outside [0, V) that is not `ignore` reads nothing:
// row_loss = NaN, row_hit = 0.  A row of -inf gives lse = -inf as torch.logsumexp does.
#include "common.h"

using namespace nd;

namespace {

struct MS {
  float m, s;
};

// fold 8 values into (m, s): 9 exponentials per 8 elements (one rescale of the running sum)
__device__ __forceinline__ void fold8(MS& a, const float* v) {
  float vm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
  const float nm = fmaxf(a.m, vm);
  const float ref = nm == -INFINITY ? 0.f : nm;  // all -inf so far: e^(-inf - 0) = 0, never -inf + inf
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) t += __expf(v[j] - ref);
  a.s = a.s * __expf(a.m - ref) + t;
  a.m = nm;
}

// one value: exactly one exponential, e^-|v - m| scales whichever side is the smaller
__device__ __forceinline__ void fold1(MS& a, float v) {
  const float d = v - a.m;  // m = -inf: +inf (v finite) or NaN (v = -inf too)
  float e = __expf(-fabsf(d));
  if (v == -INFINITY) e = 0.f;
  a.s = d > 0.f ? a.s * e + 1.f : a.s + e;  // NaN v: d > 0 is false, s + NaN
  a.m = fmaxf(a.m, v);
}

// VEC: V % 8 == 0 and a 16-B aligned base, 8 elements per thread and step; else one element per thread and step
template <int DT, bool VEC>
__global__ void __launch_bounds__(256) ce_loss_kernel(const void* __restrict__ logits, const int64_t* __restrict__ targets,
                                                      int V, int ignore, float* __restrict__ row_loss,
                                                      float* __restrict__ lse_out, uint8_t* __restrict__ row_hit) {
  __shared__ float red_m[4], red_s[4], picked_sh;
  const int64_t row = blockIdx.x;
  const int64_t base = row * (int64_t)V;
  const int64_t tgt = targets[row];
  const bool valid = tgt != (int64_t)ignore;
  if (threadIdx.x == 0) picked_sh = __uint_as_float(0x7fc00000u);  // no thread owns the target: NaN
  __syncthreads();
  MS a{-INFINITY, 0.f};
  if constexpr (VEC) {
#pragma unroll 4
    for (int col = threadIdx.x * 8; col < V; col += 256 * 8) {
      float v[8];
      Vec8<DT>::load(logits, base + col, v);
      const uint64_t d = (uint64_t)(tgt - col);
      if (d < 8u) {  // this thread holds the target column
        float p = v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) p = d == (uint64_t)j ? v[j] : p;
        picked_sh = p;
      }
      fold8(a, v);
    }
  } else {
#pragma unroll 4
    for (int col = threadIdx.x; col < V; col += 256) {
      float v;
      if constexpr (DT == BF16) v = bf2f(reinterpret_cast<const bf16_t*>(logits)[base + col]);
      else v = reinterpret_cast<const float*>(logits)[base + col];
      if ((int64_t)col == tgt) picked_sh = v;
      fold1(a, v);
    }
  }
  // wave (max, sum), then the four waves in order
  const float wm = wave_max(a.m);
  const float wref = wm == -INFINITY ? 0.f : wm;
  const float ws = wave_sum(a.s * __expf(a.m - wref));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red_m[w] = wm;
    red_s[w] = ws;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    const float ref = m == -INFINITY ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += red_s[i] * __expf(red_m[i] - ref);
    const float lse = m + __logf(s);
    const float picked = picked_sh;
    if (lse_out) lse_out[row] = lse;
    row_loss[row] = valid ? lse - picked : 0.f;
    if (row_hit) row_hit[row] = (valid && s == s && picked == m) ? 1 : 0;
  }
}

template <int DT>
void launch(const void* logits, const int64_t* targets, int64_t n, int V, int ignore, float* row_loss, float* lse_out,
            uint8_t* row_hit, hipStream_t s) {
  dim3 g((unsigned)n), b(256);
  if (V % 8 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL((ce_loss_kernel<DT, true>), g, b, 0, s, logits, targets, V, ignore, row_loss, lse_out, row_hit);
  else
    hipLaunchKernelGGL((ce_loss_kernel<DT, false>), g, b, 0, s, logits, targets, V, ignore, row_loss, lse_out, row_hit);
}

}  // namespace

// logits [n, V] contiguous (dt: F32 | BF16), targets [n]; row_loss [n]; lse_out [n] and row_hit [n] may be null.
ND_API int nd_ce_loss(const void* logits, int dt, const int64_t* targets, int64_t n, int V, int ignore,
                      float* row_loss, float* lse_out, uint8_t* row_hit, hipStream_t s) {
  if (n <= 0) return 0;
  if (V < 1 || n > 0x7fffffffLL || (dt != BF16 && dt != F32) || !logits || !targets || !row_loss)
    return (int)hipErrorInvalidValue;
  if (dt == BF16) launch<BF16>(logits, targets, n, V, ignore, row_loss, lse_out, row_hit, s);
  else launch<F32>(logits, targets, n, V, ignore, row_loss, lse_out, row_hit, s);
  ND_LAUNCH_CHECK();
}
