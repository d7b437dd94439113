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
//
// Logit soft-capping (nd_ce_loss_cap; softcap.h): the instantiations with a trailing CapArgs fold y = C tanh(x / C),
// formed in fp32 from the stored x, so lse and row_loss = lse - y[target] are those of the capped logits.  row_hit
// stays defined on the stored values -- two different logits may saturate to the same y -- so these kernels carry the
// raw maximum beside the (max, sum) of the capped row and row_hit is bitwise the uncapped call's.
//
// nd_logit_softcap: y = C tanh(x / C) in place over a flat bf16 / fp32 buffer (the logits the model hands out:
// forward().logits, prefill, decode_step), any element alignment, any length.
#include "common.h"
#include "softcap.h"

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
// CA: empty (the plain kernel) or one CapArgs (CAP = true)
template <int DT, bool VEC, class... CA>
__global__ void __launch_bounds__(256) ce_loss_kernel(const void* __restrict__ logits, const int64_t* __restrict__ targets,
                                                      int V, int ignore, float* __restrict__ row_loss,
                                                      float* __restrict__ lse_out, uint8_t* __restrict__ row_hit,
                                                      CA... ca) {
  constexpr bool CAP = sizeof...(CA) > 0;
  __shared__ float red_m[4], red_s[4], picked_sh;
  [[maybe_unused]] __shared__ float red_r[4];  // CAP: the waves' raw maxima
  [[maybe_unused]] float cap = 0.f, cinv = 0.f, rawm = -INFINITY;
  if constexpr (CAP) {
    const CapArgs c = (ca, ...);
    cap = c.cap;
    cinv = c.inv;
  }
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
      if constexpr (CAP) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          rawm = fmaxf(rawm, v[j]);
          v[j] = cap * cap_tanh(v[j] * cinv);
        }
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
      if constexpr (CAP) {
        rawm = fmaxf(rawm, v);
        v = cap * cap_tanh(v * cinv);
      }
      fold1(a, v);
    }
  }
  // wave (max, sum), then the four waves in order
  const float wm = wave_max(a.m);
  const float wref = wm == -INFINITY ? 0.f : wm;
  const float ws = wave_sum(a.s * __expf(a.m - wref));
  const int w = threadIdx.x >> 6;
  if constexpr (CAP) rawm = wave_max(rawm);
  if ((threadIdx.x & 63) == 0) {
    red_m[w] = wm;
    red_s[w] = ws;
    if constexpr (CAP) red_r[w] = rawm;
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
    if constexpr (CAP) {
      row_loss[row] = valid ? lse - cap * cap_tanh(picked * cinv) : 0.f;
      const float rm = fmaxf(fmaxf(red_r[0], red_r[1]), fmaxf(red_r[2], red_r[3]));
      if (row_hit) row_hit[row] = (valid && s == s && picked == rm) ? 1 : 0;
    } else {
      row_loss[row] = valid ? lse - picked : 0.f;
      if (row_hit) row_hit[row] = (valid && s == s && picked == m) ? 1 : 0;
    }
  }
}

template <int DT, class... CA>
void launch(const void* logits, const int64_t* targets, int64_t n, int V, int ignore, float* row_loss, float* lse_out,
            uint8_t* row_hit, hipStream_t s, CA... ca) {
  dim3 g((unsigned)n), b(256);
  if (V % 8 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0)
    hipLaunchKernelGGL((ce_loss_kernel<DT, true, CA...>), g, b, 0, s, logits, targets, V, ignore, row_loss, lse_out, row_hit, ca...);
  else
    hipLaunchKernelGGL((ce_loss_kernel<DT, false, CA...>), g, b, 0, s, logits, targets, V, ignore, row_loss, lse_out, row_hit, ca...);
}

// 16-B groups (G elements) from the first aligned element on, the elements before it and the tail one by one
template <int DT>
__global__ void __launch_bounds__(256) softcap_kernel(void* __restrict__ x, int64_t n, int64_t head, CapArgs c) {
  constexpr int G = DT == BF16 ? 8 : 4;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
  const int64_t groups = (n - head) / G;
  for (int64_t g = tid; g < groups; g += nt) {
    const int64_t i = head + g * G;
    if constexpr (DT == BF16) {
      float v[8];
      Vec8<BF16>::load(x, i, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = c.cap * cap_tanh(v[j] * c.inv);
      Vec8<BF16>::store(x, i, v);
    } else {
      float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(x) + i);
      v.x = c.cap * cap_tanh(v.x * c.inv);
      v.y = c.cap * cap_tanh(v.y * c.inv);
      v.z = c.cap * cap_tanh(v.z * c.inv);
      v.w = c.cap * cap_tanh(v.w * c.inv);
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(x) + i) = v;
    }
  }
  const int64_t tail0 = head + groups * G, rest = head + (n - tail0);
  for (int64_t k = tid; k < rest; k += nt) {
    const int64_t i = k < head ? k : tail0 + (k - head);
    if constexpr (DT == BF16) {
      bf16_t* p = reinterpret_cast<bf16_t*>(x) + i;
      *p = f2bf(c.cap * cap_tanh(bf2f(*p) * c.inv));
    } else {
      float* p = reinterpret_cast<float*>(x) + i;
      *p = c.cap * cap_tanh(*p * c.inv);
    }
  }
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

// The same over capped logits y = cap * tanh(x / cap): row_loss and lse_out are those of y, row_hit stays the top-1 on
// the stored values (bitwise nd_ce_loss's).  A cap that is <= 0, NaN or infinite is refused.
ND_API int nd_ce_loss_cap(const void* logits, int dt, const int64_t* targets, int64_t n, int V, int ignore,
                          float* row_loss, float* lse_out, uint8_t* row_hit, float cap, hipStream_t s) {
  if (!cap_ok(cap)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (V < 1 || n > 0x7fffffffLL || (dt != BF16 && dt != F32) || !logits || !targets || !row_loss)
    return (int)hipErrorInvalidValue;
  if (dt == BF16) launch<BF16>(logits, targets, n, V, ignore, row_loss, lse_out, row_hit, s, cap_args(cap));
  else launch<F32>(logits, targets, n, V, ignore, row_loss, lse_out, row_hit, s, cap_args(cap));
  ND_LAUNCH_CHECK();
}

// x [n] (dt: F32 | BF16, element-aligned) <- cap * tanh(x / cap), in place.
ND_API int nd_logit_softcap(void* x, int dt, int64_t n, float cap, hipStream_t s) {
  if (!cap_ok(cap) || (dt != BF16 && dt != F32) || n < 0 || (n > 0 && !x)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int64_t esz = dt == BF16 ? 2 : 4, G = 16 / esz;
  const uintptr_t a = reinterpret_cast<uintptr_t>(x);
  if (a % esz) return (int)hipErrorInvalidValue;
  int64_t head = (int64_t)(((16 - a % 16) % 16) / esz);
  if (head > n) head = n;
  const int64_t work = (n - head) / G + G + head;  // threads that have something to do, at most
  const unsigned blocks = (unsigned)(work / 256 + 1 < 4096 ? work / 256 + 1 : 4096);
  if (dt == BF16) hipLaunchKernelGGL(softcap_kernel<BF16>, dim3(blocks), dim3(256), 0, s, x, n, head, cap_args(cap));
  else hipLaunchKernelGGL(softcap_kernel<F32>, dim3(blocks), dim3(256), 0, s, x, n, head, cap_args(cap));
  ND_LAUNCH_CHECK();
}
