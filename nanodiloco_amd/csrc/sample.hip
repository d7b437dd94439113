// Fused sampler of the decode step: temperature, top-k, top-p and the draw in one launch (nd_sample_topk_topp).
//
// Contract (ops/sample.py states it again; the PyTorch twin there follows the same rules).  Per row of fp32 logits
// l[0..V), with x = l / temperature:
//   top-k  (0 < top_k < V)  keep every token whose logit is >= the k-th largest (ties at the threshold all stay)
//   top-p  (top_p < 1)      on what top-k kept: Z the kept mass, G(v) the mass of the kept logits strictly greater
//                           than v; the threshold is the smallest kept logit v with G(v) / Z < top_p; keep >= it
//   draw                    over the kept tokens in index order, masses m_i, total Z': the smallest kept index j whose
//                           inclusive prefix mass exceeds u Z'
//   thr = the smallest kept logit (the input value; -0 reads +0), nkept = the number of kept tokens
// -inf logits are legal (mass 0; never returned).  A row of -inf only, or one with a NaN, is outside the contract.
//
// Nothing here sorts.  Both thresholds are found by an MSB-first radix select (four levels of 8 bits) on
// order-preserving uint32 keys of the logits: per level a 256-bin LDS histogram filled by integer atomics, then one
// wave scans the bins from the top (a suffix scan by lane shuffles) and picks the bin that holds the threshold.
//   top-k  count histogram; the bin with  count(above) < r <= count(above) + count(bin)
//   top-p  mass histogram beside a count histogram (a bin whose elements all round to mass 0 is still non-empty);
//          the lowest non-empty bin whose mass above is < top_p Z.  G is non-increasing in v, so the logits that
//          qualify are an upper set and that bin holds its minimum
// Masses are 64-bit fixed point, m = rint(exp2((l - l_max) log2e / temperature) 2^40): integer sums are associative,
// so LDS atomics (ds_add_u32 / ds_add_u64), wave reductions and prefix scans give the same bits in any order and the
// result depends on the row alone -- not on B, the block size or occupancy.  No floating-point atomics.  top_p Z and
// u Z' are formed exactly in 128-bit integers (top_p = pm 2^-ps with a 24-bit pm; floor(u 2^24)).
//
// One workgroup of 1024 threads per row; wave w owns the contiguous indices [w seg, (w + 1) seg), lane-strided, so
// every global load is a 256-byte wave access and index order for the draw is wave order.  The draw reduces the waves'
// kept masses, finds the wave that holds the target and scans that wave's segment 64 elements at a time with a wave
// prefix sum.  RES (V <= RES_MAX): the row is read from global memory once, its keys stay in dynamic LDS for every later
// pass.  Otherwise the same passes re-read the row (L2-resident: 513 KB at V = 128256).  RES_MAX = 39936 keys = 156 KB:
// gfx950 has 160 KB of LDS per CU and the histograms and reduction slots take under 4 KB.
// A stage that is off is skipped.  The grid is B workgroups, nothing is read on the host: graph-capturable.
#include "common.h"
#include <math.h>

using namespace nd;

namespace {

constexpr int NT = 1024, NW = NT / 64;
constexpr int RES_MAX = 39936;
constexpr int MAX_V = 1 << 20;          // V 2^40-masses sum below 2^60
constexpr float MASS_ONE = 1099511627776.f;  // 2^40

// fp32 -> uint32 whose unsigned order is the float order (-0 joins +0); from_key is its inverse
__device__ __forceinline__ uint32_t to_key(float x) {
  uint32_t b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_key(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
// c = log2e / temperature.  v_exp_f32 flushes below 2^-126: those masses round to 0 anyway
__device__ __forceinline__ uint64_t mass_of(uint32_t key, float lmax, float c) {
  return (uint64_t)rintf(__builtin_amdgcn_exp2f((from_key(key) - lmax) * c) * MASS_ONE);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Shared {
  unsigned long long mass[256];  // per-digit kept mass of the level
  uint32_t cnt[256];             // per-digit element count of the level
  unsigned long long wmass[NW];  // draw: kept mass per wave
  uint32_t wcnt[NW], wmax[NW], wmin[NW];
  unsigned long long sel_above;  // top-p: mass above the chosen bin
  uint32_t sel_bin, sel_r;       // the chosen digit; top-k: the rank left inside it
};

// One wave: lane l holds bins 4l .. 4l+3.  The bin with count(above) < r <= count(above) + count(bin).
__device__ __forceinline__ void select_count(Shared& sh, uint32_t r, int lane) {
  const uint4 c4 = reinterpret_cast<const uint4*>(sh.cnt)[lane];
  const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
  const uint32_t own = c[0] + c[1] + c[2] + c[3];
  uint32_t incl = own;  // suffix sum over lanes >= lane
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_down(incl, o, 64);
    if (lane + o < 64) incl += t;
  }
  uint32_t above = incl - own;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (above < r && above + c[j] >= r) {
      sh.sel_bin = 4 * lane + j;
      sh.sel_r = r - above;
    }
    above += c[j];
  }
}

// One wave: the lowest non-empty bin whose mass above (gacc + the bins over it) is < P.  Level 0 (P == nullptr -> the
// total is the kept mass Z): P = ceil(top_p Z) = ceil(Z pm / 2^ps) is formed here and returned.
__device__ __forceinline__ uint64_t select_mass(Shared& sh, uint64_t gacc, uint64_t P, bool first, uint32_t pm, int ps,
                                                int lane) {
  const uint4 c4 = reinterpret_cast<const uint4*>(sh.cnt)[lane];
  const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
  uint64_t m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = sh.mass[4 * lane + j];
  const uint64_t own = m[0] + m[1] + m[2] + m[3];
  uint64_t incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_down((unsigned long long)incl, o, 64);
    if (lane + o < 64) incl += t;
  }
  if (first) {
    const uint64_t Z = __shfl((unsigned long long)incl, 0, 64);
    const unsigned __int128 pr = (unsigned __int128)Z * pm;
    const unsigned __int128 fl = pr >> ps;
    P = (uint64_t)fl + ((fl << ps) != pr ? 1u : 0u);
  }
  uint64_t above = gacc + incl - own, best_above = 0;
  int best = -1;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (c[j] != 0 && above < P) {
      best = j;
      best_above = above;
    }
    above += m[j];
  }
  // bins rise with the lane: the lowest lane that found one owns the lowest qualifying bin
  const uint64_t found = __ballot(best >= 0);
  if (lane == __ffsll((unsigned long long)found) - 1) {
    sh.sel_bin = 4 * lane + best;
    sh.sel_above = best_above;
  }
  return P;
}

template <bool RES>
__global__ void __launch_bounds__(NT) sample_topk_topp_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ u, int64_t* __restrict__ tok,
                                                              float* __restrict__ thr, int* __restrict__ nkept, int V,
                                                              int64_t ld, float c, int top_k, uint32_t pm, int ps) {
  extern __shared__ __attribute__((aligned(16))) uint32_t keys[];  // RES: the row's V keys
  __shared__ __attribute__((aligned(16))) Shared sh;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const float* __restrict__ row = logits + (int64_t)blockIdx.x * ld;
  const int seg = (V + NT - 1) / NT * 64;  // indices per wave, a multiple of 64
  const int lo = min(w * seg, V), hi = min(lo + seg, V);
  const bool do_k = top_k > 0 && top_k < V, do_p = pm != 0;
  auto key_at = [&](int i) -> uint32_t {
    if constexpr (RES) return keys[i];
    else return to_key(row[i]);
  };

  // ---- the row, once: keys (to LDS), extrema, and the top-k count histogram of the leading digit
  if (tid < 256) sh.cnt[tid] = 0u;
  __syncthreads();
  uint32_t kmax = 0u, kmin = 0xffffffffu;
#pragma unroll 8
  for (int i = lo + lane; i < hi; i += 64) {
    const uint32_t k = to_key(row[i]);
    if constexpr (RES) keys[i] = k;
    kmax = max(kmax, k);
    kmin = min(kmin, k);
    if (do_k) atomicAdd(&sh.cnt[k >> 24], 1u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, 64));
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, 64));
  }
  if (lane == 0) {
    sh.wmax[w] = kmax;
    sh.wmin[w] = kmin;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    kmax = max(kmax, sh.wmax[j]);
    kmin = min(kmin, sh.wmin[j]);
  }
  const float lmax = from_key(kmax);

  // ---- top-k: the key of the k-th largest logit
  uint32_t T = 0u;  // the threshold key; 0 keeps everything
  if (do_k) {
    uint32_t r = (uint32_t)top_k;
    for (int lvl = 0; lvl < 4; ++lvl) {
      const int s = 24 - 8 * lvl;
      if (lvl > 0) {
        if (tid < 256) sh.cnt[tid] = 0u;
        __syncthreads();
        const uint32_t himask = 0xffffffffu << (s + 8);
        for (int i = lo + lane; i < hi; i += 64) {
          const uint32_t k = key_at(i);
          if ((k & himask) == T) atomicAdd(&sh.cnt[(k >> s) & 255u], 1u);
        }
        __syncthreads();
      }
      if (w == 0) select_count(sh, r, lane);
      __syncthreads();
      T |= sh.sel_bin << s;
      r = sh.sel_r;
    }
  }

  // ---- top-p: the smallest kept key whose mass above is below top_p Z
  if (do_p) {
    uint32_t prefix = 0u;
    uint64_t gacc = 0u, P = 0u;
    for (int lvl = 0; lvl < 4; ++lvl) {
      const int s = 24 - 8 * lvl;
      __syncthreads();  // the last level's picks are read
      if (tid < 256) {
        sh.cnt[tid] = 0u;
        sh.mass[tid] = 0u;
      }
      __syncthreads();
      const uint32_t himask = lvl ? 0xffffffffu << (s + 8) : 0u;
      for (int i = lo + lane; i < hi; i += 64) {
        const uint32_t k = key_at(i);
        if (k >= T && (k & himask) == prefix) {
          const uint32_t d = (k >> s) & 255u;
          atomicAdd(&sh.cnt[d], 1u);
          const uint64_t m = mass_of(k, lmax, c);
          if (m) atomicAdd(&sh.mass[d], (unsigned long long)m);
        }
      }
      __syncthreads();
      if (w == 0) P = select_mass(sh, gacc, P, lvl == 0, pm, ps, lane);
      __syncthreads();
      prefix |= sh.sel_bin << s;
      gacc = sh.sel_above;
    }
    T = prefix;  // a kept key, so >= the top-k threshold
  }

  // ---- draw: kept mass per wave, the wave that holds the target, a prefix scan of its segment
  uint64_t wm = 0u;
  uint32_t wc = 0u;
  for (int i = lo + lane; i < hi; i += 64) {
    const uint32_t k = key_at(i);
    if (k >= T) {
      wm += mass_of(k, lmax, c);
      ++wc;
    }
  }
  wm = wave_sum_u64(wm);
  wc = wave_sum_u32(wc);
  if (lane == 0) {
    sh.wmass[w] = wm;
    sh.wcnt[w] = wc;
  }
  __syncthreads();
  uint64_t Zk = 0u, before = 0u;
  uint32_t n = 0u;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    Zk += sh.wmass[j];
    n += sh.wcnt[j];
    if (j < w) before += sh.wmass[j];
  }
  if (tid == 0) {
    if (thr) thr[blockIdx.x] = from_key(do_k || do_p ? T : kmin);
    if (nkept) nkept[blockIdx.x] = (int)n;
  }
  // the smallest j with prefix(j) > u Z'  <=>  prefix(j) > floor(U Z' / 2^24), U = floor(u 2^24) < 2^24
  const int U = min(max((int)(u[blockIdx.x] * 16777216.f), 0), 16777215);
  const uint64_t tgt = (uint64_t)(((unsigned __int128)Zk * (uint32_t)U) >> 24);
  if (before <= tgt && tgt < before + wm) {  // exactly one wave: tgt < Z'
    uint64_t run = before;
    for (int base = lo; base < hi; base += 64) {
      const int i = base + lane;
      uint64_t m = 0u;
      if (i < hi) {
        const uint32_t k = key_at(i);
        if (k >= T) m = mass_of(k, lmax, c);
      }
      uint64_t incl = m;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, o, 64);
        if (lane >= o) incl += t;
      }
      const uint64_t hit = __ballot(run + incl > tgt);
      if (hit) {  // the first lane past the target added mass there: a kept token
        if (lane == __ffsll((unsigned long long)hit) - 1) tok[blockIdx.x] = (int64_t)i;
        break;
      }
      run += __shfl((unsigned long long)incl, 63, 64);
    }
  }
}

// Raises the dynamic-LDS limit of the resident kernel (once, on first use); returns that call's error.
hipError_t resident_lds() {
  static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_topk_topp_kernel<true>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, RES_MAX * 4);
  return e;
}

}  // namespace

// logits fp32 [B, V] with row stride ld >= V; u fp32 [B] in [0, 1); tok int64 [B]; thr fp32 [B] and nkept int32 [B] may
// be null.  temperature > 0; top_k >= 0 (0 or >= V: off); 0 < top_p <= 1 (1: off).  V <= 2^20.
ND_API int nd_sample_topk_topp(const float* logits, const float* u, int64_t* tok, float* thr, int* nkept, int B, int V,
                               int64_t ld, float temperature, int top_k, float top_p, hipStream_t s) {
  if (B == 0) return 0;
  if (B < 0 || V < 1 || V > MAX_V || ld < V || !logits || !u || !tok || !(temperature > 0.f) || isinf(temperature) ||
      top_k < 0 || !(top_p > 0.f && top_p <= 1.f))
    return (int)hipErrorInvalidValue;
  const float c = (float)(1.4426950408889634 / (double)temperature);
  uint32_t pm = 0u;  // top_p = pm 2^-ps exactly; pm = 0: top-p off
  int ps = 0;
  if (top_p < 1.f) {
    int e;
    pm = (uint32_t)ldexpf(frexpf(top_p, &e), 24);
    ps = 24 - e;
    if (ps > 100) ps = 100;  // Z pm < 2^84: the quotient is in (0, 1) either way and its ceiling is 1
  }
  if (V <= RES_MAX) {
    const hipError_t e = resident_lds();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sample_topk_topp_kernel<true>, dim3((unsigned)B), dim3(NT), (size_t)((V + 3) / 4 * 16), s, logits,
                       u, tok, thr, nkept, V, ld, c, top_k, pm, ps);
  } else {
    hipLaunchKernelGGL(sample_topk_topp_kernel<false>, dim3((unsigned)B), dim3(NT), 0, s, logits, u, tok, thr, nkept, V,
                       ld, c, top_k, pm, ps);
  }
  ND_LAUNCH_CHECK();
}
