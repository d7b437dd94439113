// Single-query (decode) attention against a KV cache, with the new token's RoPE and cache append fused in.
//
// One decode step of one layer for B sequences.  Inputs: the plain (un-rotated) q|k|v projection row of the new
// token, qkv [B, (nh + 2 nkv) * hd] bf16; the fp32 RoPE tables [S, hd]; pos[b] (device int32: the cache slot and RoPE
// position of the new token); kstart[b] (device int32 or null: first real key, left padding); the caches
// [B, nkv, S_max, hd] bf16.  Output o [B, nh * hd] bf16 = softmax(scale q k^T) v over keys kstart[b] .. pos[b].
//
// Two launches on one stream, no atomics, no hand-off between workgroups inside a launch:
//   attn_decode_kernel   grid (nkv, B, ceil(S_max / SPLIT)), 256 threads.  Workgroup (c, g, b) owns keys
//                        [c SPLIT, (c+1) SPLIT) of kv head g of sequence b and writes the fp32 partial
//                        (m, l, o[rep][hd]) of ALL rep = nh / nkv query heads of the group: every K/V row is read once.
//                        A chunk outside [kstart, pos] writes the empty partial (m = -inf, l = 0) and leaves.  The
//                        workgroup whose chunk holds pos[b] also writes the rotated k row and the v row to slot pos[b].
//   attn_decode_combine  grid (nh, B), hd threads: merges a head's partials in chunk order (the chunks that meet
//                        [kstart, pos]), writes bf16 o.
// The partition depends on SPLIT and the key index alone (not on the grid, B, pos or occupancy), the grid on the
// static S_max: the launch has one shape for every step (HIP-graph capturable), and a sequence gets the same bits
// alone or in any batch.
//
// Inside a workgroup: wave w takes keys [w SPLIT/4, (w+1) SPLIT/4) of the chunk.  A K/V row is hd/8 lanes x 16 B, so
// one dwordx4 load per lane brings 64 / (hd/8) rows per wave, straight into VGPRs (no LDS staging); all of the wave's
// K and V loads are issued before the first use.  Scores are fp32 VALU dot products reduced over the hd/8 lanes of a
// row; the wave's 32 scores per head stay in registers, so the softmax inside a wave is exact two-pass (max, then
// exp2 and P V) and only the four waves and the chunks are merged online-softmax style, in fixed order.
// The new token's q (rep heads) and k are rotated in registers by every workgroup that needs them with the
// arithmetic of rope.hip -- t = x_partner * sin, y = fma(x, cos, -+t), one rounding to bf16 -- written with explicit
// fma so that the bits do not depend on what the compiler contracts; key pos[b] is taken from these registers, never
// read back from the cache.  Slots beyond pos[b] are never loaded.
#include "common.h"

using namespace nd;

namespace {

constexpr int SPLIT = 128;          // keys per workgroup (compile-time: the partition of the key range)
constexpr int DEC_WAVES = 4;
constexpr int KPW = SPLIT / DEC_WAVES;  // keys per wave
constexpr float LOG2E = 1.4426950408889634f;

// rope.hip's rotation of 8 elements x (this lane's) with partner xp (element i +- hd/2), as that kernel compiles:
// first half:  y1 = fma(x1, c, -(x2 * s));  second half:  y2 = fma(x2, c, x1 * s).  Rounded once to bf16.
__device__ __forceinline__ uint4 rope8(uint4 x, uint4 xp, const float* c, const float* s, bool second) {
#pragma clang fp contract(off)
  const float a[8] = {lo_bf(x.x), hi_bf(x.x), lo_bf(x.y), hi_bf(x.y), lo_bf(x.z), hi_bf(x.z), lo_bf(x.w), hi_bf(x.w)};
  const float p[8] = {lo_bf(xp.x), hi_bf(xp.x), lo_bf(xp.y), hi_bf(xp.y), lo_bf(xp.z), hi_bf(xp.z), lo_bf(xp.w), hi_bf(xp.w)};
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = p[j] * s[j];
    y[j] = __builtin_fmaf(a[j], c[j], second ? t : -t);
  }
  uint4 r;
  r.x = pack2(y[0], y[1]); r.y = pack2(y[2], y[3]); r.z = pack2(y[4], y[5]); r.w = pack2(y[6], y[7]);
  return r;
}

__device__ __forceinline__ void unpack8(uint4 a, float* v) {
  v[0] = lo_bf(a.x); v[1] = hi_bf(a.x); v[2] = lo_bf(a.y); v[3] = hi_bf(a.y);
  v[4] = lo_bf(a.z); v[5] = hi_bf(a.z); v[6] = lo_bf(a.w); v[7] = hi_bf(a.w);
}

// HD: head dimension; REP: compile-time bound (power of two) of the run-time group size rep = nh / nkv <= REP.
// Query slots r >= rep repeat the group's last head and are not written.
template <int HD, int REP>
__global__ void __launch_bounds__(64 * DEC_WAVES)
attn_decode_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ cosT, const float* __restrict__ sinT,
                   const int* __restrict__ pos, const int* __restrict__ kstart, bf16_t* __restrict__ kcache,
                   bf16_t* __restrict__ vcache, float* __restrict__ part_o, float* __restrict__ part_ml, int nh,
                   int nkv, int rep, int S_max, int64_t ld, float scale2, int window) {
  constexpr int LPR = HD / 8;       // lanes per K/V row
  constexpr int KPI = 64 / LPR;     // rows per wave-wide load
  constexpr int ITER = KPW / KPI;   // loads per lane for the wave's keys
  static_assert(KPW % KPI == 0, "a wave's key slice must be whole loads");
  __shared__ float sm_m[DEC_WAVES][REP], sm_l[DEC_WAVES][REP];
  __shared__ float sm_o[DEC_WAVES][REP][HD];

  // the chunk is the slowest grid dimension: workgroups go to the XCDs round-robin in linear order, and with the
  // chunk fastest a power-of-two chunk count would put every workgroup of chunk c on XCD c % 8 -- a short cache (one
  // live chunk) would run on an eighth of the chip
  const int g = blockIdx.x, b = blockIdx.y, c = blockIdx.z;
  const int nchunks = gridDim.z;
  const int p = pos[b];
  // window > 0 (sliding window, counts the query): keys below p - window + 1 are out of sight like those below kstart
  const int ks = max(kstart ? max(kstart[b], 0) : 0, (window > 0 && (unsigned)p < (unsigned)S_max) ? p - window + 1 : 0);
  const int64_t pbase = ((int64_t)(b * nkv + g) * nchunks + c) * rep;  // this workgroup's first partial row
  const int c0 = c * SPLIT;
  const bool holds_p = c0 <= p && p < c0 + SPLIT;  // this workgroup appends (even when kstart leaves it no key)
  // nothing of [ks, p] in this chunk (or a position outside the cache: nothing is read or written): empty partial
  if ((unsigned)p >= (unsigned)S_max || (!holds_p && (c0 > p || c0 + SPLIT <= ks))) {
    if ((int)threadIdx.x < rep) {
      part_ml[(pbase + threadIdx.x) * 2] = -INFINITY;
      part_ml[(pbase + threadIdx.x) * 2 + 1] = 0.f;
    }
    return;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ksub = lane / LPR, dg = lane % LPR;
  const int d0 = dg * 8;
  constexpr int HALF = HD / 2;
  const bool second = d0 >= HALF;
  const int dp = second ? d0 - HALF : d0 + HALF;  // the partner elements of the rotation
  const int i0 = second ? d0 - HALF : d0;         // table columns (first half of the table row)

  // ---- the new token: rotate q (rep heads) and k, take v; every lane for its 8 columns
  const bf16_t* row = qkv + (int64_t)b * ld;
  float cc[8], ss[8];
  {
    const float4* cp = reinterpret_cast<const float4*>(cosT + (int64_t)p * HD + i0);
    const float4* sp = reinterpret_cast<const float4*>(sinT + (int64_t)p * HD + i0);
    const float4 c0v = cp[0], c1v = cp[1], s0v = sp[0], s1v = sp[1];
    cc[0] = c0v.x; cc[1] = c0v.y; cc[2] = c0v.z; cc[3] = c0v.w; cc[4] = c1v.x; cc[5] = c1v.y; cc[6] = c1v.z; cc[7] = c1v.w;
    ss[0] = s0v.x; ss[1] = s0v.y; ss[2] = s0v.z; ss[3] = s0v.w; ss[4] = s1v.x; ss[5] = s1v.y; ss[6] = s1v.z; ss[7] = s1v.w;
  }
  const bf16_t* kin = row + (int64_t)(nh + g) * HD;
  const bf16_t* vin = row + (int64_t)(nh + nkv + g) * HD;
  const uint4 knew = rope8(*reinterpret_cast<const uint4*>(kin + d0), *reinterpret_cast<const uint4*>(kin + dp), cc, ss,
                           second);
  const uint4 vnew = *reinterpret_cast<const uint4*>(vin + d0);
  bf16_t* kc = kcache + (int64_t)(b * nkv + g) * S_max * HD;
  bf16_t* vc = vcache + (int64_t)(b * nkv + g) * S_max * HD;
  if (holds_p && threadIdx.x < LPR) {  // append
    *reinterpret_cast<uint4*>(kc + (int64_t)p * HD + d0) = knew;
    *reinterpret_cast<uint4*>(vc + (int64_t)p * HD + d0) = vnew;
  }

  // ---- this wave's K and V rows, all loads in flight before the first use
  const int kbase = c0 + w * KPW + ksub;
  uint4 kraw[ITER], vraw[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int key = kbase + it * KPI;
    kraw[it] = make_uint4(0, 0, 0, 0);
    vraw[it] = make_uint4(0, 0, 0, 0);
    if (key >= ks && key < p) {  // key < p <= S_max - 1: inside the cache
      kraw[it] = *reinterpret_cast<const uint4*>(kc + (int64_t)key * HD + d0);
      vraw[it] = *reinterpret_cast<const uint4*>(vc + (int64_t)key * HD + d0);
    } else if (key == p) {
      kraw[it] = knew;
      vraw[it] = vnew;
    }
  }

  float q[REP][8];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const bf16_t* qin = row + (int64_t)(g * rep + min(r, rep - 1)) * HD;
    unpack8(rope8(*reinterpret_cast<const uint4*>(qin + d0), *reinterpret_cast<const uint4*>(qin + dp), cc, ss, second),
            q[r]);
  }

  // ---- scores (log2 domain), -inf outside [ks, p]
  float s[REP][ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int key = kbase + it * KPI;
    const bool valid = key >= ks && key <= p;
    float kf[8];
    unpack8(kraw[it], kf);
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(q[r][j], kf[j], acc);
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      s[r][it] = valid ? acc * scale2 : -INFINITY;
    }
  }

  // ---- the wave's softmax (exact two-pass over its KPW keys) and P V
  float m[REP], l[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    float mx = s[r][0];
#pragma unroll
    for (int it = 1; it < ITER; ++it) mx = fmaxf(mx, s[r][it]);
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    m[r] = mx;
    const float ms = mx == -INFINITY ? 0.f : mx;  // a wave without a key: every p below is exp2(-inf) = 0
    float sum = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      s[r][it] = __builtin_amdgcn_exp2f(s[r][it] - ms);
      sum += s[r][it];
    }
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
    l[r] = sum;
  }
  float acc[REP][8];
#pragma unroll
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    float vf[8];
    unpack8(vraw[it], vf);
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(s[r][it], vf[j], acc[r][j]);
  }
#pragma unroll
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) acc[r][j] += __shfl_xor(acc[r][j], o, 64);

  // ---- the four waves, merged in wave order
  if (ksub == 0) {
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_o[w][r][d0 + j] = acc[r][j];
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      sm_m[w][r] = m[r];
      sm_l[w][r] = l[r];
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < rep * HD; t += 64 * DEC_WAVES) {
    const int r = t / HD, d = t % HD;
    float M = sm_m[0][r];
#pragma unroll
    for (int i = 1; i < DEC_WAVES; ++i) M = fmaxf(M, sm_m[i][r]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int i = 0; i < DEC_WAVES; ++i) {
      const float mi = sm_m[i][r];
      const float f = mi == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mi - M);
      L = __builtin_fmaf(sm_l[i][r], f, L);
      O = __builtin_fmaf(sm_o[i][r][d], f, O);
    }
    part_o[(pbase + r) * HD + d] = O;
    if (d == 0) {
      part_ml[(pbase + r) * 2] = M;
      part_ml[(pbase + r) * 2 + 1] = L;
    }
  }
}

// grid (nh, B), hd threads: o[b, h, :] from the head's partials, lowest chunk first.  Only the chunks that meet
// [kstart[b], pos[b]] are read (every other one holds the empty partial); the loads of a chunk do not depend on the
// chunk before it (an empty chunk inside the range -- kstart > pos -- is dropped by a select, its unwritten o never
// used), so the loop's loads overlap instead of paying one memory latency per chunk.
__global__ void attn_decode_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                           const int* __restrict__ pos, const int* __restrict__ kstart,
                                           bf16_t* __restrict__ o, int nh, int nkv, int rep, int hd, int nchunks,
                                           int S_max, int window) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int g = h / rep, r = h % rep;
  const int64_t base = (int64_t)(b * nkv + g) * nchunks * rep + r;  // + c * rep: chunk c's partial row
  const int p = pos[b];
  const int ks = max(kstart ? max(kstart[b], 0) : 0, (window > 0 && (unsigned)p < (unsigned)S_max) ? p - window + 1 : 0);  // see attn_decode_kernel
  float M = -INFINITY, L = 0.f, O = 0.f;
  if ((unsigned)p < (unsigned)S_max && ks <= p) {
    const int c_lo = ks / SPLIT, c_hi = p / SPLIT;  // c_hi < nchunks: p < S_max
#pragma unroll 4
    for (int c = c_lo; c <= c_hi; ++c) M = fmaxf(M, part_ml[(base + (int64_t)c * rep) * 2]);
#pragma unroll 4
    for (int c = c_lo; c <= c_hi; ++c) {
      const int64_t prow = base + (int64_t)c * rep;
      const float mc = part_ml[prow * 2], lc = part_ml[prow * 2 + 1];
      const float po = part_o[prow * hd + d];
      const bool live = mc != -INFINITY && lc != 0.f;
      const float f = __builtin_amdgcn_exp2f(mc - M);
      L = live ? __builtin_fmaf(lc, f, L) : L;
      O = live ? __builtin_fmaf(po, f, O) : O;
    }
  }
  o[((int64_t)b * nh + h) * hd + d] = f2bf(L > 0.f ? O / L : 0.f);  // no key at all: 0, as the training kernels
}

template <int HD>
int launch(const bf16_t* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart, bf16_t* kc,
           bf16_t* vc, float* part_o, float* part_ml, int B, int nh, int nkv, int rep, int S_max, int64_t ld,
           float scale2, int window, hipStream_t st) {
  const dim3 grid((unsigned)nkv, (unsigned)B, (unsigned)((S_max + SPLIT - 1) / SPLIT)), block(64 * DEC_WAVES);
#define ND_DECODE(R)                                                                                            \
  hipLaunchKernelGGL((attn_decode_kernel<HD, R>), grid, block, 0, st, qkv, cosT, sinT, pos, kstart, kc, vc, part_o, \
                     part_ml, nh, nkv, rep, S_max, ld, scale2, window)
  if (rep == 1) ND_DECODE(1);
  else if (rep == 2) ND_DECODE(2);
  else if (rep <= 4) ND_DECODE(4);
  else ND_DECODE(8);
#undef ND_DECODE
  return (int)hipGetLastError();
}

}  // namespace

// The compile-time chunk length of the key partition (tests aim at its edges).
ND_API int nd_attn_decode_split() { return SPLIT; }

// Workspace: part_o [B, nkv, nchunks, rep, hd] fp32, part_ml [B, nkv, nchunks, rep, 2] fp32, nchunks = ceil(S_max / SPLIT).
// `ld`: row stride of qkv in elements.  The tables must hold at least S_max rows; 0 <= pos[b] < S_max (a position
// outside writes nothing and gives o = 0).
// window: 0 = none; W >= 1 = sliding window, keys max(kstart[b], pos[b] - W + 1) .. pos[b] (nd_attn_decode_win).
static int decode_impl(const void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                       void* kcache, void* vcache, float* part_o, float* part_ml, void* o, int B, int nh, int nkv,
                       int hd, int S_max, int64_t ld, float scale, int window, hipStream_t st) {
  if (B < 1 || B > 65535 || nh < 1 || nkv < 1 || nkv > 65535 || nh % nkv || nh / nkv > 8 || S_max < 1 ||
      (S_max + SPLIT - 1) / SPLIT > 65535)
    return (int)hipErrorInvalidValue;
  if (hd != 32 && hd != 64 && hd != 128) return (int)hipErrorInvalidValue;
  if (ld < (int64_t)(nh + 2 * nkv) * hd || ld % 8) return (int)hipErrorInvalidValue;
  if (!qkv || !cosT || !sinT || !pos || !kcache || !vcache || !part_o || !part_ml || !o)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)cosT | (uintptr_t)sinT | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)part_o |
       (uintptr_t)part_ml) & 15)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)o & 1) || ((uintptr_t)pos & 3) || ((uintptr_t)kstart & 3)) return (int)hipErrorInvalidValue;
  const int rep = nh / nkv;
  const float scale2 = scale * LOG2E;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(qkv);
  bf16_t* kc = reinterpret_cast<bf16_t*>(kcache);
  bf16_t* vc = reinterpret_cast<bf16_t*>(vcache);
  int err;
  if (hd == 32) err = launch<32>(x, cosT, sinT, pos, kstart, kc, vc, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  else if (hd == 64) err = launch<64>(x, cosT, sinT, pos, kstart, kc, vc, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  else err = launch<128>(x, cosT, sinT, pos, kstart, kc, vc, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  if (err) return err;
  const int nchunks = (S_max + SPLIT - 1) / SPLIT;
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)nh, (unsigned)B), dim3((unsigned)hd), 0, st, part_o,
                     part_ml, pos, kstart, reinterpret_cast<bf16_t*>(o), nh, nkv, rep, hd, nchunks, S_max, window);
  ND_LAUNCH_CHECK();
}

ND_API int nd_attn_decode(const void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                          void* kcache, void* vcache, float* part_o, float* part_ml, void* o, int B, int nh, int nkv,
                          int hd, int S_max, int64_t ld, float scale, hipStream_t st) {
  return decode_impl(qkv, cosT, sinT, pos, kstart, kcache, vcache, part_o, part_ml, o, B, nh, nkv, hd, S_max, ld, scale,
                     0, st);
}

// Sliding-window decode step: as nd_attn_decode over keys max(kstart[b], pos[b] - window + 1, 0) .. pos[b], window >= 1.
// Chunks wholly below that bound write the empty partial and leave; the combine reads only the chunks that meet the
// range, so a step reads O(window) keys.  The append to slot pos[b] and the key-indexed partition are unchanged: the
// result is bitwise nd_attn_decode's with kstart' = max(kstart, pos - window + 1).
ND_API int nd_attn_decode_win(const void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                              void* kcache, void* vcache, float* part_o, float* part_ml, void* o, int B, int nh,
                              int nkv, int hd, int S_max, int64_t ld, float scale, int window, hipStream_t st) {
  if (window < 1) return (int)hipErrorInvalidValue;
  return decode_impl(qkv, cosT, sinT, pos, kstart, kcache, vcache, part_o, part_ml, o, B, nh, nkv, hd, S_max, ld, scale,
                     window, st);
}
