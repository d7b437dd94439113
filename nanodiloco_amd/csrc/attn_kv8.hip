// fp8 (e4m3) KV cache: the decode step, the multi-token step and the prefill fill on 8-bit K/V rows
// (docs/DESIGN.md "fp8 KV cache").
//
// Format.  Each K row (after RoPE) and each V row of one (sequence, kv head, slot) is hd OCP e4m3 codes plus one int8
// exponent e; the value is code * 2^e.  For a row x (bf16 values as fp32) with amax = max |x|: e = 0 if amax == 0,
// else the smallest e with amax * 2^-e <= 448, clamped to [-100, 100] and taken from the float's bits (kv8_exp);
// code = e4m3(x * 2^-e), round-to-nearest-even, saturating.  Both scalings are by powers of two, hence exact: the
// codes are a pure function of the row, and code * 2^e is exact in fp32 and in bf16 (4 significant bits, the clamp
// keeps it normal), so the attention below runs on exact operands.  Outside the contract: a row with +-inf gets
// e = 100, the infinities saturate to +-448 and its small values flush to +-0; a NaN gives the NaN code 0x7f / 0xff
// and does not enter the amax.
// Storage per layer: codes uint8 [B, nkv, S_max, hd] and exponents int8 [B, nkv, S_max], for K and for V.
//
//   nd_attn_decode_kv8   attn_decode.hip's step -- RoPE of the new row, append, split-KV attention over keys
//                        max(kstart, pos - window + 1) .. pos, combine -- with the same key partition (SPLIT keys per
//                        workgroup by absolute index), the same partials and that file's combine kernel: one launch
//                        shape per step, no atomics, a sequence's bits independent of batch and occupancy.  A K/V row
//                        is hd/8 lanes x 8 B (one dwordx2 load per lane and 64 / (hd/8) rows per wave-wide load,
//                        straight into VGPRs) plus its exponent byte; codes become fp32 by v_cvt_pk_f32_fp8.  K's 2^e
//                        is folded into the score after the lane reduction (one multiply, together with scale
//                        log2(e)), V's into p before the P V fma -- both exact, so the arithmetic is the bf16 kernel's
//                        on the dequantised rows.  The new token's k and v are quantised in registers, written as
//                        codes + exponent, and enter this step's attention as those codes: key pos looks the same to
//                        this step as to every later one.
//   nd_attn_extend_kv8   attn_extend.hip's three launches.  The append rotates q and k in place and quantises the
//                        rotated k rows and the v rows into slots pos .. pos+L-1 (a head row is shared by hd/16
//                        neighbouring threads: the amax is a shuffle reduction over them).  The attention is that
//                        file's MFMA kernel with the staging below: codes and exponents are loaded for the live slots
//                        only, converted to the exact bf16 value and written to the same swizzled tiles, so the MFMA,
//                        mask, softmax and combine code -- and the file's invariance statement -- are unchanged.
//   nd_kv8_fill          prefill: the k|v columns of the training path's packed, already rotated q|k|v buffer
//                        [B*T, W] into slots 0 .. T-1, quantised (the fp8 counterpart of cache_fill's strided copy).
// All three quantise with kv8_exp / kv8_codes8 below.  Attention soft-capping is not carried by these kernels.
#define ND_DECODE_KERNELS_ONLY 1
#define ND_EXTEND_KERNELS_ONLY 1
#include "attn_decode.hip"
#include "attn_extend.hip"

namespace {

// ---------------------------------------------------------------------------------------------- the quantiser
// amax >= 0 (not NaN) -> the row's exponent.  amax = (1 + M / 2^23) 2^(E - 127) = f 2^k with f in [0.5, 1), k = E - 126:
// e = k - 9 if f <= 0.875 (M <= 0x600000), else k - 8.  A denormal amax (E = 0) falls below the clamp either way.
__device__ __forceinline__ int kv8_exp(float amax) {
  const uint32_t u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return u == 0 ? 0 : min(max(e, -100), 100);
}
// 2^e as fp32, e in [-126, 127]
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
// 8 values x a power of two -> 8 codes (cvt4: saturating, RNE, NaN kept)
__device__ __forceinline__ uint2 kv8_codes8(const float* x, float inv) {
  uint2 o;
  o.x = cvt4<0>(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
  o.y = cvt4<0>(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv);
  return o;
}
__device__ __forceinline__ float amax8(const float* x) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(x[j]));
  return a;
}
// 8 codes -> fp32 (v_cvt_pk_f32_fp8, two codes each)
__device__ __forceinline__ void kv8_unpack8(uint2 c, float* v) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
  const f32x2_t d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = d.x; v[5] = d.y; v[6] = e.x; v[7] = e.y;
}

// ---------------------------------------------------------------------------------------------- decode
// attn_decode_kernel (see there for the partition, the softmax and the wave merge) on an fp8 cache.
template <int HD, int REP>
__global__ void __launch_bounds__(64 * DEC_WAVES)
attn_decode_kv8_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ cosT, const float* __restrict__ sinT,
                       const int* __restrict__ pos, const int* __restrict__ kstart, uint8_t* __restrict__ kcache,
                       int8_t* __restrict__ kexp, uint8_t* __restrict__ vcache, int8_t* __restrict__ vexp,
                       float* __restrict__ part_o, float* __restrict__ part_ml, int nh, int nkv, int rep, int S_max,
                       int64_t ld, float scale2, int window) {
  constexpr int LPR = HD / 8;       // lanes per K/V row, 8 codes = 8 B each
  constexpr int KPI = 64 / LPR;     // rows per wave-wide load
  constexpr int ITER = KPW / KPI;   // loads per lane for the wave's keys
  static_assert(KPW % KPI == 0, "a wave's key slice must be whole loads");
  __shared__ float sm_m[DEC_WAVES][REP], sm_l[DEC_WAVES][REP];
  __shared__ float sm_o[DEC_WAVES][REP][HD];

  const int g = blockIdx.x, b = blockIdx.y, c = blockIdx.z;  // the chunk slowest: see attn_decode_kernel
  const int nchunks = gridDim.z;
  const int p = pos[b];
  const int ks = max(kstart ? max(kstart[b], 0) : 0, (window > 0 && (unsigned)p < (unsigned)S_max) ? p - window + 1 : 0);
  const int64_t pbase = ((int64_t)(b * nkv + g) * nchunks + c) * rep;
  const int c0 = c * SPLIT;
  const bool holds_p = c0 <= p && p < c0 + SPLIT;
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
  const int dp = second ? d0 - HALF : d0 + HALF;
  const int i0 = second ? d0 - HALF : d0;

  // ---- the new token: rotate k, take v, quantise both in registers (the row's amax over its LPR lanes)
  const bf16_t* row = qkv + (int64_t)b * ld;
  float cc[8], ss[8];
  {
    const float4* cp = reinterpret_cast<const float4*>(cosT + (int64_t)p * HD + i0);
    const float4* sp = reinterpret_cast<const float4*>(sinT + (int64_t)p * HD + i0);
    const float4 c0v = cp[0], c1v = cp[1], s0v = sp[0], s1v = sp[1];
    cc[0] = c0v.x; cc[1] = c0v.y; cc[2] = c0v.z; cc[3] = c0v.w; cc[4] = c1v.x; cc[5] = c1v.y; cc[6] = c1v.z; cc[7] = c1v.w;
    ss[0] = s0v.x; ss[1] = s0v.y; ss[2] = s0v.z; ss[3] = s0v.w; ss[4] = s1v.x; ss[5] = s1v.y; ss[6] = s1v.z; ss[7] = s1v.w;
  }
  uint2 knew, vnew;
  int kenew, venew;
  {
    const bf16_t* kin = row + (int64_t)(nh + g) * HD;
    const bf16_t* vin = row + (int64_t)(nh + nkv + g) * HD;
    float kf[8], vf[8];
    unpack8(rope8(*reinterpret_cast<const uint4*>(kin + d0), *reinterpret_cast<const uint4*>(kin + dp), cc, ss, second), kf);
    unpack8(*reinterpret_cast<const uint4*>(vin + d0), vf);
    float ka = amax8(kf), va = amax8(vf);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
      ka = fmaxf(ka, __shfl_xor(ka, o, 64));
      va = fmaxf(va, __shfl_xor(va, o, 64));
    }
    kenew = kv8_exp(ka);
    venew = kv8_exp(va);
    knew = kv8_codes8(kf, pow2i(-kenew));
    vnew = kv8_codes8(vf, pow2i(-venew));
  }
  const int64_t row0 = (int64_t)(b * nkv + g) * S_max;
  uint8_t* kc = kcache + row0 * HD;
  uint8_t* vc = vcache + row0 * HD;
  if (holds_p && threadIdx.x < LPR) {  // append
    *reinterpret_cast<uint2*>(kc + (int64_t)p * HD + d0) = knew;
    *reinterpret_cast<uint2*>(vc + (int64_t)p * HD + d0) = vnew;
    if (dg == 0) {
      kexp[row0 + p] = (int8_t)kenew;
      vexp[row0 + p] = (int8_t)venew;
    }
  }

  // ---- this wave's K and V rows and exponents, all loads in flight before the first use
  const int kbase = c0 + w * KPW + ksub;
  uint2 kraw[ITER], vraw[ITER];
  int kex[ITER], vex[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int key = kbase + it * KPI;
    kraw[it] = make_uint2(0, 0);
    vraw[it] = make_uint2(0, 0);
    kex[it] = 0;
    vex[it] = 0;
    if (key >= ks && key < p) {  // key < p <= S_max - 1: inside the cache
      kraw[it] = *reinterpret_cast<const uint2*>(kc + (int64_t)key * HD + d0);
      vraw[it] = *reinterpret_cast<const uint2*>(vc + (int64_t)key * HD + d0);
      kex[it] = kexp[row0 + key];
      vex[it] = vexp[row0 + key];
    } else if (key == p) {
      kraw[it] = knew;
      vraw[it] = vnew;
      kex[it] = kenew;
      vex[it] = venew;
    }
  }

  float q[REP][8];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const bf16_t* qin = row + (int64_t)(g * rep + min(r, rep - 1)) * HD;
    unpack8(rope8(*reinterpret_cast<const uint4*>(qin + d0), *reinterpret_cast<const uint4*>(qin + dp), cc, ss, second),
            q[r]);
  }

  // ---- scores (log2 domain), -inf outside [ks, p]: the dot product on the codes, then one multiply by scale2 2^e
  float s[REP][ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int key = kbase + it * KPI;
    const bool valid = key >= ks && key <= p;
    const float ksc = scale2 * pow2i(kex[it]);
    float kf[8];
    kv8_unpack8(kraw[it], kf);
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(q[r][j], kf[j], acc);
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      s[r][it] = valid ? acc * ksc : -INFINITY;
    }
  }

  // ---- the wave's softmax (exact two-pass over its KPW keys) and P V, V's 2^e folded into p
  float m[REP], l[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    float mx = s[r][0];
#pragma unroll
    for (int it = 1; it < ITER; ++it) mx = fmaxf(mx, s[r][it]);
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    m[r] = mx;
    const float ms = mx == -INFINITY ? 0.f : mx;
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
    kv8_unpack8(vraw[it], vf);
    const float vsc = pow2i(vex[it]);
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      const float pv = s[r][it] * vsc;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(pv, vf[j], acc[r][j]);
    }
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

template <int HD>
int launch_kv8(const bf16_t* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart, uint8_t* kc,
               int8_t* ke, uint8_t* vc, int8_t* ve, float* part_o, float* part_ml, int B, int nh, int nkv, int rep,
               int S_max, int64_t ld, float scale2, int window, hipStream_t st) {
  const dim3 grid((unsigned)nkv, (unsigned)B, (unsigned)((S_max + SPLIT - 1) / SPLIT)), block(64 * DEC_WAVES);
#define ND_DECODE_KV8(R)                                                                                          \
  hipLaunchKernelGGL((attn_decode_kv8_kernel<HD, R>), grid, block, 0, st, qkv, cosT, sinT, pos, kstart, kc, ke, vc, ve, \
                     part_o, part_ml, nh, nkv, rep, S_max, ld, scale2, window)
  if (rep == 1) ND_DECODE_KV8(1);
  else if (rep == 2) ND_DECODE_KV8(2);
  else if (rep <= 4) ND_DECODE_KV8(4);
  else ND_DECODE_KV8(8);
#undef ND_DECODE_KV8
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- extend
// attn_extend_append on an fp8 cache.  One thread per (row, head, 8 pairs); the hd/16 threads of a head row are
// neighbours in a wave (an aligned group: they leave or stay together), so the row's amax is a shuffle reduction.
__global__ void __launch_bounds__(256)
attn_extend_append_kv8(bf16_t* __restrict__ qkv, const float* __restrict__ cosT, const float* __restrict__ sinT,
                       const int* __restrict__ pos, uint8_t* __restrict__ kcache, int8_t* __restrict__ kexp,
                       uint8_t* __restrict__ vcache, int8_t* __restrict__ vexp, int B, int L, int nh, int nkv, int hd,
                       int S_max, int64_t ld) {
  const int half = hd >> 1, gpr = half >> 3, heads = nh + 2 * nkv;  // gpr: threads per head row
  const int64_t total = (int64_t)B * L * heads * gpr;
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= total) return;
  const int d0 = (int)(it % gpr) * 8;
  const int64_t rh = it / gpr;
  const int head = (int)(rh % heads);
  const int64_t row = rh / heads;  // b * L + i
  const int b = (int)(row / L), i = (int)(row % L);
  const int p = pos[b];
  if (bad_pos(p, L, S_max)) return;
  const int slot = p + i;  // < S_max
  bf16_t* src = qkv + row * ld + (int64_t)head * hd + d0;
  uint4 x = *reinterpret_cast<const uint4*>(src), y = *reinterpret_cast<const uint4*>(src + half);
  if (head < nh + nkv) {
    float cc[8], ss[8];
    const float4* cp = reinterpret_cast<const float4*>(cosT + (int64_t)slot * hd + d0);
    const float4* sp = reinterpret_cast<const float4*>(sinT + (int64_t)slot * hd + d0);
    const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
    cc[0] = c0.x; cc[1] = c0.y; cc[2] = c0.z; cc[3] = c0.w; cc[4] = c1.x; cc[5] = c1.y; cc[6] = c1.z; cc[7] = c1.w;
    ss[0] = s0.x; ss[1] = s0.y; ss[2] = s0.z; ss[3] = s0.w; ss[4] = s1.x; ss[5] = s1.y; ss[6] = s1.z; ss[7] = s1.w;
    rope_pair8(x, y, cc, ss);
    *reinterpret_cast<uint4*>(src) = x;
    *reinterpret_cast<uint4*>(src + half) = y;
  }
  if (head >= nh) {  // uniform over the row's threads
    const bool isv = head >= nh + nkv;
    const int g = head - nh - (isv ? nkv : 0);
    float xf[8], yf[8];
    unpack8(x, xf);
    unpack8(y, yf);
    float a = fmaxf(amax8(xf), amax8(yf));
    for (int o = gpr >> 1; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    const int e = kv8_exp(a);
    const float inv = pow2i(-e);
    const int64_t r = (int64_t)(b * nkv + g) * S_max + slot;
    uint8_t* dst = (isv ? vcache : kcache) + r * hd + d0;
    *reinterpret_cast<uint2*>(dst) = kv8_codes8(xf, inv);
    *reinterpret_cast<uint2*>(dst + half) = kv8_codes8(yf, inv);
    if (d0 == 0) (isv ? vexp : kexp)[r] = (int8_t)e;
  }
}

// One thread per (row of the packed buffer, k or v head, 16 columns): two 16-B loads, one 16-B store of codes.
__global__ void __launch_bounds__(256)
kv8_fill_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kcache, int8_t* __restrict__ kexp,
                uint8_t* __restrict__ vcache, int8_t* __restrict__ vexp, int B, int T, int nh, int nkv, int hd, int S_max,
                int64_t ld) {
  const int tpr = hd >> 4;  // threads per head row: an aligned group of neighbours, as above
  const int64_t total = (int64_t)B * T * 2 * nkv * tpr;
  const int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= total) return;
  const int d0 = (int)(it % tpr) * 16;
  const int64_t rh = it / tpr;
  const int head = (int)(rh % (2 * nkv));  // k heads, then v heads: the buffer's column order
  const int64_t row = rh / (2 * nkv);      // b * T + t
  const int b = (int)(row / T), t = (int)(row % T);
  const bf16_t* src = qkv + row * ld + (int64_t)(nh + head) * hd + d0;
  float xf[8], yf[8];
  unpack8(*reinterpret_cast<const uint4*>(src), xf);
  unpack8(*reinterpret_cast<const uint4*>(src + 8), yf);
  float a = fmaxf(amax8(xf), amax8(yf));
  for (int o = tpr >> 1; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  const int e = kv8_exp(a);
  const float inv = pow2i(-e);
  const bool isv = head >= nkv;
  const int64_t r = (int64_t)(b * nkv + (isv ? head - nkv : head)) * S_max + t;
  const uint2 lo = kv8_codes8(xf, inv), hi = kv8_codes8(yf, inv);
  *reinterpret_cast<uint4*>((isv ? vcache : kcache) + r * hd + d0) = make_uint4(lo.x, lo.y, hi.x, hi.y);
  if (d0 == 0) (isv ? vexp : kexp)[r] = (int8_t)e;
}

// attn_extend_kernel's staging for an fp8 operand: 8 codes (8 B) and the key's exponent per piece, converted to the
// exact bf16 value code * 2^e (fp32 product, then a rounding that changes nothing) -- the same 16-B pieces in the
// same swizzled places as the bf16 staging.  Slots outside [glo, ghi] are not read, neither codes nor exponents.
template <int HD>
__device__ __forceinline__ void stage_chunk(Kv8 kcache, Kv8 vcache, bf16_t* Ks, bf16_t* Vs, int64_t row0, int c0,
                                            int glo, int ghi) {
  constexpr int CPR = HD / 8;
  constexpr int NST = SPLIT * CPR / (64 * XW);
  uint2 kr[NST], vr[NST];
  int ke[NST], ve[NST];
#pragma unroll
  for (int it = 0; it < NST; ++it) {
    const int idx = threadIdx.x + it * (64 * XW);
    const int key = c0 + idx / CPR, ch = idx % CPR;
    kr[it] = make_uint2(0, 0);
    vr[it] = make_uint2(0, 0);
    ke[it] = 0;
    ve[it] = 0;
    if (key >= glo && key <= ghi) {
      kr[it] = *reinterpret_cast<const uint2*>(kcache.codes + (row0 + key) * HD + ch * 8);
      vr[it] = *reinterpret_cast<const uint2*>(vcache.codes + (row0 + key) * HD + ch * 8);
      ke[it] = kcache.exps[row0 + key];
      ve[it] = vcache.exps[row0 + key];
    }
  }
#pragma unroll
  for (int it = 0; it < NST; ++it) {
    const int idx = threadIdx.x + it * (64 * XW);
    const int o = soff<HD>(idx / CPR, (idx % CPR) * 8);
    float kf[8], vf[8];
    kv8_unpack8(kr[it], kf);
    kv8_unpack8(vr[it], vf);
    const float ksc = pow2i(ke[it]), vsc = pow2i(ve[it]);
    *reinterpret_cast<uint4*>(&Ks[o]) = make_uint4(pack2(kf[0] * ksc, kf[1] * ksc), pack2(kf[2] * ksc, kf[3] * ksc),
                                                   pack2(kf[4] * ksc, kf[5] * ksc), pack2(kf[6] * ksc, kf[7] * ksc));
    *reinterpret_cast<uint4*>(&Vs[o]) = make_uint4(pack2(vf[0] * vsc, vf[1] * vsc), pack2(vf[2] * vsc, vf[3] * vsc),
                                                   pack2(vf[4] * vsc, vf[5] * vsc), pack2(vf[6] * vsc, vf[7] * vsc));
  }
}

// what every entry below checks of its shapes and pointers (the caches: codes 16-byte aligned, exponents any)
bool kv8_args_ok(int B, int nh, int nkv, int hd, int S_max, const void* kc, const void* ke, const void* vc,
                 const void* ve) {
  if (B < 1 || B > 65535 || nh < 1 || nkv < 1 || nkv > 65535 || nh % nkv || nh / nkv > 8 || S_max < 1 ||
      (S_max + SPLIT - 1) / SPLIT > 65535)
    return false;
  if (hd != 32 && hd != 64 && hd != 128) return false;
  if (!kc || !ke || !vc || !ve) return false;
  return !(((uintptr_t)kc | (uintptr_t)vc) & 15);
}

}  // namespace

// nd_attn_decode / _win on an fp8 cache: kcache / vcache uint8 [B, nkv, S_max, hd], kexp / vexp int8 [B, nkv, S_max].
// Workspace, `ld`, the tables and pos as there.  window: 0 = none, W >= 1 = sliding window.
ND_API int nd_attn_decode_kv8(const void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                              void* kcache, void* kexp, void* vcache, void* vexp, float* part_o, float* part_ml,
                              void* o, int B, int nh, int nkv, int hd, int S_max, int64_t ld, float scale, int window,
                              hipStream_t st) {
  if (!kv8_args_ok(B, nh, nkv, hd, S_max, kcache, kexp, vcache, vexp) || window < 0) return (int)hipErrorInvalidValue;
  if (ld < (int64_t)(nh + 2 * nkv) * hd || ld % 8) return (int)hipErrorInvalidValue;
  if (!qkv || !cosT || !sinT || !pos || !part_o || !part_ml || !o) return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)cosT | (uintptr_t)sinT | (uintptr_t)part_o | (uintptr_t)part_ml) & 15)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)o & 1) || ((uintptr_t)pos & 3) || ((uintptr_t)kstart & 3)) return (int)hipErrorInvalidValue;
  const int rep = nh / nkv;
  const float scale2 = scale * LOG2E;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(qkv);
  uint8_t* kc = reinterpret_cast<uint8_t*>(kcache);
  uint8_t* vc = reinterpret_cast<uint8_t*>(vcache);
  int8_t* ke = reinterpret_cast<int8_t*>(kexp);
  int8_t* ve = reinterpret_cast<int8_t*>(vexp);
  int err;
  if (hd == 32) err = launch_kv8<32>(x, cosT, sinT, pos, kstart, kc, ke, vc, ve, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  else if (hd == 64) err = launch_kv8<64>(x, cosT, sinT, pos, kstart, kc, ke, vc, ve, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  else err = launch_kv8<128>(x, cosT, sinT, pos, kstart, kc, ke, vc, ve, part_o, part_ml, B, nh, nkv, rep, S_max, ld, scale2, window, st);
  if (err) return err;
  const int nchunks = (S_max + SPLIT - 1) / SPLIT;
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)nh, (unsigned)B), dim3((unsigned)hd), 0, st, part_o,
                     part_ml, pos, kstart, reinterpret_cast<bf16_t*>(o), nh, nkv, rep, hd, nchunks, S_max, window);
  ND_LAUNCH_CHECK();
}

// nd_attn_extend on an fp8 cache (no soft-cap); workspace and the rest as there.
ND_API int nd_attn_extend_kv8(void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                              void* kcache, void* kexp, void* vcache, void* vexp, float* part_o, float* part_ml,
                              void* o, int B, int L, int nh, int nkv, int hd, int S_max, int64_t ld, float scale,
                              int window, hipStream_t st) {
  if (!kv8_args_ok(B, nh, nkv, hd, S_max, kcache, kexp, vcache, vexp) || window < 0) return (int)hipErrorInvalidValue;
  if (L < 1 || L > S_max || (int64_t)B * L > 0x7fffffff) return (int)hipErrorInvalidValue;
  if (ld < (int64_t)(nh + 2 * nkv) * hd || ld % 8) return (int)hipErrorInvalidValue;
  if (!qkv || !cosT || !sinT || !pos || !part_o || !part_ml || !o) return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)cosT | (uintptr_t)sinT | (uintptr_t)part_o | (uintptr_t)part_ml) & 15)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)o & 1) || ((uintptr_t)pos & 3) || ((uintptr_t)kstart & 3)) return (int)hipErrorInvalidValue;
  bf16_t* x = reinterpret_cast<bf16_t*>(qkv);
  uint8_t* kc = reinterpret_cast<uint8_t*>(kcache);
  uint8_t* vc = reinterpret_cast<uint8_t*>(vcache);
  int8_t* ke = reinterpret_cast<int8_t*>(kexp);
  int8_t* ve = reinterpret_cast<int8_t*>(vexp);
  const int64_t items = (int64_t)B * L * (nh + 2 * nkv) * (hd / 16);
  if ((items + 255) / 256 > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_extend_append_kv8, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, cosT, sinT, pos,
                     kc, ke, vc, ve, B, L, nh, nkv, hd, S_max, ld);
  const int err = (int)hipGetLastError();
  if (err) return err;
  return extend_blocks(x, pos, kstart, Kv8{kc, ke}, Kv8{vc, ve}, part_o, part_ml, reinterpret_cast<bf16_t*>(o), B, L, nh,
                       nkv, hd, S_max, ld, scale * LOG2E, window, st);
}

// Prefill: the k|v columns of the packed, already rotated q|k|v buffer [B*T, >= (nh + 2 nkv) hd] (row stride `ld`)
// quantised into slots 0 .. T-1 of the caches.
ND_API int nd_kv8_fill(const void* qkv, void* kcache, void* kexp, void* vcache, void* vexp, int B, int T, int nh,
                       int nkv, int hd, int S_max, int64_t ld, hipStream_t st) {
  if (!kv8_args_ok(B, nh, nkv, hd, S_max, kcache, kexp, vcache, vexp)) return (int)hipErrorInvalidValue;
  if (T < 1 || T > S_max || !qkv || ((uintptr_t)qkv & 15) || ld < (int64_t)(nh + 2 * nkv) * hd || ld % 8)
    return (int)hipErrorInvalidValue;
  const int64_t items = (int64_t)B * T * 2 * nkv * (hd / 16);
  if ((items + 255) / 256 > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv8_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const bf16_t*>(qkv), reinterpret_cast<uint8_t*>(kcache),
                     reinterpret_cast<int8_t*>(kexp), reinterpret_cast<uint8_t*>(vcache), reinterpret_cast<int8_t*>(vexp),
                     B, T, nh, nkv, hd, S_max, ld);
  ND_LAUNCH_CHECK();
}
