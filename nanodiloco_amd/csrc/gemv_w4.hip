// fp4 weight-only projection for the decode step (docs/DESIGN.md "fp4 weight-only decode"):
//
//   out[M, N] (bf16) = x[M, K] (bf16) . dequant(codes, exps)^T,   1 <= M <= MAX_M = 16, fp32 accumulation (W4A16).
//
// Format (ops.gemv.quantize_weight_fp4, the OCP MX block layout).  W [N, K] is cut into groups of 32 along K: codes
// uint8 [N, K / 2], element k in the low (k even) or high (k odd) nibble of byte k / 2, a nibble = sign bit + 3 bits
// indexing {0, 0.5, 1, 1.5, 2, 3, 4, 6} (e2m1); exps int8 [N, K / 32]; value = code * 2^e.
//
// The code bytes are what the kernel streams; it is laid out around them:
//   * Work split.  A workgroup (4 waves) owns one tile of 16 output channels and one K slice of `spb` steps of 128 k;
//     the partition (spb, splits) is a pure function of (N, K) (w4_partition: one slice up to K = 8192).  Wave w takes
//     steps lo + w, lo + w + 4, ... of the slice, INFLIGHT of them at a time: all their loads are issued before the
//     first use.
//   * Data path.  Lane (c = lane & 15, q = lane >> 4) loads 16 code bytes of channel n0 + c at k = 128 t + 32 q --
//     exactly one scale group -- and that group's exponent byte; the four lanes of a channel cover 64 contiguous
//     bytes, every code byte is read once, straight into VGPRs.  v_cvt_scalef32_pk_bf16_fp4 turns one code byte and
//     the scale 2^e (ldexpf(1, e): no float built from bits) into two bf16 values that already carry the exponent,
//     exactly (6 * 2^100 and 0.5 * 2^-100 are normal bf16 numbers): 16 conversions give the B operands (k x 16
//     channels) of four v_mfma_f32_16x16x32_bf16, MFMA j taking k = 128 t + 32 q + 8 j .. + 8.  The A operand (16 rows
//     of x, rows >= M zero) is 8 bf16 of x at the SAME k (the MFMA's k order is free as long as both operands
//     agree), loaded from global memory -- x is at most 16 x K bf16 and stays in L2 -- into registers; no LDS staging.
//   * Scales.  None after the conversion: the four MFMAs of a step accumulate straight into the wave's accumulator.
//   * Combine, fixed order, no atomics.  The four waves' accumulators meet in LDS and are added in wave order.  With
//     one K slice that sum is rounded to bf16 and stored; otherwise it goes to the fp32 workspace
//     [splits, MAX_M, N] and gemv_w4_combine adds the slices in slice order.
//   * Invariance.  An output row is a set of MFMA rows: its bits depend on that row of x, the weight, N and K (the
//     partition) -- not on M, the row's index, the other rows or the run.
//   * Edges.  Channels >= N and rows >= M are neither loaded nor stored (zero operands; every fp4 value is finite, so
//     a zero row of x gives zeros); K = 128 is one step on wave 0.
#include "common.h"

using namespace nd;

namespace {

constexpr int MAX_M = 16;        // rows of x: the MFMA's M (nd_gemv_w8_max_m serves both kernels)
constexpr int STEP = 128;        // k per wave step: four scale groups of 32, one per lane quarter
constexpr int GROUP = 32;        // codes per exponent
constexpr int TILE_N = 16;       // output channels per workgroup: the MFMA's N
constexpr int W4_WAVES = 4;      // waves per workgroup, splitting the K slice
constexpr int INFLIGHT = 4;      // steps a wave loads before it computes (2: 0.3-0.5 us slower at K = 2048)
constexpr int TARGET_WGS = 512;  // two workgroups per CU, once K is split at all
constexpr int MIN_SPB = 64;      // steps of the shortest K slice: K <= 8192 is never split

typedef __bf16 bfv8 __attribute__((ext_vector_type(8)));

struct W4Part {
  int spb, splits;  // steps per workgroup, K slices
};
// The K partition: a pure function of (N, K).  Measured (profiles/w4_gemv.md "Partition"): a second K slice means a
// second launch (gemv_w4_combine), about 2 us in a captured graph, more than the extra workgroups win back at any
// projection shape of configs/ -- with 0.5 byte per weight a 64-step slice is 4 KB per wave.  So a slice is never
// shorter than MIN_SPB steps, and only a longer K is cut towards TARGET_WGS workgroups.
inline W4Part w4_partition(int N, int K) {
  const int S = K / STEP, tiles = (N + TILE_N - 1) / TILE_N;
  const int want = (TARGET_WGS + tiles - 1) / tiles;
  int spb = (S + want - 1) / want;
  if (spb < MIN_SPB) spb = MIN_SPB;
  return {spb, (S + spb - 1) / spb};
}

// 8 e2m1 codes (one dword, element i in nibble i) times `scale` -> 8 bf16, exact
__device__ __forceinline__ bfv8 codes8_bf16(uint32_t d, float scale) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  const bf16x2_t e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  return bfv8{a.x, a.y, b.x, b.y, c.x, c.y, e.x, e.y};
}
__device__ __forceinline__ f32x4 mma(const uint4& a, const bfv8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfv8, a), b, c, 0, 0, 0);
}

__global__ void __launch_bounds__(64 * W4_WAVES)
gemv_w4_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ codes, const int8_t* __restrict__ exps,
               bf16_t* __restrict__ out, float* __restrict__ ws, int M, int N, int K, int64_t ldx, int spb, int splits) {
  __shared__ float red[W4_WAVES][TILE_N * MAX_M];
  const int n0 = blockIdx.x * TILE_N, s = blockIdx.y;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int S = K / STEP;
  const int t_lo = s * spb, t_hi = min(S, t_lo + spb);
  // the lane's channel (B operand and accumulator column) and its row of x (A operand): c in both roles
  const bool wlive = n0 + c < N, xlive = c < M;
  const uint8_t* wrow = codes + (int64_t)(wlive ? n0 + c : 0) * (K / 2) + q * 16;
  const int8_t* erow = exps + (int64_t)(wlive ? n0 + c : 0) * (K / GROUP) + q;
  const bf16_t* xrow = x + (int64_t)(xlive ? c : 0) * ldx + q * 32;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = t_lo + w; t < t_hi; t += W4_WAVES * INFLIGHT) {
    uint4 wv[INFLIGHT], xv[INFLIGHT][4];
    int e[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      const int tt = t + u * W4_WAVES;
      const bool live = tt < t_hi;  // wave-uniform
      e[u] = 0;
      wv[u] = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[u][j] = make_uint4(0, 0, 0, 0);
      if (live && wlive) {
        wv[u] = *reinterpret_cast<const uint4*>(wrow + (int64_t)tt * (STEP / 2));
        e[u] = erow[(int64_t)tt * (STEP / GROUP)];
      }
      if (live && xlive) {
        const uint4* xp = reinterpret_cast<const uint4*>(xrow + (int64_t)tt * STEP);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[u][j] = xp[j];
      }
    }
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      if (t + u * W4_WAVES < t_hi) {
        const float scale = ldexpf(1.f, e[u]);
        acc = mma(xv[u][0], codes8_bf16(wv[u].x, scale), acc);
        acc = mma(xv[u][1], codes8_bf16(wv[u].y, scale), acc);
        acc = mma(xv[u][2], codes8_bf16(wv[u].z, scale), acc);
        acc = mma(xv[u][3], codes8_bf16(wv[u].w, scale), acc);
      }
    }
  }

  // accumulator register r of lane (c, q) is out[m = 4 q + r][n0 + c]
#pragma unroll
  for (int r = 0; r < 4; ++r) red[w][(4 * q + r) * TILE_N + c] = acc[r];
  __syncthreads();
  const int m = threadIdx.x >> 4, n = n0 + (threadIdx.x & 15);
  float v = red[0][threadIdx.x];
#pragma unroll
  for (int i = 1; i < W4_WAVES; ++i) v += red[i][threadIdx.x];
  if (m < M && n < N) {
    if (splits == 1) out[(int64_t)m * N + n] = f2bf(v);
    else ws[((int64_t)s * MAX_M + m) * N + n] = v;
  }
}

// out[m][n] = bf16(sum over the K slices, in slice order)
__global__ void __launch_bounds__(256)
gemv_w4_combine(const float* __restrict__ ws, bf16_t* __restrict__ out, int M, int N, int splits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float v = ws[(int64_t)m * N + n];
  for (int s = 1; s < splits; ++s) v += ws[((int64_t)s * MAX_M + m) * N + n];
  out[i] = f2bf(v);
}

bool w4_shape_ok(int N, int K) {
  return N >= 1 && N <= 0x7fffffff - TILE_N && K >= STEP && K % STEP == 0;
}

}  // namespace

// K slices of the (N, K) partition: > 1 means nd_gemv_w4 needs a workspace of splits * MAX_M * N floats.  0: bad shape.
ND_API int nd_gemv_w4_splits(int N, int K) { return w4_shape_ok(N, K) ? w4_partition(N, K).splits : 0; }

// x [M, K] bf16 (row stride ldx elements, a multiple of 8), codes uint8 [N, K / 2], exps int8 [N, K / 32], out bf16
// [M, N] contiguous, ws fp32 [splits, MAX_M, N] (may be null when nd_gemv_w4_splits(N, K) == 1).  x, codes and ws
// 16-byte aligned.
ND_API int nd_gemv_w4(const void* x, const void* codes, const void* exps, void* out, float* ws, int M, int N, int K,
                      int64_t ldx, hipStream_t st) {
  if (M < 1 || M > MAX_M || !w4_shape_ok(N, K) || ldx < K || ldx % 8) return (int)hipErrorInvalidValue;
  if (!x || !codes || !exps || !out) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)x | (uintptr_t)codes | (uintptr_t)ws) & 15) || ((uintptr_t)out & 1)) return (int)hipErrorInvalidValue;
  const W4Part p = w4_partition(N, K);
  if (p.splits > 65535 || (p.splits > 1 && !ws)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((N + TILE_N - 1) / TILE_N), (unsigned)p.splits);
  hipLaunchKernelGGL(gemv_w4_kernel, grid, dim3(64 * W4_WAVES), 0, st, reinterpret_cast<const bf16_t*>(x),
                     reinterpret_cast<const uint8_t*>(codes), reinterpret_cast<const int8_t*>(exps),
                     reinterpret_cast<bf16_t*>(out), ws, M, N, K, ldx, p.spb, p.splits);
  if (p.splits > 1) {
    const int err = (int)hipGetLastError();
    if (err) return err;
    const int64_t items = (int64_t)M * N;
    hipLaunchKernelGGL(gemv_w4_combine, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, ws,
                       reinterpret_cast<bf16_t*>(out), M, N, p.splits);
  }
  ND_LAUNCH_CHECK();
}
