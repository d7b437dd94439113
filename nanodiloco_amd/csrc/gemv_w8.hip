// fp8 weight-only projection for the decode step (docs/DESIGN.md "fp8 weight-only decode"):
//
//   out[M, N] (bf16) = x[M, K] (bf16) . dequant(codes, exps)^T,   1 <= M <= MAX_M = 16, fp32 accumulation (W8A16).
//
// Format.  W [N, K] is cut into groups of 128 along K: codes uint8 [N, K] (OCP e4m3) and exps int8 [N, K / 128],
// value = code * 2^e -- ops.decode.kv8_quantize on W.view(N, K / 128, 128), the KV cache's format.
//
// At these M the product is a stream of weight bytes, so the kernel is laid out around the code loads:
//   * Work split.  A workgroup (4 waves) owns one tile of 16 output channels and one K slice of `gpb` groups; the
//     partition (gpb, splits) is a pure function of (N, K) (w8_partition: about 1024 workgroups, never less than one
//     group per wave).  Wave w takes groups lo + w, lo + w + 4, ... of the slice, two of them in flight: all their
//     loads are issued before the first use.
//   * Data path.  Lane (c = lane & 15, q = lane >> 4) loads 16 code bytes of channel n0 + c at k = 128 g + 64 h + 16 q
//     (h = 0, 1): the four lanes of a channel cover 64 contiguous bytes per load, 128 per group, every code byte is
//     read once, straight into VGPRs.  v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 turn 8 codes into the exact bf16 values:
//     the B operand (k x 16 channels) of v_mfma_f32_16x16x32_bf16.  The A operand (16 rows of x, rows >= M zero) is
//     8 bf16 of x at the SAME k (the MFMA's k order is free as long as both operands agree), loaded from global
//     memory -- x is at most 16 x K bf16 and stays in L2 -- into registers; no LDS staging.  MAX_M = 16 is the MFMA's
//     row count: one instruction shape carries every M, a larger M belongs to the tile GEMMs.
//   * Scales.  The four MFMAs of a group accumulate from zero into a partial of its own; the group's exponent (one
//     per lane: accumulator column = lane & 15 = the lane's channel) is applied to that fp32 partial with ldexp -- a
//     power of two, exact, no float built from bits -- and the result is added to the wave's accumulator.
//   * Combine, fixed order, no atomics.  The four waves' accumulators meet in LDS and are added in wave order.  With
//     one K slice that sum is rounded to bf16 and stored; otherwise it goes to the fp32 workspace
//     [splits, MAX_M, N] and gemv_w8_combine adds the slices in slice order.
//   * Invariance.  An output row is a set of MFMA rows: its bits depend on that row of x, the weight, N and K (the
//     partition) -- not on M, the row's index, the other rows or the run.
//   * Edges.  Channels >= N and rows >= M are neither loaded nor stored (zero operands); K = 128 is one group on
//     wave 0; a NaN code stays NaN through both conversions and the MFMA.
#include "common.h"

using namespace nd;

namespace {

constexpr int MAX_M = 16;         // rows of x: the MFMA's M
constexpr int GROUP = 128;        // codes per exponent
constexpr int TILE_N = 16;        // output channels per workgroup: the MFMA's N
constexpr int W8_WAVES = 4;       // waves per workgroup, splitting the K slice
constexpr int INFLIGHT = 2;       // groups a wave loads before it computes
constexpr int TARGET_WGS = 1024;  // four workgroups per CU

typedef __bf16 bfv8 __attribute__((ext_vector_type(8)));

struct W8Part {
  int gpb, splits;  // groups per workgroup, K slices
};
// The K partition: a pure function of (N, K).
inline W8Part w8_partition(int N, int K) {
  const int G = K / GROUP, tiles = (N + TILE_N - 1) / TILE_N;
  const int want = (TARGET_WGS + tiles - 1) / tiles;
  int gpb = (G + want - 1) / want;
  if (gpb < W8_WAVES) gpb = W8_WAVES;
  return {gpb, (G + gpb - 1) / gpb};
}

// 8 e4m3 codes (two dwords) -> 8 bf16, exact
__device__ __forceinline__ bfv8 codes8_bf16(uint32_t lo, uint32_t hi) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(bfv8, (u32x4{pack2(a.x, a.y), pack2(b.x, b.y), pack2(c.x, c.y), pack2(d.x, d.y)}));
}
__device__ __forceinline__ f32x4 mma(const uint4& a, const bfv8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfv8, a), b, c, 0, 0, 0);
}

__global__ void __launch_bounds__(64 * W8_WAVES)
gemv_w8_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ codes, const int8_t* __restrict__ exps,
               bf16_t* __restrict__ out, float* __restrict__ ws, int M, int N, int K, int64_t ldx, int gpb, int splits) {
  __shared__ float red[W8_WAVES][TILE_N * MAX_M];
  const int n0 = blockIdx.x * TILE_N, s = blockIdx.y;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int G = K / GROUP;
  const int g_lo = s * gpb, g_hi = min(G, g_lo + gpb);
  // the lane's channel (B operand and accumulator column) and its row of x (A operand): c in both roles
  const bool wlive = n0 + c < N, xlive = c < M;
  const uint8_t* wrow = codes + (int64_t)(wlive ? n0 + c : 0) * K + q * 16;
  const int8_t* erow = exps + (int64_t)(wlive ? n0 + c : 0) * G;
  const bf16_t* xrow = x + (int64_t)(xlive ? c : 0) * ldx + q * 16;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int g = g_lo + w; g < g_hi; g += W8_WAVES * INFLIGHT) {
    uint4 wv[INFLIGHT][2], xv[INFLIGHT][4];
    int e[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      const int gg = g + u * W8_WAVES;
      const bool live = gg < g_hi;  // wave-uniform
      e[u] = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        wv[u][h] = make_uint4(0, 0, 0, 0);
        xv[u][2 * h] = xv[u][2 * h + 1] = make_uint4(0, 0, 0, 0);
      }
      if (live && wlive) {
        wv[u][0] = *reinterpret_cast<const uint4*>(wrow + (int64_t)gg * GROUP);
        wv[u][1] = *reinterpret_cast<const uint4*>(wrow + (int64_t)gg * GROUP + 64);
        e[u] = erow[gg];
      }
      if (live && xlive) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4* xp = reinterpret_cast<const uint4*>(xrow + (int64_t)gg * GROUP + h * 64);
          xv[u][2 * h] = xp[0];
          xv[u][2 * h + 1] = xp[1];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      if (g + u * W8_WAVES < g_hi) {
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          p = mma(xv[u][2 * h], codes8_bf16(wv[u][h].x, wv[u][h].y), p);
          p = mma(xv[u][2 * h + 1], codes8_bf16(wv[u][h].z, wv[u][h].w), p);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += ldexpf(p[r], e[u]);
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
  for (int i = 1; i < W8_WAVES; ++i) v += red[i][threadIdx.x];
  if (m < M && n < N) {
    if (splits == 1) out[(int64_t)m * N + n] = f2bf(v);
    else ws[((int64_t)s * MAX_M + m) * N + n] = v;
  }
}

// out[m][n] = bf16(sum over the K slices, in slice order)
__global__ void __launch_bounds__(256)
gemv_w8_combine(const float* __restrict__ ws, bf16_t* __restrict__ out, int M, int N, int splits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float v = ws[(int64_t)m * N + n];
  for (int s = 1; s < splits; ++s) v += ws[((int64_t)s * MAX_M + m) * N + n];
  out[i] = f2bf(v);
}

bool w8_shape_ok(int N, int K) {
  return N >= 1 && N <= 0x7fffffff - TILE_N && K >= GROUP && K % GROUP == 0;
}

}  // namespace

// The largest M of nd_gemv_w8 (compile-time).
ND_API int nd_gemv_w8_max_m() { return MAX_M; }

// K slices of the (N, K) partition: > 1 means nd_gemv_w8 needs a workspace of splits * MAX_M * N floats.  0: bad shape.
ND_API int nd_gemv_w8_splits(int N, int K) { return w8_shape_ok(N, K) ? w8_partition(N, K).splits : 0; }

// x [M, K] bf16 (row stride ldx elements, a multiple of 8), codes uint8 [N, K], exps int8 [N, K / 128], out bf16
// [M, N] contiguous, ws fp32 [splits, MAX_M, N] (may be null when nd_gemv_w8_splits(N, K) == 1).  x, codes and ws
// 16-byte aligned.
ND_API int nd_gemv_w8(const void* x, const void* codes, const void* exps, void* out, float* ws, int M, int N, int K,
                      int64_t ldx, hipStream_t st) {
  if (M < 1 || M > MAX_M || !w8_shape_ok(N, K) || ldx < K || ldx % 8) return (int)hipErrorInvalidValue;
  if (!x || !codes || !exps || !out) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)x | (uintptr_t)codes | (uintptr_t)ws) & 15) || ((uintptr_t)out & 1)) return (int)hipErrorInvalidValue;
  const W8Part p = w8_partition(N, K);
  if (p.splits > 65535 || (p.splits > 1 && !ws)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((N + TILE_N - 1) / TILE_N), (unsigned)p.splits);
  hipLaunchKernelGGL(gemv_w8_kernel, grid, dim3(64 * W8_WAVES), 0, st, reinterpret_cast<const bf16_t*>(x),
                     reinterpret_cast<const uint8_t*>(codes), reinterpret_cast<const int8_t*>(exps),
                     reinterpret_cast<bf16_t*>(out), ws, M, N, K, ldx, p.gpb, p.splits);
  if (p.splits > 1) {
    const int err = (int)hipGetLastError();
    if (err) return err;
    const int64_t items = (int64_t)M * N;
    hipLaunchKernelGGL(gemv_w8_combine, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, ws,
                       reinterpret_cast<bf16_t*>(out), M, N, p.splits);
  }
  ND_LAUNCH_CHECK();
}
