// Low-rank (PowerSGD) transport of the DiLoCo pseudo-gradient with error feedback (format and rules:
// docs/DESIGN.md "Low-rank transport").  Every compressed matrix [m, n] of the flat vector travels as two thin
// factors P [m, R] and Q [n, R]; both are linear in the pseudo-gradient, so both are all-reduced.
//
//   nd_lowrank_project          acc = (sync - master) + e -> e ; P = acc Q -> wire 1 ; dense spans: sync - master
//   -- all-reduce(SUM) of wire 1 = [dense | all P] --
//   nd_lowrank_orthonormalize   modified Gram-Schmidt over the R columns of every summed P, in column order
//   nd_lowrank_backproject      Q_loc = acc^T P^ -> wire 2 (acc read from e)
//   -- all-reduce(SUM) of wire 2 = [all Q] --
//   nd_outer_nesterov_lowrank   s = sum_c P^[i,c] Q_sum[j,c] ; d = s / W ; e = acc - d ; the outer Nesterov update
//                               of outer_update.h with d ; Q <- Q_sum / W, dead columns re-seeded from Q0
//
// Tables (int64, one copy on the host for the launcher's checks and one on the device for the kernels):
//   matrices  nmat rows (offset, m, n, p_off, q_off): the matrix is flat[offset .. offset + m n), row-major; its P is
//             wire1[p_off .. p_off + m R), its Q is q[q_off .. q_off + n R) (and the same place in wire 2).  offset,
//             n and q_off are multiples of 4, so every row of the matrix and of Q starts on a 16-byte boundary.
//   dense     S rows (start, end) followed by the S + 1 packed offsets pre[0] = 0 .. pre[S]: wire1[pre[s] + i] carries
//             flat[start_s + i].  Any alignment and length; the dense part of a model is its norm weights, so these
//             kernels go element by element.
// All index arithmetic is 64-bit.  Nothing is launched when a table fails its check.
//
// The matrix kernels walk a list of work items (a block of rows or of columns of one matrix) with a capped grid;
// a workgroup's item index only grows, so it walks the table forwards and keeps the current matrix in registers.
// No atomics: every sum has one owner and a fixed order, so the same bytes give the same bits on every worker.
#include "common.h"
#include "outer_update.h"

using namespace nd;

namespace {

constexpr int NT = 256;         // threads per workgroup of the matrix kernels
constexpr int NW = NT / 64;     // waves per workgroup
constexpr int GRID_CAP = 1024;  // workgroups (every kernel here strides over the rest)
constexpr int ONT = 1024;       // orthonormalize: one workgroup per matrix
constexpr int BPC = 64;         // back-project: columns per work item, one per lane
constexpr int BNT = 1024;       // back-project: threads per workgroup
constexpr int MAXR = 32;
constexpr float DEP2 = 5.9604644775390625e-08f;  // 2^-24: a column that lost 12 bits of its norm is dependent

struct Mat {
  int64_t off, m, n, p, q;
};

__device__ __forceinline__ Mat load_mat(const int64_t* __restrict__ tab, int i) {
  const int64_t* r = tab + (int64_t)i * 5;
  return Mat{r[0], r[1], r[2], r[3], r[4]};
}

// Work item w -> (matrix, block inside it); COL 1: blocks of DIV rows, COL 2: blocks of DIV columns.
template <int COL, int DIV>
struct ItemCursor {
  const int64_t* __restrict__ tab;
  int nmat, mi;
  int64_t base, cnt;
  __device__ __forceinline__ ItemCursor(const int64_t* t, int n) : tab(t), nmat(n), mi(0), base(0) { cnt = count(0); }
  __device__ __forceinline__ int64_t count(int i) const { return (tab[(int64_t)i * 5 + COL] + DIV - 1) / DIV; }
  // w must not decrease between calls; false past the last matrix (never for w < the launcher's total)
  __device__ __forceinline__ bool seek(int64_t w) {
    while (w >= base + cnt) {
      if (mi + 1 >= nmat) return false;
      base += cnt;
      ++mi;
      cnt = count(mi);
    }
    return true;
  }
};

// dense table: the span of packed index k (binary search over pre[0 .. S])
__device__ __forceinline__ int64_t dense_flat(const int64_t* __restrict__ dt, int S, int64_t k) {
  const int64_t* pre = dt + 2 * (int64_t)S;
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  return dt[2 * (int64_t)lo] + (k - pre[lo]);
}

// d = s * inv_w ; returns a - d: TWO roundings.  The compiler contracts a plain `a - s * inv_w` (and HIP's __fmul_rn /
// __fsub_rn, which are plain operators) into one fma; the pragma keeps the residual the difference against the d
// that the update uses.
__device__ __forceinline__ float scaled_and_rest(float a, float s, float inv_w, float& d) {
#pragma clang fp contract(off)
  d = s * inv_w;
  return a - d;
}

unsigned capped(int64_t items) { return (unsigned)(items > GRID_CAP ? GRID_CAP : (items < 1 ? 1 : items)); }

// ------------------------------------------------------------------------------------------------ project
// A wave owns RW rows; its lanes stride over the columns 16 bytes at a time, each with RW x R running sums, and
// one butterfly per sum ends the row.  Q is re-read per row block from L1 / L2 (n R floats per matrix).
template <int RMAX, int RW>
__global__ void __launch_bounds__(NT) project_kernel(const float* __restrict__ sync, const float* __restrict__ master,
                                                     float* __restrict__ resid, const float* __restrict__ q,
                                                     float* __restrict__ wire1, const int64_t* __restrict__ tab,
                                                     int nmat, int64_t total, int R) {
  constexpr int RB = NW * RW;
  ItemCursor<1, RB> cur(tab, nmat);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    if (!cur.seek(w)) break;
    const Mat M = load_mat(tab, cur.mi);
    const int64_t r0 = (w - cur.base) * RB + (int64_t)wv * RW;
    if (r0 >= M.m) continue;  // wave-uniform; no barrier in this loop
    float acc[RW][RMAX];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int c = 0; c < RMAX; ++c) acc[r][c] = 0.f;
    for (int64_t j = (int64_t)lane * 4; j < M.n; j += 256) {  // n % 4 == 0: a vector is inside the row or past it
      float x[RW][4];
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        if (r0 + r < M.m) {
          const int64_t g = M.off + (r0 + r) * M.n + j;
          const float4 S = *reinterpret_cast<const float4*>(sync + g);
          const float4 P = *reinterpret_cast<const float4*>(master + g);
          const float4 E = *reinterpret_cast<const float4*>(resid + g);
          x[r][0] = (S.x - P.x) + E.x;
          x[r][1] = (S.y - P.y) + E.y;
          x[r][2] = (S.z - P.z) + E.z;
          x[r][3] = (S.w - P.w) + E.w;
          *reinterpret_cast<float4*>(resid + g) = make_float4(x[r][0], x[r][1], x[r][2], x[r][3]);
        } else {
          x[r][0] = x[r][1] = x[r][2] = x[r][3] = 0.f;
        }
      }
      const float* qj = q + M.q + j * R;
      if (R == RMAX) {  // R % 4 == 0: rows of Q are 16-byte aligned
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int c4 = 0; c4 < RMAX / 4; ++c4) {
            const float4 qv = *reinterpret_cast<const float4*>(qj + jj * RMAX + c4 * 4);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
              acc[r][c4 * 4 + 0] = __fmaf_rn(x[r][jj], qv.x, acc[r][c4 * 4 + 0]);
              acc[r][c4 * 4 + 1] = __fmaf_rn(x[r][jj], qv.y, acc[r][c4 * 4 + 1]);
              acc[r][c4 * 4 + 2] = __fmaf_rn(x[r][jj], qv.z, acc[r][c4 * 4 + 2]);
              acc[r][c4 * 4 + 3] = __fmaf_rn(x[r][jj], qv.w, acc[r][c4 * 4 + 3]);
            }
          }
      } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int c = 0; c < RMAX; ++c)
            if (c < R) {
              const float qv = qj[jj * R + c];
#pragma unroll
              for (int r = 0; r < RW; ++r) acc[r][c] = __fmaf_rn(x[r][jj], qv, acc[r][c]);
            }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      float out = 0.f;
#pragma unroll
      for (int c = 0; c < RMAX; ++c) {
        if (c < R) {  // the same in every lane
          const float v = wave_sum(acc[r][c]);
          if (lane == c) out = v;
        }
      }
      if (r0 + r < M.m && lane < R) wire1[M.p + (r0 + r) * R + lane] = out;
    }
  }
}

__global__ void __launch_bounds__(256) dense_project_kernel(const float* __restrict__ sync,
                                                            const float* __restrict__ master,
                                                            float* __restrict__ wire1,
                                                            const int64_t* __restrict__ dt, int S, int64_t total) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t g = dense_flat(dt, S, k);
    wire1[k] = sync[g] - master[g];
  }
}

// ------------------------------------------------------------------------------------------------ orthonormalize
// One workgroup per matrix.  Thread t owns rows t, t + ONT, ..., so a column's elements never change hands and only
// the sums cross threads: block_sum is a butterfly per wave and the waves' sums in wave order -- a fixed tree.
__global__ void __launch_bounds__(ONT) ortho_kernel(float* __restrict__ wire1, const int64_t* __restrict__ tab,
                                                    int nmat, int R) {
  __shared__ float red[ONT / 64];
  const int t = threadIdx.x;
  for (int mi = blockIdx.x; mi < nmat; mi += gridDim.x) {
    const Mat M = load_mat(tab, mi);
    float* P = wire1 + M.p;
    for (int c = 0; c < R; ++c) {
      float s0 = 0.f;
      for (int64_t i = t; i < M.m; i += ONT) {
        const float v = P[i * R + c];
        s0 = __fmaf_rn(v, v, s0);
      }
      s0 = block_sum<ONT>(s0, red);
      for (int k = 0; k < c; ++k) {
        float d = 0.f;
        for (int64_t i = t; i < M.m; i += ONT) d = __fmaf_rn(P[i * R + k], P[i * R + c], d);
        d = block_sum<ONT>(d, red);
        for (int64_t i = t; i < M.m; i += ONT) P[i * R + c] = __fmaf_rn(-d, P[i * R + k], P[i * R + c]);
      }
      float s1 = 0.f;
      for (int64_t i = t; i < M.m; i += ONT) {
        const float v = P[i * R + c];
        s1 = __fmaf_rn(v, v, s1);
      }
      s1 = block_sum<ONT>(s1, red);
      // zero, non-finite (NaN fails every comparison) or numerically dependent on the columns before it: dropped
      const bool keep = s1 > 0.f && s1 < INFINITY && s1 > s0 * DEP2;
      const float nrm = sqrtf(s1);
      for (int64_t i = t; i < M.m; i += ONT) P[i * R + c] = keep ? P[i * R + c] / nrm : 0.f;
    }
  }
}

__device__ __forceinline__ float comp_of(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// The same Gram-Schmidt, right-looking, for R in {4, 8, 16, 32} with every P on a 16-byte boundary: once column k is
// normalised, its projection is taken out of EVERY later column in one sweep, so a step reads whole rows (contiguous
// 16-byte vectors) instead of walking two columns with a stride of R.  Per column the operations and their order are
// those of ortho_kernel; only the order inside the sums differs.  Thread t owns the vectors t, t + ONT, ... of P:
// always the same four columns (quad g = t % G, G = R / 4), and the G lanes of one row are neighbours, so a row's
// column-k element is one shuffle away.  Sums: per thread in vector order, a butterfly over the lanes of equal quad,
// then the waves in wave order.
template <int R>
__global__ void __launch_bounds__(ONT) ortho_rows_kernel(float* __restrict__ wire1, const int64_t* __restrict__ tab,
                                                         int nmat) {
  constexpr int G = R / 4, NWV = ONT / 64;
  __shared__ float red[NWV][G][4];   // the dots of a step
  __shared__ float red0[NWV][G][4];  // squared norms of the columns as they came
  __shared__ float red1[NWV];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, g = t % G;
  const int row_lane = (lane / G) * G;  // first lane of this lane's row
  for (int mi = blockIdx.x; mi < nmat; mi += gridDim.x) {
    const Mat M = load_mat(tab, mi);
    float4* P4 = reinterpret_cast<float4*>(wire1 + M.p);
    const int64_t total = M.m * G;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t f = t; f < total; f += ONT) {
      const float4 V = P4[f];
      a[0] = __fmaf_rn(V.x, V.x, a[0]);
      a[1] = __fmaf_rn(V.y, V.y, a[1]);
      a[2] = __fmaf_rn(V.z, V.z, a[2]);
      a[3] = __fmaf_rn(V.w, V.w, a[3]);
    }
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
      for (int o = 32; o >= G; o >>= 1) a[cc] += __shfl_xor(a[cc], o, 64);
    __syncthreads();  // the previous matrix is done with red0
    if (lane < G)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) red0[wv][lane][cc] = a[cc];
    __syncthreads();
    float s1 = 0.f;
    for (int w = 0; w < NWV; ++w) s1 += red0[w][0][0];
    for (int k = 0; k < R; ++k) {
      const int gk = k >> 2, kc = k & 3;
      float s0 = 0.f;
      for (int w = 0; w < NWV; ++w) s0 += red0[w][gk][kc];
      const bool keep = s1 > 0.f && s1 < INFINITY && s1 > s0 * DEP2;  // as ortho_kernel
      const float nrm = sqrtf(s1);
      const bool mine = g >= gk;  // this quad still holds column k or a later one
      float d[4] = {0.f, 0.f, 0.f, 0.f};
      for (int64_t b = 0; b < total; b += ONT) {  // the same trip count in every lane: there is a shuffle inside
        const int64_t f = b + t;
        const bool act = mine && f < total;
        float4 V = act ? P4[f] : make_float4(0.f, 0.f, 0.f, 0.f);
        float qk = 0.f;
        if (g == gk) {
          qk = keep ? comp_of(V, kc) / nrm : 0.f;
          if (kc == 0) V.x = qk; else if (kc == 1) V.y = qk; else if (kc == 2) V.z = qk; else V.w = qk;
          if (act) P4[f] = V;
        }
        const float qb = __shfl(qk, row_lane + gk, 64);
        const float v[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (4 * g + cc > k) d[cc] = __fmaf_rn(qb, v[cc], d[cc]);
      }
      if (k == R - 1) break;  // the same for every thread
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
        for (int o = 32; o >= G; o >>= 1) d[cc] += __shfl_xor(d[cc], o, 64);
      __syncthreads();  // the previous step's readers are done with red
      if (lane < G)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) red[wv][lane][cc] = d[cc];
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        float s = 0.f;
        for (int w = 0; w < NWV; ++w) s += red[w][g][cc];
        d[cc] = s;
      }
      const int gn = (k + 1) >> 2, nc = (k + 1) & 3;
      float ss = 0.f;
      for (int64_t b = 0; b < total; b += ONT) {
        const int64_t f = b + t;
        const bool act = mine && f < total;
        float4 V = act ? P4[f] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float qb = __shfl(g == gk ? comp_of(V, kc) : 0.f, row_lane + gk, 64);
        float v[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (4 * g + cc > k) v[cc] = __fmaf_rn(-d[cc], qb, v[cc]);
        if (act) P4[f] = make_float4(v[0], v[1], v[2], v[3]);
        if (g == gn) {
          const float x = nc == 0 ? v[0] : nc == 1 ? v[1] : nc == 2 ? v[2] : v[3];
          ss = __fmaf_rn(x, x, ss);
        }
      }
      s1 = block_sum<ONT>(ss, red1);
    }
  }
}

// ------------------------------------------------------------------------------------------------ back-project
// A work item is 64 columns of one matrix, one per lane; wave w of 16 sums rows w, w + 16, ... in ascending order,
// eight rows in flight (a column walk is latency-bound: one 256-byte request per row and wave), the row of P^ being
// the same for the whole wave.  Then the 16 partial sums are added in wave order through LDS.
template <int RMAX>
__global__ void __launch_bounds__(BNT) backproject_kernel(const float* __restrict__ resid,
                                                          const float* __restrict__ wire1, float* __restrict__ wire2,
                                                          const int64_t* __restrict__ tab, int nmat, int64_t total,
                                                          int R) {
  constexpr int BNW = BNT / 64, FL = 8;
  __shared__ float part[RMAX][BPC];
  ItemCursor<2, BPC> cur(tab, nmat);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    if (!cur.seek(w)) break;  // the same for the whole workgroup
    const Mat M = load_mat(tab, cur.mi);
    const int64_t j0 = (w - cur.base) * BPC, j = j0 + lane;
    const bool in = j < M.n;
    const float* col = resid + M.off + (in ? j : j0);  // a lane past the row's end reads nothing
    const float* ph = wire1 + M.p;
    float acc[RMAX];
#pragma unroll
    for (int c = 0; c < RMAX; ++c) acc[c] = 0.f;
    int64_t i = wv;
    for (; i + (FL - 1) * BNW < M.m; i += FL * BNW) {
      float x[FL];
#pragma unroll
      for (int u = 0; u < FL; ++u) x[u] = in ? col[(i + u * BNW) * M.n] : 0.f;
#pragma unroll
      for (int u = 0; u < FL; ++u) {
        const float* pr = ph + (i + u * BNW) * R;
#pragma unroll
        for (int c = 0; c < RMAX; ++c)
          if (c < R) acc[c] = __fmaf_rn(x[u], pr[c], acc[c]);
      }
    }
    for (; i < M.m; i += BNW) {
      const float x = in ? col[i * M.n] : 0.f;
      const float* pr = ph + i * R;
#pragma unroll
      for (int c = 0; c < RMAX; ++c)
        if (c < R) acc[c] = __fmaf_rn(x, pr[c], acc[c]);
    }
    for (int u = 0; u < BNW; ++u) {  // wave 0's sums, then + wave 1's, ...: a fixed order
      if (wv == u) {
#pragma unroll
        for (int c = 0; c < RMAX; ++c) part[c][lane] = u == 0 ? acc[c] : part[c][lane] + acc[c];
      }
      __syncthreads();
    }
    for (int idx = threadIdx.x; idx < R * BPC; idx += BNT) {
      const int l = idx / R, c = idx - l * R;  // consecutive threads write consecutive words of wire 2
      if (j0 + l < M.n) wire2[M.q + (j0 + l) * R + c] = part[c][l];
    }
    __syncthreads();  // the next item overwrites `part`
  }
}

// ------------------------------------------------------------------------------------------------ apply
// A wave owns 4 rows and strides over the columns 16 bytes at a time; per element one fma chain over c ascending.
template <int RMAX, int SDT>
__global__ void __launch_bounds__(NT) apply_kernel(float* __restrict__ p, float* __restrict__ sync,
                                                   float* __restrict__ resid, const float* __restrict__ wire1,
                                                   const float* __restrict__ wire2, float* __restrict__ buf,
                                                   void* __restrict__ sh, float* __restrict__ s_out,
                                                   const int64_t* __restrict__ tab, int nmat, int64_t total, int R,
                                                   float inv_w, float lr, float mu, int first) {
  constexpr int RW = 4, RB = NW * RW;
  ItemCursor<1, RB> cur(tab, nmat);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    if (!cur.seek(w)) break;
    const Mat M = load_mat(tab, cur.mi);
    const int64_t r0 = (w - cur.base) * RB + (int64_t)wv * RW;
    if (r0 >= M.m) continue;
    const int nr = (int)(M.m - r0 < RW ? M.m - r0 : RW);  // rows of this wave, >= 1
    for (int64_t j = (int64_t)lane * 4; j < M.n; j += 256) {
      float s[RW][4];
#pragma unroll
      for (int r = 0; r < RW; ++r) s[r][0] = s[r][1] = s[r][2] = s[r][3] = 0.f;
      const float* qj = wire2 + M.q + j * R;
      // a row past the matrix repeats the last one: its sums are never stored
      if (R == RMAX) {  // R % 4 == 0: the rows of Q are 16-byte aligned; per (row, column) c still ascends
#pragma unroll
        for (int c4 = 0; c4 < RMAX / 4; ++c4) {
          float pv[RW][4];
#pragma unroll
          for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) pv[r][cc] = wire1[M.p + (r0 + (r < nr ? r : nr - 1)) * RMAX + c4 * 4 + cc];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const float4 qv = *reinterpret_cast<const float4*>(qj + jj * RMAX + c4 * 4);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
              s[r][jj] = __fmaf_rn(pv[r][0], qv.x, s[r][jj]);
              s[r][jj] = __fmaf_rn(pv[r][1], qv.y, s[r][jj]);
              s[r][jj] = __fmaf_rn(pv[r][2], qv.z, s[r][jj]);
              s[r][jj] = __fmaf_rn(pv[r][3], qv.w, s[r][jj]);
            }
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < RMAX; ++c) {
          if (c < R) {
            float qv[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) qv[jj] = qj[jj * R + c];
#pragma unroll
            for (int r = 0; r < RW; ++r) {
              const float pv = wire1[M.p + (r0 + (r < nr ? r : nr - 1)) * R + c];
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) s[r][jj] = __fmaf_rn(pv, qv[jj], s[r][jj]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        if (r >= nr) break;
        const int64_t g = M.off + (r0 + r) * M.n + j;
        const float4 A = *reinterpret_cast<const float4*>(resid + g);
        const float4 B = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(buf + g);
        const float4 So = *reinterpret_cast<const float4*>(sync + g);
        const float a[4] = {A.x, A.y, A.z, A.w};
        float b[4] = {B.x, B.y, B.z, B.w}, so[4] = {So.x, So.y, So.z, So.w}, np[4], e[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float d;
          e[jj] = scaled_and_rest(a[jj], s[r][jj], inv_w, d);
          np[jj] = outer_update(d, b[jj], so[jj], 0.f, false, 0.f, lr, mu, first);
        }
        *reinterpret_cast<float4*>(resid + g) = make_float4(e[0], e[1], e[2], e[3]);
        *reinterpret_cast<float4*>(buf + g) = make_float4(b[0], b[1], b[2], b[3]);
        *reinterpret_cast<float4*>(sync + g) = make_float4(so[0], so[1], so[2], so[3]);
        *reinterpret_cast<float4*>(p + g) = make_float4(np[0], np[1], np[2], np[3]);
        if (SDT == BF16)
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(sh) + g) = make_uint2(pack2(np[0], np[1]), pack2(np[2], np[3]));
        if (s_out) *reinterpret_cast<float4*>(s_out + g) = make_float4(s[r][0], s[r][1], s[r][2], s[r][3]);
      }
    }
  }
}

template <int SDT>
__global__ void __launch_bounds__(256) dense_apply_kernel(float* __restrict__ p, float* __restrict__ sync,
                                                          const float* __restrict__ wire1, float* __restrict__ buf,
                                                          void* __restrict__ sh, float* __restrict__ s_out,
                                                          const int64_t* __restrict__ dt, int S, int64_t total,
                                                          float inv_w, float lr, float mu, int first) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int64_t g = dense_flat(dt, S, k);
    const float x = wire1[k];
    float b = first ? 0.f : buf[g];
    float so = sync[g];
    const float np = outer_update(x * inv_w, b, so, 0.f, false, 0.f, lr, mu, first);
    buf[g] = b;
    sync[g] = so;
    p[g] = np;
    if (SDT == BF16) reinterpret_cast<bf16_t*>(sh)[g] = f2bf(np);
    if (s_out) s_out[g] = x;
  }
}

// Q <- Q_sum / W per matrix and column; a column that is all zero or holds a non-finite value is taken from Q0.
__global__ void __launch_bounds__(NT) q_update_kernel(float* __restrict__ q, const float* __restrict__ q0,
                                                      const float* __restrict__ wire2,
                                                      const int64_t* __restrict__ tab, int nmat, int R, float inv_w) {
  for (int mi = blockIdx.x; mi < nmat; mi += gridDim.x) {
    const Mat M = load_mat(tab, mi);
    for (int c = 0; c < R; ++c) {
      int bad = 0, nz = 0;
      for (int64_t j = threadIdx.x; j < M.n; j += NT) {
        const float v = wire2[M.q + j * R + c] * inv_w;
        bad |= !(fabsf(v) < INFINITY);
        nz |= v != 0.f;
      }
      const int anybad = __syncthreads_or(bad);
      const int anynz = __syncthreads_or(nz);
      const bool reseed = anybad || !anynz;
      for (int64_t j = threadIdx.x; j < M.n; j += NT) {
        const int64_t a = M.q + j * R + c;
        q[a] = reseed ? q0[a] : wire2[a] * inv_w;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host checks
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Every matrix inside [0, span), its P inside wire 1 (w1 elements), its Q inside the Q buffers (w2 elements).
// items: blocks of `rb` rows (rb > 0) or of BPC columns (rb == 0) over all matrices.
bool check_mats(const int64_t* h, int nmat, int R, int64_t span, int64_t w1, int64_t w2, int rb, int64_t* items) {
  if (nmat < 0 || R < 1 || R > MAXR || span < 0 || w1 < 0 || w2 < 0 || (nmat > 0 && !h)) return false;
  int64_t it = 0;
  for (int i = 0; i < nmat; ++i) {
    const int64_t off = h[5 * i], m = h[5 * i + 1], n = h[5 * i + 2], po = h[5 * i + 3], qo = h[5 * i + 4];
    if (off < 0 || m < 1 || n < 1 || off > span || (off & 3) || (n & 3) || (qo & 3)) return false;
    if (m > (span - off) / n) return false;  // off + m n <= span without overflow
    if (po < 0 || po > w1 || m > (w1 - po) / R) return false;
    if (qo < 0 || qo > w2 || n > (w2 - qo) / R) return false;
    it += rb > 0 ? (m + rb - 1) / rb : (n + BPC - 1) / BPC;
  }
  if (items) *items = it;
  return true;
}

bool check_dense(const int64_t* h, int S, int64_t span, int64_t w1, int64_t* total) {
  *total = 0;
  if (S < 0 || (S > 0 && !h)) return false;
  if (S == 0) return true;
  const int64_t* pre = h + 2 * (int64_t)S;
  if (pre[0] != 0) return false;
  for (int s = 0; s < S; ++s) {
    const int64_t a = h[2 * s], b = h[2 * s + 1];
    if (a < 0 || b <= a || b > span || pre[s + 1] - pre[s] != b - a) return false;
  }
  if (pre[S] > w1) return false;
  *total = pre[S];
  return true;
}

unsigned dense_grid(int64_t total) { return capped((total + 255) / 256); }

}  // namespace

#define ND_BY_RANK(R, CALL) \
  do {                      \
    if ((R) <= 4) { CALL(4); } else if ((R) <= 8) { CALL(8); } else if ((R) <= 16) { CALL(16); } else { CALL(32); } \
  } while (0)

// sync / master / resid: `span` fp32 each, 16-byte aligned (resid is rewritten in place on the matrices); q: w2 fp32;
// wire1: w1 fp32; both 16-byte aligned.  htab / hdense: the host copies of dtab / ddense.
ND_API int nd_lowrank_project(const float* sync, const float* master, float* resid, const float* q, float* wire1,
                              const int64_t* htab, const int64_t* dtab, int nmat, const int64_t* hdense,
                              const int64_t* ddense, int S, int R, int64_t span, int64_t w1, int64_t w2,
                              hipStream_t s) {
  int64_t dtotal = 0, items = 0;
  if (!sync || !master || !resid || !q || !wire1 || (nmat > 0 && !dtab) || (S > 0 && !ddense)) return (int)hipErrorInvalidValue;
  if (!aligned(sync, 16) || !aligned(master, 16) || !aligned(resid, 16) || !aligned(q, 16) || !aligned(wire1, 16))
    return (int)hipErrorInvalidValue;
  if (R < 1 || R > MAXR) return (int)hipErrorInvalidValue;
  const int rw = R <= 8 ? 4 : 2;
  if (!check_mats(htab, nmat, R, span, w1, w2, NW * rw, &items) || !check_dense(hdense, S, span, w1, &dtotal))
    return (int)hipErrorInvalidValue;
  if (dtotal > 0)
    hipLaunchKernelGGL(dense_project_kernel, dim3(dense_grid(dtotal)), dim3(256), 0, s, sync, master, wire1, ddense, S, dtotal);
  if (items > 0) {
#define ND_PJ(RM) hipLaunchKernelGGL((project_kernel<RM, (RM <= 8 ? 4 : 2)>), dim3(capped(items)), dim3(NT), 0, s, sync, master, resid, q, wire1, dtab, nmat, items, R)
    ND_BY_RANK(R, ND_PJ);
#undef ND_PJ
  }
  ND_LAUNCH_CHECK();
}

ND_API int nd_lowrank_orthonormalize(float* wire1, const int64_t* htab, const int64_t* dtab, int nmat, int R,
                                     int64_t w1, hipStream_t s) {
  if (!wire1 || !aligned(wire1, 16) || (nmat > 0 && !dtab)) return (int)hipErrorInvalidValue;
  if (nmat < 0 || R < 1 || R > MAXR || w1 < 0 || (nmat > 0 && !htab)) return (int)hipErrorInvalidValue;
  bool rows = true;  // every P on a 16-byte boundary (with R % 4 == 0: all of them or none): the row-sweeping kernel
  for (int i = 0; i < nmat; ++i) {  // only P is touched: the rows of P inside wire 1
    const int64_t m = htab[5 * i + 1], po = htab[5 * i + 3];
    if (m < 1 || po < 0 || po > w1 || m > (w1 - po) / R) return (int)hipErrorInvalidValue;
    if (po & 3) rows = false;
  }
  if (nmat > 0) {
    const dim3 grid(capped(nmat)), block(ONT);
    if (rows && R == 4) hipLaunchKernelGGL(ortho_rows_kernel<4>, grid, block, 0, s, wire1, dtab, nmat);
    else if (rows && R == 8) hipLaunchKernelGGL(ortho_rows_kernel<8>, grid, block, 0, s, wire1, dtab, nmat);
    else if (rows && R == 16) hipLaunchKernelGGL(ortho_rows_kernel<16>, grid, block, 0, s, wire1, dtab, nmat);
    else if (rows && R == 32) hipLaunchKernelGGL(ortho_rows_kernel<32>, grid, block, 0, s, wire1, dtab, nmat);
    else hipLaunchKernelGGL(ortho_kernel, grid, block, 0, s, wire1, dtab, nmat, R);
  }
  ND_LAUNCH_CHECK();
}

ND_API int nd_lowrank_backproject(const float* resid, const float* wire1, float* wire2, const int64_t* htab,
                                  const int64_t* dtab, int nmat, int R, int64_t span, int64_t w1, int64_t w2,
                                  hipStream_t s) {
  int64_t items = 0;
  if (!resid || !wire1 || !wire2 || (nmat > 0 && !dtab)) return (int)hipErrorInvalidValue;
  if (!aligned(resid, 16) || !aligned(wire1, 16) || !aligned(wire2, 16)) return (int)hipErrorInvalidValue;
  if (!check_mats(htab, nmat, R, span, w1, w2, 0, &items)) return (int)hipErrorInvalidValue;
  if (items > 0) {
#define ND_BP(RM) hipLaunchKernelGGL((backproject_kernel<RM>), dim3(capped(items)), dim3(BNT), 0, s, resid, wire1, wire2, dtab, nmat, items, R)
    ND_BY_RANK(R, ND_BP);
#undef ND_BP
  }
  ND_LAUNCH_CHECK();
}

// master / sync / resid / mom (and s_out when given): `span` fp32, 16-byte aligned; sh (bf16, optional): 8-byte
// aligned; wire1 (w1), wire2 / q / q0 (w2 each): 16-byte aligned.
ND_API int nd_outer_nesterov_lowrank(float* master, float* sync, float* resid, const float* wire1, const float* wire2,
                                     float* q, const float* q0, float* mom, void* sh, int shdt, float* s_out,
                                     const int64_t* htab, const int64_t* dtab, int nmat, const int64_t* hdense,
                                     const int64_t* ddense, int S, int R, int64_t span, int64_t w1, int64_t w2,
                                     float inv_w, float lr, float mu, int first, hipStream_t s) {
  int64_t dtotal = 0, items = 0;
  if (!master || !sync || !resid || !wire1 || !wire2 || !q || !q0 || !mom || (nmat > 0 && !dtab) || (S > 0 && !ddense))
    return (int)hipErrorInvalidValue;
  if (!aligned(master, 16) || !aligned(sync, 16) || !aligned(resid, 16) || !aligned(wire1, 16) || !aligned(wire2, 16) ||
      !aligned(q, 16) || !aligned(q0, 16) || !aligned(mom, 16) || !aligned(sh, 8) || !aligned(s_out, 16))
    return (int)hipErrorInvalidValue;
  if (!check_mats(htab, nmat, R, span, w1, w2, NW * 4, &items) || !check_dense(hdense, S, span, w1, &dtotal))
    return (int)hipErrorInvalidValue;
  const bool bsh = sh && shdt == BF16;
  if (dtotal > 0) {
    if (bsh) hipLaunchKernelGGL(dense_apply_kernel<BF16>, dim3(dense_grid(dtotal)), dim3(256), 0, s, master, sync, wire1, mom, sh, s_out, ddense, S, dtotal, inv_w, lr, mu, first);
    else hipLaunchKernelGGL(dense_apply_kernel<F32>, dim3(dense_grid(dtotal)), dim3(256), 0, s, master, sync, wire1, mom, sh, s_out, ddense, S, dtotal, inv_w, lr, mu, first);
  }
  if (items > 0) {
#define ND_AP(RM)                                                                                                     \
  do {                                                                                                                \
    if (bsh) hipLaunchKernelGGL((apply_kernel<RM, BF16>), dim3(capped(items)), dim3(NT), 0, s, master, sync, resid, wire1, wire2, mom, sh, s_out, dtab, nmat, items, R, inv_w, lr, mu, first); \
    else hipLaunchKernelGGL((apply_kernel<RM, F32>), dim3(capped(items)), dim3(NT), 0, s, master, sync, resid, wire1, wire2, mom, sh, s_out, dtab, nmat, items, R, inv_w, lr, mu, first); \
  } while (0)
    ND_BY_RANK(R, ND_AP);
#undef ND_AP
    hipLaunchKernelGGL(q_update_kernel, dim3(capped(nmat)), dim3(NT), 0, s, q, q0, wire2, dtab, nmat, R, inv_w);
  }
  ND_LAUNCH_CHECK();
}
