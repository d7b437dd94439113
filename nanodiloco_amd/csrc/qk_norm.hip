// QK-norm: per-head RMSNorm of the q and k heads of the packed q|k|v projection output, alone (decode) or fused
// with RoPE (training / prefill forward), and its backward.
//
// Layout: rows = B*T tokens, each row = [q heads (nh*hd) | k heads (nkv*hd) | v heads (nkv*hd)], row stride `ld`
// elements; v is never read or written.  One (token, head) is owned by LPH = hd/16 neighbouring lanes; lane `sub`
// of them holds chunk `sub` (elements sub*8 .. sub*8+7) and chunk `sub + hd/16` (the same elements + hd/2), so
// both elements of every RoPE pair (i, i + hd/2) live in one lane (the StageRope layout of attention.hip) and a
// head is read once with 16-B (bf16) / 32-B (fp32) vector accesses.  The statistics are fp32, reduced over the LPH
// lanes with an xor butterfly (no LDS); a wave carries 64 / LPH heads, which may straddle rows.
//
// Forward:  rstd = rsqrt(mean_d x^2 + eps);  y = w * (x * rstd), w = wq for the q heads, wk for the k heads.
//   nd_qk_norm           stores y (rounded to the compute dtype) in place.
//   nd_qk_norm_rope_fwd  rounds y to the compute dtype exactly as nd_qk_norm stores it, then rotates it with
//                        rope.hip's arithmetic -- t = y_partner * sin, out = fma(y, cos, -+t), one rounding --
//                        written with explicit fma (as attn_decode.hip does), so the result is bitwise
//                        nd_rope_inplace(nd_qk_norm(x)).  It also writes rstd [rows, nh + nkv] and, when `save`
//                        is given, the raw q|k compactly ([rows, (nh + nkv) * hd]) for the backward.
// Every sum is written with explicit fma in a fixed order and shared by both forward kernels.
//
// Backward (nd_qk_norm_bwd), in place on the gradient dy with respect to the normed q|k (v columns untouched):
//   xhat = x * rstd;  g = w * dy;  dx = rstd * (g - xhat * mean_d(g * xhat));  dw[d] += sum_{token, head} dy * xhat.
// dw partials stay in registers across the heads a lane visits (one set for q, one for k); the lanes that hold the
// same chunk are summed by butterfly, the four waves through LDS in wave order, one partial row [dwq | dwk] per
// block; a second launch adds the partial rows into the fp32 gradient views in a fixed order (beta = 1, no
// atomics: bitwise repeatable).
#include "common.h"

using namespace nd;

namespace {

constexpr int QKN_THREADS = 256;
constexpr int QKN_MAX_PARTS = 1024;  // partial rows of the backward == its grid (the finishing kernel's budget)

template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int o = LPH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float sumsq16(const float* a, const float* b) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(a[j], a[j], ss);
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(b[j], b[j], ss);
  return ss;
}

template <int HD, int DT, bool ROPE>
__global__ void __launch_bounds__(QKN_THREADS) qk_norm_fwd_kernel(void* qkv, const float* __restrict__ wq,
                                                                  const float* __restrict__ wk,
                                                                  const float* __restrict__ cosT,
                                                                  const float* __restrict__ sinT,
                                                                  float* __restrict__ rstd_out, void* __restrict__ save,
                                                                  int64_t rows, int T, int nh, int nkv, int64_t ld,
                                                                  float eps) {
#pragma clang fp contract(off)
  constexpr int LPH = HD / 16, GPB = QKN_THREADS / LPH, HALF = HD / 2;
  const int nheads = nh + nkv;
  const int64_t total = rows * nheads;
  const int sub = threadIdx.x % LPH, g = threadIdx.x / LPH;
  for (int64_t it0 = (int64_t)blockIdx.x * GPB; it0 < total; it0 += (int64_t)gridDim.x * GPB) {
    const int64_t item = it0 + g;
    const bool valid = item < total;  // the same for the LPH lanes of a head
    float a[8], b[8];
    int64_t row = 0, off = 0;
    int head = 0;
    if (valid) {
      row = item / nheads;
      head = (int)(item - row * nheads);
      off = row * ld + (int64_t)head * HD + sub * 8;
      Vec8<DT>::load(qkv, off, a);
      Vec8<DT>::load(qkv, off + HALF, b);
      if (save) {
        const int64_t so = item * HD + sub * 8;
        Vec8<DT>::store(save, so, a);
        Vec8<DT>::store(save, so + HALF, b);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
    }
    const float ss = head_sum<LPH>(sumsq16(a, b));
    const float rs = rsqrtf(ss * (1.f / (float)HD) + eps);
    if (!valid) continue;
    if (rstd_out && sub == 0) rstd_out[item] = rs;
    const float* w = head < nh ? wq : wk;
    float wa[8], wb[8];
    Vec8<F32>::load(w, sub * 8, wa);
    Vec8<F32>::load(w, HALF + sub * 8, wb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = wa[j] * (a[j] * rs);
      b[j] = wb[j] * (b[j] * rs);
    }
    if (ROPE) {
      if (DT == BF16) {  // the value nd_qk_norm stores
        round_bf16x8(a);
        round_bf16x8(b);
      }
      const int64_t tb = (row % T) * HD + sub * 8;
      float c[8], s[8];
      Vec8<F32>::load(cosT, tb, c);
      Vec8<F32>::load(sinT, tb, s);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float ta = b[j] * s[j], tb2 = a[j] * s[j];
        const float ya = __builtin_fmaf(a[j], c[j], -ta);
        const float yb = __builtin_fmaf(b[j], c[j], tb2);
        a[j] = ya;
        b[j] = yb;
      }
    }
    Vec8<DT>::store(qkv, off, a);
    Vec8<DT>::store(qkv, off + HALF, b);
  }
}

template <int HD, int DT>
__global__ void __launch_bounds__(QKN_THREADS) qk_norm_bwd_kernel(void* dqkv, const void* __restrict__ x,
                                                                  const float* __restrict__ rstd,
                                                                  const float* __restrict__ wq,
                                                                  const float* __restrict__ wk, float* __restrict__ part,
                                                                  int64_t rows, int nh, int nkv, int64_t ld) {
#pragma clang fp contract(off)
  constexpr int LPH = HD / 16, GPB = QKN_THREADS / LPH, HALF = HD / 2;
  __shared__ float sdw[QKN_THREADS / 64][2 * HD];  // the block combine of the weight-gradient partials
  const int nheads = nh + nkv;
  const int64_t total = rows * nheads;
  const int sub = threadIdx.x % LPH, g = threadIdx.x / LPH;
  float accq[16], acck[16];  // [0..7]: chunk sub, [8..15]: chunk sub + hd/16
#pragma unroll
  for (int j = 0; j < 16; ++j) accq[j] = acck[j] = 0.f;
  for (int64_t it0 = (int64_t)blockIdx.x * GPB; it0 < total; it0 += (int64_t)gridDim.x * GPB) {
    const int64_t item = it0 + g;
    const bool valid = item < total;
    float da[8], db[8], xa[8], xb[8], wa[8], wb[8];
    float rs = 0.f;
    int64_t off = 0;
    bool isq = true;
    if (valid) {
      const int64_t row = item / nheads;
      const int head = (int)(item - row * nheads);
      isq = head < nh;
      off = row * ld + (int64_t)head * HD + sub * 8;
      Vec8<DT>::load(dqkv, off, da);
      Vec8<DT>::load(dqkv, off + HALF, db);
      const int64_t so = item * HD + sub * 8;
      Vec8<DT>::load(x, so, xa);
      Vec8<DT>::load(x, so + HALF, xb);
      rs = rstd[item];
      const float* w = isq ? wq : wk;
      Vec8<F32>::load(w, sub * 8, wa);
      Vec8<F32>::load(w, HALF + sub * 8, wb);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) da[j] = db[j] = xa[j] = xb[j] = wa[j] = wb[j] = 0.f;
    }
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xa[j] *= rs;  // xhat
      const float dw = da[j] * xa[j];
      accq[j] += isq ? dw : 0.f;
      acck[j] += isq ? 0.f : dw;
      da[j] *= wa[j];  // g
      dot = __builtin_fmaf(da[j], xa[j], dot);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xb[j] *= rs;
      const float dw = db[j] * xb[j];
      accq[8 + j] += isq ? dw : 0.f;
      acck[8 + j] += isq ? 0.f : dw;
      db[j] *= wb[j];
      dot = __builtin_fmaf(db[j], xb[j], dot);
    }
    dot = head_sum<LPH>(dot) * (1.f / (float)HD);
    if (valid) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        da[j] = rs * (da[j] - xa[j] * dot);
        db[j] = rs * (db[j] - xb[j] * dot);
      }
      Vec8<DT>::store(dqkv, off, da);
      Vec8<DT>::store(dqkv, off + HALF, db);
    }
  }
  // lanes sub, sub + LPH, sub + 2 LPH, ... of a wave hold the same chunks: butterfly over them, then the four waves
  // in wave order through LDS
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int o = LPH; o < 64; o <<= 1) {
      accq[j] += __shfl_xor(accq[j], o, 64);
      acck[j] += __shfl_xor(acck[j], o, 64);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < LPH) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sdw[wave][lane * 8 + j] = accq[j];
      sdw[wave][HALF + lane * 8 + j] = accq[8 + j];
      sdw[wave][HD + lane * 8 + j] = acck[j];
      sdw[wave][HD + HALF + lane * 8 + j] = acck[8 + j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * HD; i += QKN_THREADS)
    part[(int64_t)blockIdx.x * (2 * HD) + i] = ((sdw[0][i] + sdw[1][i]) + sdw[2][i]) + sdw[3][i];
}

// gwq[c] += sum_r part[r][c], gwk[c] += sum_r part[r][hd + c]: 1024 / (2 hd) row groups per column, each summing
// its rows in order, the groups combined through LDS in group order.
__global__ void __launch_bounds__(1024) qk_norm_dw_finish_kernel(const float* __restrict__ part, int nparts, int hd,
                                                                 float* gwq, float* gwk) {
  __shared__ float red[1024];
  const int cols = 2 * hd, groups = 1024 / cols;
  const int c = threadIdx.x % cols, gr = threadIdx.x / cols;
  float acc = 0.f;
  for (int r = gr; r < nparts; r += groups) acc += part[(int64_t)r * cols + c];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (gr == 0) {
    float s = red[c];
    for (int i = 1; i < groups; ++i) s += red[i * cols + c];
    float* dst = c < hd ? gwq + c : gwk + (c - hd);
    *dst += s;
  }
}

bool qkn_args_ok(const void* qkv, int dt, int64_t rows, int nh, int nkv, int hd, int64_t ld) {
  if (hd != 32 && hd != 64 && hd != 128) return false;
  if ((dt != F32 && dt != BF16) || rows < 0 || nh < 1 || nkv < 1) return false;
  if (ld < (int64_t)(nh + nkv) * hd || ld % 8 || ((uintptr_t)qkv & 15)) return false;
  return true;
}

unsigned qkn_fwd_blocks(int64_t rows, int nheads, int hd) {
  const int64_t gpb = QKN_THREADS / (hd / 16);
  int64_t blocks = (rows * nheads + gpb - 1) / gpb;
  if (blocks > 4096) blocks = 4096;
  return (unsigned)blocks;
}

template <bool ROPE>
int qkn_fwd_launch(void* qkv, int dt, const float* wq, const float* wk, const float* cosT, const float* sinT,
                   float* rstd, void* save, int64_t rows, int T, int nh, int nkv, int hd, int64_t ld, float eps,
                   hipStream_t s) {
  const dim3 grid(qkn_fwd_blocks(rows, nh + nkv, hd)), block(QKN_THREADS);
#define ND_QKN_FWD(HD, DT) \
  hipLaunchKernelGGL((qk_norm_fwd_kernel<HD, DT, ROPE>), grid, block, 0, s, qkv, wq, wk, cosT, sinT, rstd, save, rows, \
                     T, nh, nkv, ld, eps)
  if (dt == BF16) {
    if (hd == 32) ND_QKN_FWD(32, BF16);
    else if (hd == 64) ND_QKN_FWD(64, BF16);
    else ND_QKN_FWD(128, BF16);
  } else {
    if (hd == 32) ND_QKN_FWD(32, F32);
    else if (hd == 64) ND_QKN_FWD(64, F32);
    else ND_QKN_FWD(128, F32);
  }
#undef ND_QKN_FWD
  ND_LAUNCH_CHECK();
}

}  // namespace

// y = w * x * rstd on the q and k heads of every row, in place (the decode step's form).
ND_API int nd_qk_norm(void* qkv, int dt, const float* wq, const float* wk, int64_t rows, int nh, int nkv, int hd,
                      int64_t ld, float eps, hipStream_t s) {
  if (!qkn_args_ok(qkv, dt, rows, nh, nkv, hd, ld) || !wq || !wk) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  return qkn_fwd_launch<false>(qkv, dt, wq, wk, nullptr, nullptr, nullptr, nullptr, rows, 1, nh, nkv, hd, ld, eps, s);
}

// The same followed by RoPE at position row % T (tables fp32 [>= T, hd]); rstd [rows, nh + nkv]; save (optional):
// the raw q|k, [rows, (nh + nkv) * hd] in the dtype of qkv.
ND_API int nd_qk_norm_rope_fwd(void* qkv, int dt, const float* wq, const float* wk, const float* cosT,
                               const float* sinT, float* rstd, void* save, int64_t rows, int T, int nh, int nkv, int hd,
                               int64_t ld, float eps, hipStream_t s) {
  if (!qkn_args_ok(qkv, dt, rows, nh, nkv, hd, ld) || !wq || !wk || !cosT || !sinT || !rstd || T < 1 ||
      ((uintptr_t)save & 15) || ((uintptr_t)cosT & 15) || ((uintptr_t)sinT & 15))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  return qkn_fwd_launch<true>(qkv, dt, wq, wk, cosT, sinT, rstd, save, rows, T, nh, nkv, hd, ld, eps, s);
}

// dqkv: dy on entry, dx on return (q and k heads; v columns untouched).  x: the raw q|k the forward saved.
// part: nparts * 2 * hd floats, 1 <= nparts <= 1024 (nparts is the grid).  gwq / gwk (fp32 [hd], both or neither):
// accumulated into.
ND_API int nd_qk_norm_bwd(void* dqkv, int dt, const void* x, const float* rstd, const float* wq, const float* wk,
                          float* part, int nparts, float* gwq, float* gwk, int64_t rows, int nh, int nkv, int hd,
                          int64_t ld, hipStream_t s) {
  if (!qkn_args_ok(dqkv, dt, rows, nh, nkv, hd, ld) || !x || !rstd || !wq || !wk || !part || nparts < 1 ||
      nparts > QKN_MAX_PARTS || ((uintptr_t)x & 15) || (gwq == nullptr) != (gwk == nullptr))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  const dim3 grid((unsigned)nparts), block(QKN_THREADS);
#define ND_QKN_BWD(HD, DT) \
  hipLaunchKernelGGL((qk_norm_bwd_kernel<HD, DT>), grid, block, 0, s, dqkv, x, rstd, wq, wk, part, rows, nh, nkv, ld)
  if (dt == BF16) {
    if (hd == 32) ND_QKN_BWD(32, BF16);
    else if (hd == 64) ND_QKN_BWD(64, BF16);
    else ND_QKN_BWD(128, BF16);
  } else {
    if (hd == 32) ND_QKN_BWD(32, F32);
    else if (hd == 64) ND_QKN_BWD(64, F32);
    else ND_QKN_BWD(128, F32);
  }
#undef ND_QKN_BWD
  if (gwq)
    hipLaunchKernelGGL(qk_norm_dw_finish_kernel, dim3(1), dim3(1024), 0, s, part, nparts, hd, gwq, gwk);
  ND_LAUNCH_CHECK();
}
