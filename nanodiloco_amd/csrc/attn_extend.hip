// Multi-token (extend) attention against a KV cache on the matrix cores: L new tokens per sequence appended to a
// cache that already holds keys -- continuing a live cache, chunked prefill, scoring a block of candidates.
//
// One layer's step for B sequences.  qkv [B*L, (nh + 2 nkv) * hd] bf16 is the plain (un-rotated) q|k|v projection of
// the new tokens, row b*L + i = token i of sequence b, which sits at cache slot and RoPE position pos[b] + i (pos,
// kstart: device int32 as in attn_decode.hip; caches [B, nkv, S_max, hd]).  Query row i sees keys
// max(kstart[b], pos[b] + i - window + 1) .. pos[b] + i; scores are scale q.k, or C tanh(scale q.k / C) with a cap.
// Output o [B*L, nh * hd] bf16.  pos is not advanced; qkv is overwritten (q and k rotated in place).
//
// Three kernels on one stream, no atomics, no hand-off between workgroups inside a launch:
//   attn_extend_append   rotates q and k of all B*L rows in place (rope.hip's arithmetic: explicit fma, contraction
//                        off, one rounding) and writes the rotated k rows and the v rows to slots pos[b] .. pos[b]+L-1.
//                        A launch of its own, so that the attention reads EVERY key from the cache without a race.
//   attn_extend_kernel   grid (nkv * row_tiles, B, ceil(S_max / SPLIT)), 256 threads, per block of at most QBLOCK
//                        queries.  The L_b * rep query rows of kv head g (row = token * rep + head-in-group: a tile's
//                        rows are neighbouring tokens, its key range is tight) are cut into 32-row tiles, four tiles
//                        = four waves per workgroup.  The workgroup stages the chunk's K and V -- keys
//                        [c SPLIT, (c+1) SPLIT) by ABSOLUTE index, as the decode kernel partitions them -- once in
//                        LDS (swizzled like the training kernels' tiles); only the slots inside [min lo, max hi] of its
//                        rows are loaded, the rest of the tile is zero, so no slot past pos[b] + L - 1 or below kstart
//                        is ever read.  Each wave, queries on the lanes: S^T = K Q^T on v_mfma_f32_32x32x16_bf16 (four
//                        32-key blocks, Q fragments in registers), the row's own (lo, hi) mask, an exact two-pass
//                        softmax over the chunk in registers, P rounded to bf16, O^T += V^T P^T on the same MFMA with
//                        V through ds_read_b64_tr_b16.  It writes the fp32 partial (m, l, o[hd]) of each row.  A row
//                        without a live key in the chunk writes the empty partial (-inf, 0); a workgroup whose chunk
//                        lies outside its rows' key range does that for all its rows and leaves before touching K/V.
//   attn_extend_combine  grid (L_b * nh, B), hd threads: merges a row's partials in chunk order (only the chunks that
//                        meet its [lo, hi]) and writes bf16; a row with no live key (a pad query) writes zeros.
//
// Invariance: a row's bits depend on its query, its key range and SPLIT alone -- not on L, the row's place in a tile,
// B, or how a run of tokens was cut into calls.  The partition is by absolute key index; an MFMA output column (one
// query) is accumulated independently of its neighbours, the k-steps in key order; keys outside the row's range --
// zeros in LDS or other rows' live keys -- enter with p = +0 exactly; the row reductions are lane-local plus one
// exchange with lane ^ 32; the combine walks the chunks in order.
//
// K/V staging goes through registers, not the LDS-DMA of lds_dma.h: a chunk is live only between two row bounds and
// the rest must read as zero (0 * NaN of a stale slot would poison P V), which a lane-linear 1-KiB DMA piece cannot
// express at either end.
#include "lds_dma.h"
#include "softcap.h"

using namespace nd;

namespace {

#ifndef ND_DECODE_KERNELS_ONLY  // attn_kv8.hip includes this file after attn_decode.hip, which has these two
constexpr int SPLIT = 128;   // keys per workgroup: the decode kernel's partition (nd_attn_decode_split)
constexpr float LOG2E = 1.4426950408889634f;
#endif
constexpr int QBLOCK = 64;   // queries per attention / combine launch (the workspace is sized for it)
constexpr int XW = 4;        // waves = 32-row tiles per workgroup

// rope.hip's rotation of 8 elements x (first half) and y (second half, element + hd/2), as that kernel compiles:
// x' = fma(x, c, -(y * s)), y' = fma(y, c, x * s), rounded once to bf16 (attn_decode.hip's rope8)
__device__ __forceinline__ void rope_pair8(uint4& x, uint4& y, const float* c, const float* s) {
#pragma clang fp contract(off)
  const float a[8] = {lo_bf(x.x), hi_bf(x.x), lo_bf(x.y), hi_bf(x.y), lo_bf(x.z), hi_bf(x.z), lo_bf(x.w), hi_bf(x.w)};
  const float p[8] = {lo_bf(y.x), hi_bf(y.x), lo_bf(y.y), hi_bf(y.y), lo_bf(y.z), hi_bf(y.z), lo_bf(y.w), hi_bf(y.w)};
  float u[8], v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t1 = p[j] * s[j], t2 = a[j] * s[j];
    u[j] = __builtin_fmaf(a[j], c[j], -t1);
    v[j] = __builtin_fmaf(p[j], c[j], t2);
  }
  x.x = pack2(u[0], u[1]); x.y = pack2(u[2], u[3]); x.z = pack2(u[4], u[5]); x.w = pack2(u[6], u[7]);
  y.x = pack2(v[0], v[1]); y.y = pack2(v[2], v[3]); y.z = pack2(v[4], v[5]); y.w = pack2(v[6], v[7]);
}

// a sequence whose L new slots do not fit the cache reads and writes nothing
__device__ __forceinline__ bool bad_pos(int p, int L, int S_max) { return p < 0 || p > S_max - L; }

// One thread per (row, head, 8 pairs): q and k heads are rotated in place, k and v heads go to the cache.
__global__ void __launch_bounds__(256)
attn_extend_append(bf16_t* __restrict__ qkv, const float* __restrict__ cosT, const float* __restrict__ sinT,
                   const int* __restrict__ pos, bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, int B, int L,
                   int nh, int nkv, int hd, int S_max, int64_t ld) {
  const int half = hd >> 1, gpr = half >> 3, heads = nh + 2 * nkv;  // gpr: 16-B groups per half head
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
  if (head >= nh) {
    const bool isv = head >= nh + nkv;
    const int g = head - nh - (isv ? nkv : 0);
    bf16_t* dst = (isv ? vcache : kcache) + ((int64_t)(b * nkv + g) * S_max + slot) * hd + d0;
    *reinterpret_cast<uint4*>(dst) = x;
    *reinterpret_cast<uint4*>(dst + half) = y;
  }
}

// Stages keys [c0, c0 + SPLIT) of one (sequence, kv head) -- `row0` is its first cache row -- as swizzled LDS tiles:
// slots [glo, ghi] are loaded, the rest of the tile is zero.  All 64 * XW threads; the caller's barrier follows.
template <int HD>
__device__ __forceinline__ void stage_chunk(const bf16_t* kcache, const bf16_t* vcache, bf16_t* Ks, bf16_t* Vs,
                                            int64_t row0, int c0, int glo, int ghi) {
  constexpr int CPR = HD / 8;
  constexpr int NST = SPLIT * CPR / (64 * XW);  // 16-B pieces per thread and operand
  const bf16_t* kc = kcache + row0 * HD;
  const bf16_t* vc = vcache + row0 * HD;
  uint4 kr[NST], vr[NST];
#pragma unroll
  for (int it = 0; it < NST; ++it) {
    const int idx = threadIdx.x + it * (64 * XW);
    const int key = c0 + idx / CPR, ch = idx % CPR;
    kr[it] = make_uint4(0, 0, 0, 0);
    vr[it] = make_uint4(0, 0, 0, 0);
    if (key >= glo && key <= ghi) {
      kr[it] = *reinterpret_cast<const uint4*>(kc + (int64_t)key * HD + ch * 8);
      vr[it] = *reinterpret_cast<const uint4*>(vc + (int64_t)key * HD + ch * 8);
    }
  }
#pragma unroll
  for (int it = 0; it < NST; ++it) {
    const int idx = threadIdx.x + it * (64 * XW);
    const int o = soff<HD>(idx / CPR, (idx % CPR) * 8);
    *reinterpret_cast<uint4*>(&Ks[o]) = kr[it];
    *reinterpret_cast<uint4*>(&Vs[o]) = vr[it];
  }
}

// An fp8 cache operand (docs/DESIGN.md "fp8 KV cache"): e4m3 codes [B, nkv, S_max, hd] and one int8 exponent per row.
// Its staging -- codes and exponents to the exact bf16 value code * 2^e, the same tiles -- is in attn_kv8.hip.
struct Kv8 {
  const uint8_t* codes;
  const int8_t* exps;
};
template <int HD>
__device__ __forceinline__ void stage_chunk(Kv8 kcache, Kv8 vcache, bf16_t* Ks, bf16_t* Vs, int64_t row0, int c0,
                                            int glo, int ghi);

// The geometry of one attention / combine launch: queries off .. off + Lb - 1 of the L new tokens.
struct Block {
  int L, off, Lb;
};

// CA: empty, or one CapArgs: the scores become C log2(e) tanh(q.k scale / C), and `scale2` is then the plain scale
// (as attn_decode_kernel).  KC: the cache operand, const bf16_t* or Kv8 -- only stage_chunk looks at it.
template <int HD, class KC, class... CA>
__global__ void __launch_bounds__(64 * XW)
attn_extend_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ pos, const int* __restrict__ kstart,
                   KC kcache, KC vcache, float* __restrict__ part_o,
                   float* __restrict__ part_ml, int nkv, int rep, int row_tiles, int S_max, int64_t ld, float scale2,
                   int window, Block blk, CA... ca) {
  constexpr bool CAP = has_cap<CA...>;
  static_assert(sizeof...(CA) == (CAP ? 1 : 0), "at most one trailing argument, a CapArgs");
  constexpr int NT = HD / 16, NO = HD / 32;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[SPLIT * HD];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[SPLIT * HD];

  // the chunk is the slowest grid dimension (see attn_decode_kernel: the XCD round-robin)
  const int g = blockIdx.x / row_tiles, rt = blockIdx.x % row_tiles, b = blockIdx.y, c = blockIdx.z;
  const int nchunks = gridDim.z;
  const int rows = blk.Lb * rep;                       // query rows of one kv head in this launch
  const int r0 = rt * (32 * XW), r1 = min(rows, r0 + 32 * XW);  // this workgroup's rows [r0, r1), r0 < rows
  const int p = pos[b];
  const int ks = kstart ? max(kstart[b], 0) : 0;
  const int c0 = c * SPLIT;
  const int64_t pbase = ((int64_t)(b * nkv + g) * nchunks + c) * rows;  // the chunk's first partial row of (b, g)
  // token i's keys: lo(i) = max(ks, p + i - window + 1) .. hi(i) = p + i, both monotone in i
  const int gi0 = blk.off + r0 / rep, gi1 = blk.off + (r1 - 1) / rep;
  const int glo = max(ks, window > 0 ? p + gi0 - window + 1 : 0), ghi = p + gi1;
  if (bad_pos(p, blk.L, S_max) || c0 > ghi || c0 + SPLIT <= glo) {
    if ((int)threadIdx.x < r1 - r0) {
      part_ml[(pbase + r0 + threadIdx.x) * 2] = -INFINITY;
      part_ml[(pbase + r0 + threadIdx.x) * 2 + 1] = 0.f;
    }
    return;
  }

  // ---- stage the chunk: slots [glo, ghi] (inside [kstart, pos + L - 1], below S_max) are loaded, the rest is zero
  stage_chunk<HD>(kcache, vcache, Ks, Vs, (int64_t)(b * nkv + g) * S_max, c0, glo, ghi);

  // ---- this wave's tile: query row on the lane (both halves of the wave hold the same 32 rows)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, c32 = lane & 31, g16 = lane >> 4, i16 = lane & 15;
  const int rw0 = r0 + 32 * w, r = rw0 + c32;
  const bool valid = r < r1;
  const int ti = blk.off + min(r, r1 - 1) / rep;  // the row's token among the L new ones
  const int hq = g * rep + min(r, r1 - 1) % rep;
  const int lo = valid ? max(ks, window > 0 ? p + ti - window + 1 : 0) : 1, hi = valid ? p + ti : 0;
  bf16x8 qf[NT];
  {
    const bf16_t* qrow = qkv + ((int64_t)b * blk.L + ti) * ld + (int64_t)hq * HD + 8 * h;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      qf[t] = valid ? *reinterpret_cast<const bf16x8*>(qrow + 16 * t) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  __syncthreads();  // the only barrier: from here on the waves only read LDS
  if (rw0 >= r1) return;
  // the wave's key range (scalars: its first and last row's tokens)
  const int wi0 = blk.off + rw0 / rep, wi1 = blk.off + (min(rw0 + 32, r1) - 1) / rep;
  const int wlo = max(ks, window > 0 ? p + wi0 - window + 1 : 0), whi = p + wi1;

  // ---- S^T = K Q^T, four 32-key blocks; a block outside the wave's range stays masked
  const float ucap = scale2 * cap_of(ca...).inv, ccap = cap_of(ca...).cap * LOG2E;
  f32x16 s[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int k0 = c0 + kt * 32;
    if (k0 <= whi && k0 + 32 > wlo) {
      s[kt] = f32x16{};
#pragma unroll
      for (int t = 0; t < NT; ++t) s[kt] = mfma32(row_frag<HD>(Ks, kt * 32 + c32, t, h), qf[t], s[kt]);
#pragma unroll
      for (int x = 0; x < 16; ++x) {
        const int key = k0 + (x & 3) + 8 * (x >> 2) + 4 * h;
        float z;
        if constexpr (CAP) z = cap_tanh(s[kt][x] * ucap) * ccap;
        else z = s[kt][x] * scale2;
        s[kt][x] = (key >= lo && key <= hi) ? z : -INFINITY;
      }
    } else {
#pragma unroll
      for (int x = 0; x < 16; ++x) s[kt][x] = -INFINITY;
    }
  }

  // ---- the row's softmax over the chunk, exact two-pass: the lane's 64 scores, then the other half's
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int x = 0; x < 16; ++x) m = fmaxf(m, s[kt][x]);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float ms = m == -INFINITY ? 0.f : m;  // no live key: every p below is exp2(-inf) = 0
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int x = 0; x < 16; ++x) {
      s[kt][x] = __builtin_amdgcn_exp2f(s[kt][x] - ms);
      l += s[kt][x];
    }
  l += __shfl_xor(l, 32, 64);

  // ---- O^T += V^T P^T, P rounded to bf16
  f32x16 oacc[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) oacc[o] = f32x16{};
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int k0 = c0 + kt * 32;
    if (k0 <= whi && k0 + 32 > wlo) {
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = pack_frag(s[kt], sidx);
#pragma unroll
        for (int o = 0; o < NO; ++o)
          oacc[o] = mfma32(tr_frag<HD>(Vs, kt * 32 + 16 * sidx, o * 32, g16, i16), pf, oacc[o]);
      }
    }
  }

  // ---- the row's partial: accumulator register x of block o is o[d = 32 o + 8 (x >> 2) + 4 h + (x & 3)]
  if (valid) {
    const int64_t prow = pbase + r;
    float* po = part_o + prow * HD + 4 * h;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        *reinterpret_cast<float4*>(po + 32 * o + 8 * q4) =
            make_float4(oacc[o][4 * q4], oacc[o][4 * q4 + 1], oacc[o][4 * q4 + 2], oacc[o][4 * q4 + 3]);
    if (h == 0) *reinterpret_cast<float2*>(part_ml + prow * 2) = make_float2(m, l);
  }
}

// grid (Lb * nh, B), hd threads: o[b, off + i, head, :] from the row's partials, lowest chunk first; only the chunks
// that meet [lo, hi] are read (attn_decode_combine_kernel's loop: an empty chunk inside the range is dropped by a
// select, its o never used).
__global__ void attn_extend_combine(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                    const int* __restrict__ pos, const int* __restrict__ kstart,
                                    bf16_t* __restrict__ o, int nh, int nkv, int rep, int hd, int nchunks, int S_max,
                                    int window, Block blk) {
  const int il = blockIdx.x / nh, head = blockIdx.x % nh, b = blockIdx.y, d = threadIdx.x;
  const int g = head / rep, rows = blk.Lb * rep;
  const int64_t base = (int64_t)(b * nkv + g) * nchunks * rows + il * rep + head % rep;  // + c * rows: chunk c
  const int p = pos[b], ti = blk.off + il;
  const int ks = kstart ? max(kstart[b], 0) : 0;
  float M = -INFINITY, Lsum = 0.f, O = 0.f;
  if (!bad_pos(p, blk.L, S_max)) {
    const int lo = max(ks, window > 0 ? p + ti - window + 1 : 0), hi = p + ti;  // hi < S_max: hi / SPLIT < nchunks
    if (lo <= hi) {
      const int c_lo = lo / SPLIT, c_hi = hi / SPLIT;
#pragma unroll 4
      for (int c = c_lo; c <= c_hi; ++c) M = fmaxf(M, part_ml[(base + (int64_t)c * rows) * 2]);
#pragma unroll 4
      for (int c = c_lo; c <= c_hi; ++c) {
        const int64_t prow = base + (int64_t)c * rows;
        const float mc = part_ml[prow * 2], lc = part_ml[prow * 2 + 1];
        const float po = part_o[prow * hd + d];
        const bool live = mc != -INFINITY && lc != 0.f;
        const float f = __builtin_amdgcn_exp2f(mc - M);
        Lsum = live ? __builtin_fmaf(lc, f, Lsum) : Lsum;
        O = live ? __builtin_fmaf(po, f, O) : O;
      }
    }
  }
  o[(((int64_t)b * blk.L + ti) * nh + head) * hd + d] = f2bf(Lsum > 0.f ? O / Lsum : 0.f);
}

template <int HD, class KC, class... CA>
int launch_block(const bf16_t* qkv, const int* pos, const int* kstart, KC kc, KC vc,
                 float* part_o, float* part_ml, bf16_t* o, int B, int nh, int nkv, int S_max, int64_t ld, float scale2,
                 int window, Block blk, hipStream_t st, CA... ca) {
  const int rep = nh / nkv, nchunks = (S_max + SPLIT - 1) / SPLIT;
  const int row_tiles = (blk.Lb * rep + 32 * XW - 1) / (32 * XW);
  hipLaunchKernelGGL((attn_extend_kernel<HD, KC, CA...>), dim3((unsigned)(nkv * row_tiles), (unsigned)B, (unsigned)nchunks),
                     dim3(64 * XW), 0, st, qkv, pos, kstart, kc, vc, part_o, part_ml, nkv, rep, row_tiles, S_max, ld,
                     scale2, window, blk, ca...);
  hipLaunchKernelGGL(attn_extend_combine, dim3((unsigned)(blk.Lb * nh), (unsigned)B), dim3((unsigned)HD), 0, st, part_o,
                     part_ml, pos, kstart, o, nh, nkv, rep, HD, nchunks, S_max, window, blk);
  return (int)hipGetLastError();
}

template <class KC, class... CA>
int extend_blocks(const bf16_t* qkv, const int* pos, const int* kstart, KC kc, KC vc,
                  float* part_o, float* part_ml, bf16_t* o, int B, int L, int nh, int nkv, int hd, int S_max,
                  int64_t ld, float scale2, int window, hipStream_t st, CA... ca) {
  for (int off = 0; off < L; off += QBLOCK) {
    const Block blk{L, off, L - off < QBLOCK ? L - off : QBLOCK};
    int err;
    if (hd == 32) err = launch_block<32>(qkv, pos, kstart, kc, vc, part_o, part_ml, o, B, nh, nkv, S_max, ld, scale2, window, blk, st, ca...);
    else if (hd == 64) err = launch_block<64>(qkv, pos, kstart, kc, vc, part_o, part_ml, o, B, nh, nkv, S_max, ld, scale2, window, blk, st, ca...);
    else err = launch_block<128>(qkv, pos, kstart, kc, vc, part_o, part_ml, o, B, nh, nkv, S_max, ld, scale2, window, blk, st, ca...);
    if (err) return err;
  }
  return 0;
}

}  // namespace

#ifndef ND_EXTEND_KERNELS_ONLY  // attn_kv8.hip includes this file for everything but the library entries
// Queries per attention launch: the workspace holds the partials of this many (tests aim at its edge).
ND_API int nd_attn_extend_qblock() { return QBLOCK; }

// Workspace: part_o [B, nkv, nchunks, QBLOCK * rep, hd] fp32, part_ml [.., 2] fp32, nchunks = ceil(S_max / SPLIT);
// a block of Lb < QBLOCK queries uses the front of it.  `ld`: row stride of qkv in elements; o is contiguous
// [B*L, nh * hd].  The tables must hold at least S_max rows.  A sequence with pos[b] < 0 or pos[b] + L > S_max reads
// and writes nothing and gives o = 0.  window: 0 = none, W >= 1 = sliding window; cap: 0 = none, C > 0 = soft-cap.
ND_API int nd_attn_extend(void* qkv, const float* cosT, const float* sinT, const int* pos, const int* kstart,
                          void* kcache, void* vcache, float* part_o, float* part_ml, void* o, int B, int L, int nh,
                          int nkv, int hd, int S_max, int64_t ld, float scale, int window, float cap, hipStream_t st) {
  if (B < 1 || B > 65535 || L < 1 || nh < 1 || nkv < 1 || nh % nkv || nh / nkv > 8 || S_max < 1 || L > S_max ||
      (S_max + SPLIT - 1) / SPLIT > 65535 || (int64_t)B * L > 0x7fffffff)
    return (int)hipErrorInvalidValue;
  if (hd != 32 && hd != 64 && hd != 128) return (int)hipErrorInvalidValue;
  if (ld < (int64_t)(nh + 2 * nkv) * hd || ld % 8 || window < 0 || (cap != 0.f && !cap_ok(cap)))
    return (int)hipErrorInvalidValue;
  if (!qkv || !cosT || !sinT || !pos || !kcache || !vcache || !part_o || !part_ml || !o)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)cosT | (uintptr_t)sinT | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)part_o |
       (uintptr_t)part_ml) & 15)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)o & 1) || ((uintptr_t)pos & 3) || ((uintptr_t)kstart & 3)) return (int)hipErrorInvalidValue;
  bf16_t* x = reinterpret_cast<bf16_t*>(qkv);
  bf16_t* kc = reinterpret_cast<bf16_t*>(kcache);
  bf16_t* vc = reinterpret_cast<bf16_t*>(vcache);
  const bf16_t* kr = kc;  // the attention's read-only view: extend_blocks deduces its operand type from these
  const bf16_t* vr = vc;
  const int64_t items = (int64_t)B * L * (nh + 2 * nkv) * (hd / 16);
  if ((items + 255) / 256 > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_extend_append, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, cosT, sinT, pos,
                     kc, vc, B, L, nh, nkv, hd, S_max, ld);
  int err = (int)hipGetLastError();
  if (err) return err;
  bf16_t* out = reinterpret_cast<bf16_t*>(o);
  if (cap != 0.f)
    return extend_blocks(x, pos, kstart, kr, vr, part_o, part_ml, out, B, L, nh, nkv, hd, S_max, ld, scale, window, st,
                         cap_args(cap));
  return extend_blocks(x, pos, kstart, kr, vr, part_o, part_ml, out, B, L, nh, nkv, hd, S_max, ld, scale * LOG2E,
                       window, st);
}
#endif  // ND_EXTEND_KERNELS_ONLY
