// Top-k sparse transport of the DiLoCo pseudo-gradient with error feedback (wire format and rules:
// docs/DESIGN.md "Top-k sparse transport").
//
//   nd_pseudograd_topk      acc = (sync - master) + e; per chunk of 4096 elements the k entries with the largest
//                           |acc| go to the wire slot (ascending index), e keeps what was not sent
//   nd_outer_nesterov_topk  per chunk: the W workers' entries are summed, in worker order, into a dense LDS chunk,
//                           then the outer Nesterov update (outer_update.h) runs on every element
//
// Order of the selection: key = the int32 bit pattern of |acc| (31 bits), larger key first, lower index first among
// equal keys -- a total order, so the selected set is a pure function of the inputs (NaN > inf > finite; -0 == +0).
// The selector is a most-significant-digit radix select: four passes (8 + 8 + 8 + 7 bits) over LDS histograms
// narrow the key of the k-th largest entry, one block-wide scan in index order ranks the entries that tie with it,
// and a second one compacts the selected entries.  LDS atomics only count; nothing depends on their order.
//
// One 256-thread workgroup owns one chunk; thread t holds elements 16t .. 16t+15 in registers, so thread order is
// index order and each scan is ONE pass over per-thread counts.  The grid is capped at 2048 workgroups like the
// other flat kernels and strides over the remaining chunks.
//
// A wire slot of nchunks chunks is [uint16 idx[nchunks][k], padded to 16 B][val[nchunks][k], padded to 16 B]
// (val fp32 or bf16).  Unused entries of a chunk with fewer than k elements: idx 0xFFFF, val 0.  The padding bytes
// are never written.
#include "common.h"
#include "outer_update.h"

using namespace nd;

namespace {

constexpr int C = 4096;       // elements per chunk
constexpr int NT = 256;       // threads per workgroup
constexpr int PER = C / NT;   // elements per thread
constexpr int GRID_CAP = 2048;
constexpr unsigned NONE = 0xFFFFu;

__host__ __device__ inline int64_t pad16(int64_t b) { return (b + 15) & ~(int64_t)15; }

unsigned chunk_grid(int64_t nchunks) { return (unsigned)(nchunks > GRID_CAP ? GRID_CAP : (nchunks < 1 ? 1 : nchunks)); }

// Exclusive prefix sum of v over the workgroup in thread order (two barriers; red: NT / 64 ints of LDS).
__device__ __forceinline__ int block_excl_scan(int v, int* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();  // the previous scan's readers are done with red
  if (lane == 63) red[w] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i)
    if (i < w) base += red[i];
  return base + inc - v;
}

template <int VDT>
__global__ void __launch_bounds__(NT) topk_kernel(const float* __restrict__ sync, const float* __restrict__ p,
                                                  float* __restrict__ resid, int64_t n, uint16_t* __restrict__ idx,
                                                  void* __restrict__ val, int k, int64_t nchunks) {
  __shared__ int hist[NT / 64][256];  // one histogram per wave: fewer same-bin collisions
  __shared__ int red[NT / 64];
  __shared__ int pick[2];             // the pass's result: key prefix, entries still to take at that prefix
  const int t = threadIdx.x, w = t >> 6;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t base = ch * C;
    const int m = (int)(n - base < C ? n - base : C);  // real elements of this chunk, >= 1
    const int kk = k < m ? k : m;
    const int e0 = t * PER;
    float x[PER];
    int key[PER];  // -1 past the chunk's end: matches no prefix, ties with nothing
    if (e0 + PER <= m) {
#pragma unroll
      for (int j = 0; j < PER / 4; ++j) {
        const float4 S = *reinterpret_cast<const float4*>(sync + base + e0 + 4 * j);
        const float4 P = *reinterpret_cast<const float4*>(p + base + e0 + 4 * j);
        const float4 E = *reinterpret_cast<const float4*>(resid + base + e0 + 4 * j);
        x[4 * j + 0] = (S.x - P.x) + E.x;
        x[4 * j + 1] = (S.y - P.y) + E.y;
        x[4 * j + 2] = (S.z - P.z) + E.z;
        x[4 * j + 3] = (S.w - P.w) + E.w;
      }
#pragma unroll
      for (int q = 0; q < PER; ++q) key[q] = __float_as_int(x[q]) & 0x7fffffff;
    } else {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const bool in = e0 + q < m;
        x[q] = in ? (sync[base + e0 + q] - p[base + e0 + q]) + resid[base + e0 + q] : 0.f;
        key[q] = in ? (__float_as_int(x[q]) & 0x7fffffff) : -1;
      }
    }

    // ---- the key of the kk-th largest entry, digit by digit
    int prefix = 0, need = kk;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int bits = pass == 3 ? 7 : 8;
      const int sh = pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0;
      const int psh = sh + bits;  // key >> psh: the digits fixed so far (pass 0: the sign, 0 for a real element)
      for (int i = t; i < (NT / 64) * 256; i += NT) (&hist[0][0])[i] = 0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PER; ++q)
        if ((key[q] >> psh) == prefix) atomicAdd(&hist[w][(key[q] >> sh) & ((1 << bits) - 1)], 1);
      __syncthreads();
      const int bin = 255 - t;  // thread order = descending digit: the exclusive scan counts the entries above
      int h = 0;
#pragma unroll
      for (int i = 0; i < NT / 64; ++i) h += hist[i][bin];
      const int above = block_excl_scan(h, red);
      if (above < need && above + h >= need) {  // exactly one thread: need >= 1 entries match the prefix
        pick[0] = (prefix << bits) | bin;
        pick[1] = need - above;
      }
      __syncthreads();
      prefix = pick[0];
      need = pick[1];
    }
    const int T = prefix;  // every key > T is taken, and the first `need` entries with key == T

    // ---- ties in index order, then compaction in index order
    int tc = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) tc += key[q] == T;
    int rank = block_excl_scan(tc, red);
    unsigned sel = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      if (key[q] > T) sel |= 1u << q;
      else if (key[q] == T) {
        if (rank < need) sel |= 1u << q;
        ++rank;
      }
    }
    int pos = block_excl_scan(__popc(sel), red);
    uint16_t* oi = idx + ch * k;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      if ((sel & (1u << q)) && pos < kk) {  // exactly kk are selected; the bound keeps every store inside the k entries
        oi[pos] = (uint16_t)(e0 + q);
        if (VDT == BF16) {
          const bf16_t s = f2bf(x[q]);
          reinterpret_cast<bf16_t*>(val)[ch * k + pos] = s;
          x[q] = x[q] - bf2f(s);
        } else {
          reinterpret_cast<float*>(val)[ch * k + pos] = x[q];
          x[q] = x[q] - x[q];  // 0, or NaN for a non-finite entry
        }
        ++pos;
      }
    }
    for (int i = kk + t; i < k; i += NT) {
      oi[i] = (uint16_t)NONE;
      if (VDT == BF16) reinterpret_cast<bf16_t*>(val)[ch * k + i] = 0;
      else reinterpret_cast<float*>(val)[ch * k + i] = 0.f;
    }
    if (e0 + PER <= m) {
#pragma unroll
      for (int j = 0; j < PER / 4; ++j)
        *reinterpret_cast<float4*>(resid + base + e0 + 4 * j) =
            make_float4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < PER; ++q)
        if (e0 + q < m) resid[base + e0 + q] = x[q];
    }
  }
}

template <int VDT, int SDT>
__global__ void __launch_bounds__(NT) outer_topk_kernel(float* __restrict__ p, float* __restrict__ sync,
                                                        const uint8_t* __restrict__ gath, int nw, int64_t slot_bytes,
                                                        int64_t val_off, int k, float* __restrict__ buf,
                                                        void* __restrict__ sh, int64_t n, int64_t nchunks, float inv_w,
                                                        float lr, float mu, int first) {
  __shared__ __attribute__((aligned(16))) float dense[C];
  const int t = threadIdx.x;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t base = ch * C;
    const int m = (int)(n - base < C ? n - base : C);
    for (int i = t; i < C / 4; i += NT) reinterpret_cast<float4*>(dense)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int r = 0; r < nw; ++r) {  // worker order: deterministic; one worker's indices are distinct
      const uint8_t* slot = gath + r * slot_bytes;
      const uint16_t* ix = reinterpret_cast<const uint16_t*>(slot) + ch * k;
      for (int i = t; i < k; i += NT) {
        const unsigned id = ix[i];
        if (id < (unsigned)m) {  // skips 0xFFFF, and keeps any other index inside the chunk
          const float v = VDT == BF16 ? bf2f(reinterpret_cast<const bf16_t*>(slot + val_off)[ch * k + i])
                                      : reinterpret_cast<const float*>(slot + val_off)[ch * k + i];
          dense[id] = dense[id] + v;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < C / (4 * NT); ++j) {
      const int e = j * 4 * NT + t * 4;
      const int64_t g = base + e;
      if (e + 4 <= m) {
        const float4 D = *reinterpret_cast<const float4*>(dense + e);
        float4 B = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(buf + g);
        float4 S = *reinterpret_cast<const float4*>(sync + g);
        float4 P;
        P.x = outer_update(D.x * inv_w, B.x, S.x, 0.f, false, 0.f, lr, mu, first);
        P.y = outer_update(D.y * inv_w, B.y, S.y, 0.f, false, 0.f, lr, mu, first);
        P.z = outer_update(D.z * inv_w, B.z, S.z, 0.f, false, 0.f, lr, mu, first);
        P.w = outer_update(D.w * inv_w, B.w, S.w, 0.f, false, 0.f, lr, mu, first);
        *reinterpret_cast<float4*>(buf + g) = B;
        *reinterpret_cast<float4*>(sync + g) = S;
        *reinterpret_cast<float4*>(p + g) = P;
        if (SDT == BF16)
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(sh) + g) = make_uint2(pack2(P.x, P.y), pack2(P.z, P.w));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (e + q < m) {
            float b = first ? 0.f : buf[g + q];
            float so = sync[g + q];
            const float np = outer_update(dense[e + q] * inv_w, b, so, 0.f, false, 0.f, lr, mu, first);
            buf[g + q] = b;
            sync[g + q] = so;
            p[g + q] = np;
            if (SDT == BF16) reinterpret_cast<bf16_t*>(sh)[g + q] = f2bf(np);
          }
        }
      }
    }
    __syncthreads();  // the next chunk zeroes `dense`
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// slot: pad16(nchunks * k * 2) + pad16(nchunks * k * sizeof(val)) bytes, nchunks = ceil(n / 4096).  sync / master /
// resid (n fp32 each; resid is rewritten in place) and slot: 16-byte aligned.  vdt: F32 or BF16 values.
ND_API int nd_pseudograd_topk(const float* sync, const float* p, float* resid, int64_t n, void* slot, int k, int vdt,
                              hipStream_t s) {
  if (k < 1 || k > C || n < 0 || (vdt != F32 && vdt != BF16) || !resid || !slot) return (int)hipErrorInvalidValue;
  if (!aligned(sync, 16) || !aligned(p, 16) || !aligned(resid, 16) || !aligned(slot, 16)) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  const int64_t nchunks = (n + C - 1) / C;
  uint16_t* idx = static_cast<uint16_t*>(slot);
  void* val = static_cast<uint8_t*>(slot) + pad16(nchunks * k * 2);
  if (vdt == BF16) hipLaunchKernelGGL(topk_kernel<BF16>, dim3(chunk_grid(nchunks)), dim3(NT), 0, s, sync, p, resid, n, idx, val, k, nchunks);
  else hipLaunchKernelGGL(topk_kernel<F32>, dim3(chunk_grid(nchunks)), dim3(NT), 0, s, sync, p, resid, n, idx, val, k, nchunks);
  ND_LAUNCH_CHECK();
}

// gath: nw slots of the layout above, back to back, in worker order.  p / sync / buf: 16-byte aligned; sh (bf16):
// 8-byte aligned; gath: 16-byte aligned.
ND_API int nd_outer_nesterov_topk(float* p, float* sync, const void* gath, int nw, int k, int vdt, float* buf, void* sh,
                                  int shdt, int64_t n, float inv_w, float lr, float mu, int first, hipStream_t s) {
  if (k < 1 || k > C || n < 0 || nw < 1 || (vdt != F32 && vdt != BF16) || !gath) return (int)hipErrorInvalidValue;
  if (!aligned(p, 16) || !aligned(sync, 16) || !aligned(buf, 16) || !aligned(gath, 16) || !aligned(sh, 8))
    return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  const int64_t nchunks = (n + C - 1) / C;
  const int64_t val_off = pad16(nchunks * k * 2);
  const int64_t slot_bytes = val_off + pad16(nchunks * k * (vdt == BF16 ? 2 : 4));
  const uint8_t* g = static_cast<const uint8_t*>(gath);
  const unsigned grid = chunk_grid(nchunks);
  const bool bsh = sh && shdt == BF16;
#define ND_OT(V, S) hipLaunchKernelGGL((outer_topk_kernel<V, S>), dim3(grid), dim3(NT), 0, s, p, sync, g, nw, slot_bytes, val_off, k, buf, sh, n, nchunks, inv_w, lr, mu, first)
  if (vdt == BF16) { if (bsh) ND_OT(BF16, BF16); else ND_OT(BF16, F32); }
  else { if (bsh) ND_OT(F32, BF16); else ND_OT(F32, F32); }
#undef ND_OT
  ND_LAUNCH_CHECK();
}
