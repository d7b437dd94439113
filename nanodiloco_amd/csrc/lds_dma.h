// LDS-DMA, barrier, wait and transposing-read primitives shared by the gfx950 GEMM and attention kernels.
//
// Every LDS-DMA piece is ONE wave-instruction (64 lanes x 16 B -> 1 KiB of LDS, lane-linear), issued from inline
// asm so hipcc does not track it: otherwise it conservatively waits vmcnt(0) before the first LDS read of the
// OTHER buffer, which serialises the DMA of tile k + 1 with the MFMAs of tile k.  The caller owns the vmcnt wait
// (vmwait<N>()).  M0 (the DMA destination base) is compiler-reserved: every asm that writes it saves and
// restores it inside the same statement.  The one wait state between an m0 write and the LDS-DMA that reads it
// is the s_nop.
#pragma once
#include "common.h"

namespace nd {

typedef __bf16 bfv8 __attribute__((ext_vector_type(8)));
typedef short sv4 __attribute__((ext_vector_type(4)));

// byte address of an LDS object (the m0 / ds_* view of a __shared__ pointer)
template <class T_>
__device__ __forceinline__ uint32_t lds_addr(const T_* p) {
  return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) T_*)p);
}

// V# over [base, base + bytes): lanes whose offset lies past the record count read nothing
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// the same from a 64-bit byte count, clamped to [0, 0x7ffffffe]
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_clamped(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0,
                                           (int)(bytes > 0 ? (bytes < 0x7ffffffe ? bytes : 0x7ffffffe) : 0), 0x00020000);
}

// buffer form: 64 lanes x 16 B from descriptor r at per-lane byte offset voff to LDS [lds, lds + 1 KiB); lanes
// past the descriptor's record count read nothing (tail rows)
__device__ __forceinline__ void dma(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(r), "s"(lds) : "memory");
}
// FLAT-global form: 64-bit uniform base in SGPRs + 32-bit per-lane byte offset (no per-lane 64-bit math, no
// range check): tiles whose rows / columns all exist
__device__ __forceinline__ void gdma(const void* base, uint32_t voff, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds) : "memory");
}

// Four pieces from per-lane byte offsets v0..v3 into LDS lds, lds + ST, lds + 2 ST, lds + 3 ST: m0 is saved /
// restored once per burst and stepped with one s_add per piece (SCC is declared clobbered).
template <uint32_t ST>
__device__ __forceinline__ void gdma4(const void* base, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "s"(lds), "i"(ST)
      : "memory", "scc");
}
template <uint32_t ST>
__device__ __forceinline__ void dma4(__amdgpu_buffer_rsrc_t r, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3,
                                     uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %5, 0 offen lds\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %5, 0 offen lds\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %5, 0 offen lds\n\t"
      "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %4, %5, 0 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(r), "s"(lds), "i"(ST)
      : "memory", "scc");
}

// workgroup barrier the compiler moves nothing across
__device__ __forceinline__ void bar() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}
// counted wait on this wave's own pieces (never a drain of the whole stream unless N == 0)
template <int N> __device__ __forceinline__ void vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }

// ds_read_b64_tr_b16: 4 consecutive rows of one column per lane
__device__ __forceinline__ sv4 tr_read(const bf16_t* lds_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((sv4 __attribute__((address_space(3)))*)(lds_ptr));
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bfv8, a), __builtin_bit_cast(bfv8, b), c, 0, 0, 0);
}

}  // namespace nd
