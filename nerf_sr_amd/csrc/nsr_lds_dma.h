// LDS-DMA and LDS access primitives of the matrix kernels: every inline-asm VMEM statement of the project (global -> LDS
// pieces, the panel stores), the counted wait and the lane offsets that go with them, and LDS access by 32-bit byte address.  The only file
// of csrc/ that names the LDS address space or a global_load_lds / global_store in an asm string
// (tests/test_lds_primitives_cpu.py); build.isa_contract checks the two rules below on the compiled listings.
#pragma once
#include "nsr_common.h"

namespace nsr {
namespace dma {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef __fp16 fp4 __attribute__((__vector_size__(4 * sizeof(__fp16))));   // what ds_read_tr16 takes

__device__ __forceinline__ h8 as_h8(const u32x4& v) { return __builtin_bit_cast(h8, v); }

// ---- LDS by byte address ---------------------------------------------------------------------------------------------------
// LDS byte address (32-bit) of a __shared__ object
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)((const __attribute__((address_space(3))) char*)p);
}
// 16-byte vector view of an LDS byte address
__device__ __forceinline__ const u32x4* lds_vec(unsigned byte_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (const u32x4*)(const __attribute__((address_space(3))) u32x4*)(size_t)byte_addr;
#else
  (void)byte_addr;
  return nullptr;   // host pass of the single-source compile; never executed
#endif
}
// one ds_read / ds_write of a T
template <class T>
__device__ __forceinline__ T lds_load(unsigned byte_addr) {
  return *(const __attribute__((address_space(3))) T*)(size_t)byte_addr;
}
template <class T>
__device__ __forceinline__ void lds_store(unsigned byte_addr, T v) {
  *(__attribute__((address_space(3))) T*)(size_t)byte_addr = v;
}
// the transposing LDS read: lane l of a 16-lane group receives, of the sixteen 8-byte pieces the group's lanes address,
// half (l & 3) of the pieces of lanes (l >> 2), 4 + (l >> 2), 8 + (l >> 2), 12 + (l >> 2) -- i.e. with lane 4 q + p
// addressing row q, columns 4 p .. 4 p + 3 of a 4 x 16 block, lane i receives column i of the four rows
__device__ __forceinline__ h4 tr16(unsigned byte_addr) {
  return __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp4*)(size_t)byte_addr));
}

// ---- VMEM from inline asm --------------------------------------------------------------------------------------------------
// Weight DMA (global -> LDS, 64 lanes x 16 B) issued from inline asm: wave-uniform 64-bit base in SGPRs
// + one 32-bit lane offset.  Why not __builtin_amdgcn_global_load_lds: hipcc's waitcnt insertion treats
// an in-flight LDS-DMA as a FLAT-like event and from then on waits lgkmcnt(0) — i.e. for the fragment
// loads issued two instructions earlier — before every MFMA group.  The asm form is invisible to that
// pass; its completion is waited for by hand (dma_drain) right before the barrier that publishes the
// chunk.  OFF (0..3072) is added to BOTH the global and the LDS address, so one (base, M0) pair serves
// four consecutive 1 KiB pieces.  M0 is written in the same statement that consumes it (hipcc reserves
// M0 and uses it nowhere else in these kernels).
// The base is copied into a scratch SGPR pair INSIDE the statement: when hipcc has spilled the descriptor to VGPR lanes
// it restores it with v_readlane right in front of the statement, and a VMEM instruction that reads a VALU-written SGPR
// needs five wait states which hipcc's hazard pass cannot see through inline asm (round 4: a persistent-loop build read
// a stale pair and faulted).  An SALU read is interlocked, and the copy doubles as the wait state after the M0 write.
// M0 is a reserved register for hipcc (it never allocates it: naming it in a clobber list is a warning), so the pieces
// 4q+1 .. 4q+3 of a 4 KiB group reuse the M0 piece 4q wrote (glds16_keep_asm).
// The same two rules hold for every statement below: M0 is written only here, and a VMEM instruction reads the in-statement
// copy of its base, never the compiler's own SGPR pair.
template <int OFF>
__device__ __forceinline__ void glds16_asm(const char* base_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  unsigned long long tmp;
  asm volatile(
      "s_mov_b32 m0, %3\n\t"
      "s_mov_b64 %0, %2\n\t"
      "global_load_lds_dwordx4 %1, %0 offset:%4"
      : "=&s"(tmp)
      : "v"(lane_off), "s"(base_uniform), "s"(lds_dst_uniform), "i"(OFF)
      : "memory");
}
// a further piece of the 4 KiB group whose first piece set M0 (same base, same M0)
template <int OFF>
__device__ __forceinline__ void glds16_keep_asm(const char* base_uniform, unsigned lane_off) {
  unsigned long long tmp;
  asm volatile(
      "s_mov_b64 %0, %2\n\t"
      "global_load_lds_dwordx4 %1, %0 offset:%3"
      : "=&s"(tmp)
      : "v"(lane_off), "s"(base_uniform), "i"(OFF)
      : "memory");
}
// the dword form: 64 lanes x 4 B, lane-linear, global -> LDS
__device__ __forceinline__ void glds4_asm(const void* base_uniform, unsigned lane_off, unsigned lds_dst_uniform) {
  unsigned long long tmp;
  asm volatile(
      "s_mov_b32 m0, %3\n\t"
      "s_mov_b64 %0, %2\n\t"
      "global_load_lds_dword %1, %0"
      : "=&s"(tmp)
      : "v"(lane_off), "s"(base_uniform), "s"(lds_dst_uniform)
      : "memory");
}
// Lane offsets made at the issue site.  volatile: the value is a constant of the whole kernel and hipcc would keep it in a
// register of its own from the prologue on; made here it lives from its group's first piece to its last.
// lane_off + ADD (the 4 KiB group ADD / 4096 of a share)
template <int ADD>
__device__ __forceinline__ unsigned lane_offset_group(unsigned lane_off) {
  unsigned r;
  asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "n"(ADD), "v"(lane_off));
  return r;
}
// lane_off / 4 + add_uniform: the dword form's lane offset (lane * 4) from the 16-byte one, plus a wave-uniform byte offset
__device__ __forceinline__ unsigned lane_offset_dword(unsigned lane_off, unsigned add_uniform) {
  unsigned r;
  asm volatile(
      "v_lshrrev_b32 %0, 2, %1\n\t"
      "v_add_u32 %0, %2, %0"
      : "=&v"(r)
      : "v"(lane_off), "s"(add_uniform));
  return r;
}
// 16 B per lane to base + voff + OFF, non-temporal; 4 B per lane to base + voff (the training panels' two stores)
template <int OFF>
__device__ __forceinline__ void gstore16_nt_asm(const u32x4& v, const void* base_uniform, unsigned voff) {
  unsigned long long tmp;
  asm volatile("s_mov_b64 %0, %3\n\tglobal_store_dwordx4 %1, %2, %0 offset:%4 nt" : "=&s"(tmp) : "v"(voff), "v"(v), "s"(base_uniform), "n"(OFF) : "memory");
}
__device__ __forceinline__ void gstore4_asm(unsigned v, const void* base_uniform, unsigned voff) {
  unsigned long long tmp;
  asm volatile("s_mov_b64 %0, %3\n\tglobal_store_dword %1, %2, %0" : "=&s"(tmp) : "v"(voff), "v"(v), "s"(base_uniform) : "memory");
}

// vector memory operations complete in issue order: wait with N younger operations (loads / stores issued AFTER the last
// DMA piece that must have landed) allowed to stay in flight
template <int N = 0>
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory"); }
__device__ __forceinline__ void dma_drain() { dma_wait<0>(); }

}  // namespace dma
}  // namespace nsr
