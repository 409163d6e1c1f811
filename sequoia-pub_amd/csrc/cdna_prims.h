// Leaf helpers of the MFMA kernels (gfx950): buffer descriptors, the 16-byte LDS-DMA load, LDS accesses, counted waits, the bf16
// MFMA and the XCD tile walk -- each once.  A new kernel file includes this header instead of pasting the block.  Tile loops,
// ring bookkeeping, swizzles and epilogues stay in their kernel files.
#pragma once
#include "sq_common.h"
#include "tile_walk.h"      // sq_xcd_tile(block, n_tiles): each XCD walks a contiguous run of tiles

typedef __attribute__((address_space(3))) void lds_void;

// A voffset with this bit set lies beyond every descriptor's extent (at most 0x7fffffff bytes, sq_desc_extent): the load is
// redirected out of range and lands in LDS as zeros, the store is dropped.
constexpr uint32_t SQ_OOB = 0x80000000u;
// Word 3 of a raw buffer descriptor: 32-bit data format, no swizzle, no stride -- the range check is on the plain byte offset.
constexpr int SQ_RSRC_FLAGS = 0x00020000;

// Descriptor over `bytes` bytes at p (wave-uniform values only).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sq_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, SQ_RSRC_FLAGS);
}

// 16 B per lane, HBM/L2 -> LDS without a VGPR round trip.  LDS destination = lds_base + lane*16
// (lane-linear); the source offset is per lane.  Kept in a non-template helper: the host pass of a
// kernel TEMPLATE that names this builtin directly silently drops the kernel's launch stub.
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, char* lds_base, uint32_t voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_base, 16, voffset, soffset, 0, 0);
}
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, char* lds_base, uint32_t voffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_base, 16, voffset, 0, 0, 0);
}
__device__ __forceinline__ void glds16_nt(__amdgpu_buffer_rsrc_t rsrc, char* lds_base, uint32_t voffset) {      // streaming (read-once) data
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_base, 16, voffset, 0, 0, 2);
}

__device__ __forceinline__ u32x4 lds128(const char* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x2 lds64(const char* p) { return *reinterpret_cast<const u32x2*>(p); }
__device__ __forceinline__ void st_lds64(char* p, u32x2 v) { *reinterpret_cast<u32x2*>(p) = v; }

// waits until at most N vector-memory operations (LDS-DMA loads among them) are outstanding
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// (wait_vm_n(int), the run-time count, stays in chain_x3.hip and chain_x3w.hip: their two bodies differ.)

// v_mfma_f32_32x32x16_bf16, fp32 accumulate: 8 bf16 per lane and operand, packed in four dwords
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, f32x16 acc) {
    union { u32x4 u; bf16x8 h; } ua, ub;
    ua.u = a; ub.u = b;
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ua.h, ub.h, acc, 0, 0, 0);
}
