// rtdm_pk16.h -- what the packed kernels share (k_lrcheck.hip, k_speckle.hip, and through rtdm_sgm.h the StereoSGBM units):
// eight int16 columns as one 16-byte value, packed 16-bit arithmetic on two values per dword -- the only copy of it --
// and LDS accesses by byte address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtdm {

struct alignas(16) Short8 { int16_t v[8]; };

typedef short lr_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short lr_u2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint32_t lr_lds_u32;
__device__ __forceinline__ lr_s2 lr_s(uint32_t v) { return __builtin_bit_cast(lr_s2, v); }
__device__ __forceinline__ lr_u2 lr_u(uint32_t v) { return __builtin_bit_cast(lr_u2, v); }
__device__ __forceinline__ uint32_t lr_w(lr_s2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t lr_w(lr_u2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) { return lr_w(lr_u(a) + lr_u(b)); }
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return lr_w(lr_u(a) - lr_u(b)); }
__device__ __forceinline__ uint32_t pk_subsat_u(uint32_t a, uint32_t b) { return lr_w(__builtin_elementwise_sub_sat(lr_u(a), lr_u(b))); }
__device__ __forceinline__ uint32_t pk_addsat_u(uint32_t a, uint32_t b) { return lr_w(__builtin_elementwise_add_sat(lr_u(a), lr_u(b))); }
__device__ __forceinline__ uint32_t pk_min_u(uint32_t a, uint32_t b) { return lr_w(__builtin_elementwise_min(lr_u(a), lr_u(b))); }
__device__ __forceinline__ uint32_t pk_max_u(uint32_t a, uint32_t b) { return lr_w(__builtin_elementwise_max(lr_u(a), lr_u(b))); }
__device__ __forceinline__ uint32_t pk_max_i(uint32_t a, uint32_t b) { return lr_w(__builtin_elementwise_max(lr_s(a), lr_s(b))); }
template <int N> __device__ __forceinline__ uint32_t pk_ashr(uint32_t a) { return lr_w(lr_s(a) >> (short)N); }
template <int N> __device__ __forceinline__ uint32_t pk_shl(uint32_t a) { return lr_w(lr_u(a) << (unsigned short)N); }
// 1 in every half of x that is zero, else 0 -- as ONE saturating packed subtraction (written as asm: from min(x, 1) or a
// compare the compiler builds two v_cmp, two v_cndmask and a v_perm)
__device__ __forceinline__ uint32_t pk_is_zero(uint32_t x)
{ uint32_t r; asm("v_pk_sub_u16 %0, 1, %1 op_sel_hi:[0,1] clamp" : "=v"(r) : "v"(x)); return r; }
__device__ __forceinline__ uint32_t lr_bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }   // mask ? a : b (v_bfi_b32)
__device__ __forceinline__ void lr_lds_min(uint32_t addr, uint32_t v)
{ __hip_atomic_fetch_min((lr_lds_u32*)(uintptr_t)addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t lr_lds_ld(uint32_t addr) { return *(const lr_lds_u32*)(uintptr_t)addr; }
// Barrier for threads that talk through LDS only: waits for the wave's LDS operations, NOT for its global loads and stores
// (__syncthreads() is a workgroup-scope fence + s_barrier: s_waitcnt vmcnt(0) -- every barrier behind the row's write-back
// would wait for that store to reach memory, and a trip of k_lrcheck_pk is a chain of four barriers).
__device__ __forceinline__ void lr_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// eight flags, one per 16-bit half of h[0..3] (each half 0 or 1), as bits 0..7 in column order
__device__ __forceinline__ unsigned lr_bits8(const uint32_t (&h)[4])
{
    const uint32_t g0 = __builtin_amdgcn_perm(h[1], h[0], 0x06040200u), g1 = __builtin_amdgcn_perm(h[3], h[2], 0x06040200u);
    return __builtin_amdgcn_udot4(g1, 0x80402010u, __builtin_amdgcn_udot4(g0, 0x08040201u, 0u, false), false);
}

}  // namespace rtdm
