// chaindp_lanes.h -- what the part-wave DP kernel (chaindp_twin.hip: two units per wave) is written with, and the prepass borrows: raw
// LDS access by byte address, loads through the scalar cache, lane masks straight from vector compares.  gfx950 only.
#ifndef CHAINDP_LANES_H
#define CHAINDP_LANES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chaindp {

#if defined(__HIP_DEVICE_COMPILE__)
#define TW_LDS(T, a) ((__attribute__((address_space(3))) T*)(a))
#else
#define TW_LDS(T, a) ((T*)(uintptr_t)(a))          /* host pass of the single-source compile; never executed */
#endif
// unit records and their UnitAux are read through the scalar cache: a load from the constant address space with a wave-uniform
// address is an s_load (the arrays are written by the prepass, never by this kernel)
#if defined(__HIP_DEVICE_COMPILE__)
#define TW_CONST(T, p) ((const __attribute__((address_space(4))) T*)(uintptr_t)(p))
#else
#define TW_CONST(T, p) ((const T*)(p))
#endif
typedef uint32_t tw_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t tw_u32x4 __attribute__((ext_vector_type(4)));

// The kernel's argument struct where it is used, not where the kernel starts: a pointer to the kernel-argument segment (the struct
// is the kernel's only parameter: byte 0 of the segment), so that a field is one s_load through the scalar cache at its point of
// use.  The empty asm hides where the pointer comes from: the compiler can neither hoist these loads above the pass loops nor keep
// the by-value struct's fields in scalar registers through them -- it spilled those into vector lanes and took them back a
// sixteen-register tuple at a time, a v_readlane each.  Take a new one (TW_KARGS) in every rarely run region.
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> __device__ __forceinline__ const __attribute__((address_space(4))) T *tw_kargs(const T &)
{
	const __attribute__((address_space(4))) T *k = (const __attribute__((address_space(4))) T*)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(k));
	return k;
}
#define TW_KARGS(g) tw_kargs(g)
// element of type T at byte `off` (32 bits, per lane, unsigned) behind the wave-uniform global pointer p: the scalar base + vector
// offset form of the global instructions -- no 64-bit address arithmetic in vector registers
#define TW_AT(T, p, off) (*(__attribute__((address_space(1))) T*)((__attribute__((address_space(1))) char*)(p) + (uint32_t)(off)))
#else
#define TW_KARGS(g) (&(g))
#define TW_AT(T, p, off) (*(T*)((char*)(p) + (uint32_t)(off)))
#endif
// atomicMin (device scope, result unused) on an element addressed by TW_AT
template <class P> __device__ __forceinline__ void tw_atomic_min(P *p, int v)
{
	(void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ tw_u32x2 tw_ld64(uint32_t a) { return *TW_LDS(const tw_u32x2, a); }
__device__ __forceinline__ int tw_ld32(uint32_t a) { return *TW_LDS(const int, a); }
__device__ __forceinline__ int tw_ld_i8(uint32_t a) { return (int)*TW_LDS(const signed char, a); }
__device__ __forceinline__ int tw_ld_u8(uint32_t a) { return (int)*TW_LDS(const unsigned char, a); }
__device__ __forceinline__ void tw_st64(uint32_t a, uint32_t x, uint32_t y) { tw_u32x2 t; t.x = x; t.y = y; *TW_LDS(tw_u32x2, a) = t; }
__device__ __forceinline__ void tw_st32(uint32_t a, int v) { *TW_LDS(int, a) = v; }
__device__ __forceinline__ void tw_st8(uint32_t a, int v) { *TW_LDS(signed char, a) = (signed char)v; }

// keeps a value in a vector register: the compiler would otherwise hold wave-uniform values in SGPRs and feed them
// to VALU instructions as scalar operands, which halves their issue rate
#if defined(__HIP_DEVICE_COMPILE__)
#define TW_VREG(x) asm volatile("" : "+v"(x))
#else
#define TW_VREG(x) ((void)(x))
#endif

// hides how a vector value was computed, so that the compiler does not fold what follows into a three-operand instruction (which
// issues at half rate); unlike TW_VREG it does not pin the value's place in the schedule
#if defined(__HIP_DEVICE_COMPILE__)
#define TW_OPAQUE(x) asm("" : "+v"(x))
#else
#define TW_OPAQUE(x) ((void)(x))
#endif

// a lane mask is wave-uniform by construction; where the compiler's divergence analysis loses track of that (values merged
// behind loops) this keeps it in scalar registers (folds away when it already is)
#define TW_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))

// |a - b| + c in one instruction
__device__ __forceinline__ uint32_t tw_sad(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("v_sad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
#endif
	return d;
}

// |a - b| in one instruction
__device__ __forceinline__ uint32_t tw_absdiff(uint32_t a, uint32_t b)
{
	uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("v_sad_u32 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
#endif
	return d;
}

// b - a - 1 in one instruction ((a ^ ~0) + b)
__device__ __forceinline__ uint32_t tw_sub_m1(uint32_t b, uint32_t a)
{
	uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("v_xad_u32 %0, %1, -1, %2" : "=v"(d) : "v"(a), "v"(b));
#endif
	return d;
}

// lane masks straight from a vector compare (v_cmp_*_e64 into an SGPR pair, no bool in between)
#define TW_ULT(a, b) __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 36)
#define TW_EQ(a, b)  __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 32)
#define TW_SGT(a, b) __builtin_amdgcn_sicmp((int)(a), (int)(b), 38)
#define TW_SGE(a, b) __builtin_amdgcn_sicmp((int)(a), (int)(b), 39)
#define TW_SEL(m, a, b) (__builtin_amdgcn_inverse_ballot_w64(m) ? (a) : (b))

} // namespace chaindp
#endif
