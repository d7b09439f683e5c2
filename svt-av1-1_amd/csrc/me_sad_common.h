// svt-av1-1_amd/csrc/me_sad_common.h -- small device helpers shared by the packed-SAD search kernels (me_fullpel_impl.h,
// me_fullpel209_impl.h, me_hme_impl.h, me_sadloop.hip): dword pairs for v_qsad_pk_u16_u8, (sad << k | index) key minima, wave minima,
// loads that need a fixed shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svthip {

__device__ __forceinline__ uint64_t pack64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// one ds_read_b128 that stays one: where only dword PAIRS of the result are used the compiler otherwise splits the 16-byte load into
// 8-byte pieces and re-merges them as ds_read2_b64 (twice the LDS cycles, 32-bank rule)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 lds_read_b128(const uint8_t* p)
{
    // the volatile access loses the address space that the compiler infers for smem, so it is named
    const u32x4_t v = *(const volatile __attribute__((address_space(3))) u32x4_t*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// global loads at byte alignment (one global_load_dword / _dwordx4 each; this target needs no alignment for them)
struct __attribute__((packed, aligned(1))) unaligned_u32 { uint32_t v; };
struct __attribute__((packed, aligned(1))) unaligned_u32x4 { uint32_t v[4]; };

__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// keys for the four positions of a quad from packed u16 SADs (lo: slots 0,1  hi: slots 2,3)
__device__ __forceinline__ uint32_t track4(uint32_t best, uint64_t acc, const uint32_t* idx, uint32_t himask)
{
    const uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
    uint32_t k0 = (lo << 16) | idx[0];
    uint32_t k1 = (lo & himask) | idx[1];
    uint32_t k2 = (hi << 16) | idx[2];
    uint32_t k3 = (hi & himask) | idx[3];
    best = min3u(best, k0, k1);
    best = min3u(best, k2, k3);
    return best;
}

__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the same through the compiler's own packed minimum: it knows the instruction, so it schedules a tree of them without the s_nop that
// follows every inline-asm result used by the next instruction
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min_u16_tree(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        uint32_t o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        unsigned long long o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t mv_word(int x, int y)
{
    // (uint16)(4*y) << 16 | (uint16)(4*x), Codec/EbMotionEstimation.c:1389-1391
    return ((uint32_t)(uint16_t)(y * 4) << 16) | (uint32_t)(uint16_t)(x * 4);
}

}  // namespace svthip
