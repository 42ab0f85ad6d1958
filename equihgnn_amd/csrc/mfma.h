// Register vector types of the matrix instructions, the fp32 16x16x4 product and the bf16 16x16x16 product, defined ONCE.  (The
// wide bf16 products, v_mfma_f32_32x32x16_bf16 / 16x16x32, are written out where they are used; the order of the x3 / x6 plane
// products is always the kernel's.)
#pragma once
#include "common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// v_mfma_f32_16x16x4f32: c += A B with A [16 x 4], B [4 x 16].  Lane (r, q) = (lane & 15, lane >> 4) passes a = A[r][q],
// b = B[q][r] and holds c[g] = C[4 q + g][r].  Every lane must be active.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// v_mfma_f32_16x16x16_bf16: c += A B with A [16 x 16], B [16 x 16] in bf16, fp32 accumulation.  Lane (r, q) passes four
// CONSECUTIVE K values, a = A[r][4 q .. 4 q + 3] and b = B[4 q .. 4 q + 3][r], packed two per register (the lower index in the low
// half: the packing of bf16x3.h's planes) and holds c[g] = C[4 q + g][r] -- the accumulator map of mfma16.  Every lane must be active.
__device__ __forceinline__ f32x4 mfma16_bf16(uint2 a, uint2 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(bf16x4, a), __builtin_bit_cast(bf16x4, b), c, 0, 0, 0);
}

}  // namespace
