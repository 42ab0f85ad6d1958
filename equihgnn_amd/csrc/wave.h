// Cross-lane primitives of a 64-lane wavefront, defined ONCE: a reduction fixes the order in which its partial sums
// are added, so two kernels give bit-identical sums only while they share the definition.  Every lane of the wavefront
// must be active in all of them (DPP and readlane read the registers of inactive lanes as they are).
#pragma once
#include "common.h"

namespace {

// v of the lane that the DPP control CTRL selects (all rows and banks enabled)
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over the 16 lanes of a DPP row, in every lane of the row, on the DPP network (no LDS round trips): two quad
// butterflies, (0+1)+(2+3), then the four quad totals by rotations, (q + q-1) + (q-2 + q-3).
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_move<0x124>(v);  // row_ror:4
    v += dpp_move<0x128>(v);  // row_ror:8
    return v;
}

// v of lane j in every lane, through a scalar read (no LDS traffic); j: compile-time constant after unrolling
__device__ __forceinline__ float bcast(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));  // readlane moves 32-bit integers
}

// Wavefront all-reduce: row16_sum, then the four row totals as (row 0 + row 1) + (row 2 + row 3).
__device__ __forceinline__ float wave_sum(float v) {
    const int bits = __float_as_int(row16_sum(v));  // readlane moves 32-bit integers
    return (__int_as_float(__builtin_amdgcn_readlane(bits, 0)) + __int_as_float(__builtin_amdgcn_readlane(bits, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(bits, 32)) + __int_as_float(__builtin_amdgcn_readlane(bits, 48)));
}
__device__ __forceinline__ void wave_sum2(float& a, float& b) {
    a = wave_sum(a);
    b = wave_sum(b);
}

// Wavefront maximum in every lane: xor butterfly over lane distances 32, 16, .. 1 (fmaxf: order-free but for NaN)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

}  // namespace
