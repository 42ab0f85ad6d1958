// A dense row of C <= 1024 channels (C a multiple of 4) in the registers of one 64-lane wavefront: NV float4 per lane,
// lane l holds channels 4 (l + 64 i) .. + 3 for i < NV; channels >= C are held as zeros.  Shared by the row kernels
// (rowln.h and its users, rmsnorm.hip, faformer_ew.hip's row dots).
#pragma once
#include <type_traits>

#include "common.h"

namespace {

template <int NV>
struct Row {
    float4 v[NV];
};

// row r of the dense [., C] matrix at p (16-byte aligned rows); a caller that holds the row's address passes it with r = 0
template <int NV>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int64_t r, int C, int lane, Row<NV>& x) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        x.v[i] = (c < C) ? *reinterpret_cast<const float4*>(p + r * C + c) : f4_zero();
    }
}

// host side: f(std::integral_constant<int, NV>) with the smallest NV in {1, 2, 4} that holds a row of C channels
template <typename F>
int dispatch_nv(int C, F&& f) {
    if (C <= 256) return f(std::integral_constant<int, 1>{});
    if (C <= 512) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}

}  // namespace
