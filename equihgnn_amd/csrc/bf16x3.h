// The exact three-way bf16 split of an fp32 number (a = a0 + a1 + a2, every plane a truncation: gemm_x6.hip's header has the
// derivation) shared by the x6 GEMM, the panel kernels and the weight packer: ONE definition, so that a weight split ahead of
// time (hg_panel_pack) and an activation split inside a kernel follow the same arithmetic.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t fbits(float x) { return __float_as_uint(x); }

// (x0, x1) -> their three bf16 planes, packed as bf16x2 (x0 in the low half)
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
#ifdef GX_ABLATE_SPLIT
    p0 = fbits(x0); p1 = fbits(x1); p2 = fbits(x0) ^ fbits(x1);
    return;
#endif
    const uint32_t u0 = fbits(x0), u1 = fbits(x1);
    p0 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    const uint32_t v0 = fbits(r0), v1 = fbits(r1);
    p1 = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    p2 = __builtin_amdgcn_perm(fbits(s1), fbits(s0), 0x07060302u);
}

// The same split cut short, for kernels that split in registers and read fewer planes (the reduced matmul precision modes of the
// batched weight gradients): only the planes a mode reads are formed.  Plane for plane the bits of split_pair.
// (x0, x1) -> their first two planes
__device__ __forceinline__ void split_pair2(float x0, float x1, uint32_t& p0, uint32_t& p1) {
#ifdef GX_ABLATE_SPLIT
    p0 = fbits(x0); p1 = fbits(x1);
    return;
#endif
    const uint32_t u0 = fbits(x0), u1 = fbits(x1);
    p0 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    p1 = __builtin_amdgcn_perm(fbits(r1), fbits(r0), 0x07060302u);
}

// (x0, x1) -> plane 0 alone: a truncation, the two high halves packed into one register (one instruction per pair)
__device__ __forceinline__ uint32_t split_pair1(float x0, float x1) {
    return __builtin_amdgcn_perm(fbits(x1), fbits(x0), 0x07060302u);
}

// (x0, x1) -> their first PL planes through the three functions above; the planes past PL are set to zero and fall away
template <int PL>
__device__ __forceinline__ void split_pair_n(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
    static_assert(PL >= 1 && PL <= 3, "one, two or three planes");
    if constexpr (PL == 3) {
        split_pair(x0, x1, p0, p1, p2);
    } else if constexpr (PL == 2) {
        split_pair2(x0, x1, p0, p1);
        p2 = 0u;
    } else {
        p0 = split_pair1(x0, x1);
        p1 = p2 = 0u;
    }
}

// Four values -> their first PL <= 2 planes, each plane as the two registers a K = 16 bf16 MFMA reads per lane (mfma.h, mfma16_bf16)
struct Planes4 {
    uint2 p0, p1;   // p1 is zero, and unused, with one plane
};
template <int PL>
__device__ __forceinline__ Planes4 split_quad(float x0, float x1, float x2, float x3) {
    static_assert(PL == 1 || PL == 2, "one or two planes");
    Planes4 o;
    uint32_t none;
    split_pair_n<PL>(x0, x1, o.p0.x, o.p1.x, none);
    split_pair_n<PL>(x2, x3, o.p0.y, o.p1.y, none);
    return o;
}

}  // namespace
