// Row-wise LayerNorm arithmetic shared by the aggregation kernels (incidence.hip) and the panel GEMM kernels
// (panel.hip): one 64-lane wavefront per row, a row of C <= 1024 channels is NV float4 per lane (lane l holds channels
// 4 (l + 64 i) .. + 3).  ONE definition, so that a LayerNorm fused into a GEMM prologue / epilogue gives bit-identical
// results to the stand-alone row kernels (mlp.py:91-99: Linear -> ReLU -> LayerNorm).  The row itself is row.h's Row<NV>, the
// sums are wave.h's wave_sum.
#pragma once
#include "common.h"
#include "drop_hash.h"
#include "row.h"
#include "wave.h"

namespace {

// h = relu(u + w) (RELU) or u + w; returns xhat in `x`, rstd in *rstd, relu mask in `pos` (bit per comp)
template <int NV, bool RELU = true>
__device__ __forceinline__ void norm_pair(const Row<NV>& u, const Row<NV>& w, int C, int lane, float inv_c,
                                          float eps, Row<NV>& x, unsigned& pos, float* rstd) {
    float s = 0.f;
    pos = 0u;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float4 h = make_float4(u.v[i].x + w.v[i].x, u.v[i].y + w.v[i].y, u.v[i].z + w.v[i].z, u.v[i].w + w.v[i].w);
        if (RELU) {
            pos |= ((h.x > 0.f) ? 1u : 0u) << (4 * i) | ((h.y > 0.f) ? 2u : 0u) << (4 * i) |
                   ((h.z > 0.f) ? 4u : 0u) << (4 * i) | ((h.w > 0.f) ? 8u : 0u) << (4 * i);
            h.x = fmaxf(h.x, 0.f); h.y = fmaxf(h.y, 0.f); h.z = fmaxf(h.z, 0.f); h.w = fmaxf(h.w, 0.f);
        } else {
            pos |= 15u << (4 * i);
        }
        x.v[i] = h;
        s += (h.x + h.y) + (h.z + h.w);
    }
    const float mu = wave_sum(s) * inv_c;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        float4 d = x.v[i];
        if (c < C) { d.x -= mu; d.y -= mu; d.z -= mu; d.w -= mu; }
        x.v[i] = d;
        ss += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
    const float r = 1.0f / sqrtf(wave_sum(ss) * inv_c + eps);
    *rstd = r;
#pragma unroll
    for (int i = 0; i < NV; ++i) { x.v[i].x *= r; x.v[i].y *= r; x.v[i].z *= r; x.v[i].w *= r; }
}

// the workgroup's NW wavefronts' copies of one accumulator row -> one slab row [C], summed in wavefront order
// (s_red: NW * 64 float4 of LDS)
template <int NV, int NW>
__device__ __forceinline__ void slab_store(float4* s_red, float* __restrict__ sl, int C, const Row<NV>& a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        s_red[threadIdx.x] = a.v[i];
        __syncthreads();
        if (wave == 0) {
            float4 t = s_red[lane];
            for (int w2 = 1; w2 < NW; ++w2) f4_add(t, s_red[w2 * 64 + lane]);
            const int c = (lane + 64 * i) * 4;
            if (c < C) *reinterpret_cast<float4*>(sl + c) = t;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Training dropout behind the LayerNorm (mlp.py:91-99: Linear -> ReLU -> LayerNorm -> dropout) as a template flag of the
// row kernels.  keep is 0 or 1 / (1 - p): the hash of (seed in device memory, element index) of drop_hash.h.  No mask is
// stored: a backward recomputes the decisions.
// ------------------------------------------------------------------------------------------------
// The LayerNorm's eps and, with DROP, the dropout arguments: ONE kernel argument, in the place of the `float eps` of a kernel
// without the flag.  LnArgs<false> is that float and nothing else, so the p = 0 instantiation has the argument block and
// the instruction stream of such a kernel.
template <bool DROP>
struct LnArgs {
    float eps;
};
template <>
struct LnArgs<true> {
    float eps;
    uint32_t threshold;     // drop_threshold(p)
    float inv_keep;         // drop_inv_keep(p)
    const int64_t* seed;
    const int* perm;        // k_inc_fwd_col only: the positions of the (rowptr, col) CSR's entries in ia / ib
};
// host side
template <bool DROP>
LnArgs<DROP> ln_args(float eps, float p, const int64_t* seed, const int* perm = nullptr) {
    if constexpr (DROP) return {eps, drop_threshold(p), drop_inv_keep(p), seed, perm};
    else return {eps};
}

// what a thread derives from them once: the key of the hash
template <bool DROP>
struct Keep {
    __device__ explicit Keep(const LnArgs<DROP>&) {}
};
template <>
struct Keep<true> {
    DropKey key;
    uint32_t threshold;
    float inv_keep;
    __device__ explicit Keep(const LnArgs<true>& d)
        : key(drop_key(d.threshold ? (uint64_t)*d.seed : 0)), threshold(d.threshold), inv_keep(d.inv_keep) {}
};

// keep-scales of row `row` of a [., C] tensor (elements row * C + c): the lane's float4 group i ...
__device__ __forceinline__ float4 keep_group(const Keep<true>& kp, int64_t row, int C, int lane, int i) {
    const uint64_t base = (uint64_t)row * (uint64_t)C;      // C % 4 == 0: every float4 group starts at a multiple of 4
    float4 k = make_float4(1.f, 1.f, 1.f, 1.f);
    keep_scale4(kp.key, base + (uint64_t)((lane + 64 * i) * 4), kp.threshold, kp.inv_keep, k);
    return k;
}
// ... and the whole row, in the Row layout
template <int NV>
__device__ __forceinline__ void keep_row(const Keep<true>& kp, int64_t row, int C, int lane, Row<NV>& k) {
#pragma unroll
    for (int i = 0; i < NV; ++i) k.v[i] = keep_group(kp, row, C, lane, i);
}

// d *= keep[row]: the mask ahead of a LayerNorm backward
template <int NV>
__device__ __forceinline__ void mask_row(const Keep<true>& kp, int64_t row, int C, int lane, Row<NV>& d) {
    Row<NV> k;
    keep_row<NV>(kp, row, C, lane, k);
#pragma unroll
    for (int i = 0; i < NV; ++i) { d.v[i].x *= k.v[i].x; d.v[i].y *= k.v[i].y; d.v[i].z *= k.v[i].z; d.v[i].w *= k.v[i].w; }
}

// acc += keep[row] . (gamma * x + beta): with a mask between beta and a sum over rows, gamma and beta no longer factor out
template <int NV>
__device__ __forceinline__ void add_kept(const Keep<true>& kp, int64_t row, int C, int lane, const Row<NV>& x,
                                         const Row<NV>& gam, const Row<NV>& bet, Row<NV>& acc) {
    Row<NV> k;
    keep_row<NV>(kp, row, C, lane, k);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        acc.v[i].x = fmaf(k.v[i].x, fmaf(gam.v[i].x, x.v[i].x, bet.v[i].x), acc.v[i].x);
        acc.v[i].y = fmaf(k.v[i].y, fmaf(gam.v[i].y, x.v[i].y, bet.v[i].y), acc.v[i].y);
        acc.v[i].z = fmaf(k.v[i].z, fmaf(gam.v[i].z, x.v[i].z, bet.v[i].z), acc.v[i].z);
        acc.v[i].w = fmaf(k.v[i].w, fmaf(gam.v[i].w, x.v[i].w, bet.v[i].w), acc.v[i].w);
    }
}

// out[r] = acc / (mean && deg > 1 ? deg : 1)
template <int NV>
__device__ __forceinline__ void store_reduced(float* __restrict__ out, int64_t r, int C, int lane, const Row<NV>& acc,
                                              int deg, int mean) {
    const float den = (mean && deg > 1) ? (float)deg : 1.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C)
            *reinterpret_cast<float4*>(out + r * C + c) =
                make_float4(acc.v[i].x / den, acc.v[i].y / den, acc.v[i].z / den, acc.v[i].w / den);
    }
}

}  // namespace
