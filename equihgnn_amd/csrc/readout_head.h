// What the two one-launch read-out heads share (readout.hip: k_readout_mse, one pool; readout_pair.hip: k_readout_pair_mse, two
// pools side by side).  Both are  pool -> h1 = LN1(relu(W1 z + b1)) -> h2 = LN2(relu(W2 h1 + b2)) -> y = w3 . h2 + b3 ->
// loss = mean_{b < n_real} (y_b - t_b)^2  with the complete backward, in ONE launch: a workgroup of 512 threads owns 16 molecules
// (the M of the fp32 16 x 16 x 4 MFMA), the activations stay in LDS for the backward half, every workgroup leaves one slab of every
// parameter gradient for the library's fixed-order reducer (deferred into the step's batched reduction when that is active), and
// nothing is atomic on data: the launch is bitwise reproducible.
//
// MFMA operand convention (lane l: r = l & 15, q = l >> 4): A[m = r][k = q], B[k = q][n = r], D[m = 4 q + g][n = r] in accumulator
// component g.  Four MFMAs share one float4 of K: the j-th of them takes component j on both sides, i.e. k = 16 s + 4 q + j (a
// permutation of K, which a sum does not see).
//
// Training dropout (template flag DROP of the kernels): keep = 0 or 1 / (1 - p) from the hash of (seed in device memory, element
// index) of drop_hash.h, nothing stored.  The element indices are those of the separate launches a head replaces:
//   pre-pool (p_x)    element n C + c of the [rows, C] input: x_b[c] = sum_n keep(n C + c) X[n, c], dX[n, c] = keep(n C + c)
//                     dxpool[b, c] (faf_dropout_add's element);
//   hidden 1, 2 (p_h) element b H + c, b the global molecule row: h_i[b, c] = keep_i(b H + c) LN_i(relu(.)), the element of
//                     hg_bias_relu_ln_drop_*.  LDS holds the masked h_i (dW2, dw3 and the next product read it as it is); the
//                     backward masks dh ahead of the LayerNorm backward, so dgamma and dbeta are column sums of the masked dh.
// A kernel's Sites type says how it keeps the hash keys: `ks.hidden(layer)` is all the helpers here ask of it.
//
// The loss: thread H of a workgroup stores the workgroup's squared-error partial with the v3 slab and, at the end of the kernel,
// takes a ticket; the last workgroup to arrive sums the partials in workgroup order and resets the ticket for the next launch.
//
// NOT here, although both kernels have them statement for statement: the staging of the parameter vectors, the output / dy
// phase, the v3 slab and the loss ticket.  As helpers each of them moved the instruction stream of the kernel that calls it
// (the compiler promotes a kernel's locals before it inlines a helper, and the order of the values a phase merges follows the
// set of locals the kernel has at that point); they stay written out in the kernels.  The LayerNorm backward stays apart too:
// readout.hip's stores the masked dh unconditionally, the paired kernel's only where it has a buffer, and one body with a
// nullable destination put a null test into k_readout_mse's DROP forms.
//
// Other losses (template flag SL1 of the kernels, entries hg_readout_sl1_* / hg_readout_pair_sl1_*): the family of
// loss_family.h in the place of the squared error -- the two statements that form a row's dy and its loss term, under
// `if constexpr (SL1)`, with the MSE statements literally where they were.  The partial is then the workgroup's sum of terms.
// beta and scale travel behind the kernel's own argument block (RoLossArgs), so an MSE form keeps its block as it is.
#pragma once
#include <type_traits>

#include "common.h"
#include "drop_hash.h"
#include "loss_family.h"
#include "mfma.h"

namespace {

// a head's argument block A (RhArgs / RpArgs) with the family's two floats behind it -- for the SL1 forms only
template <class A>
struct RoSl1Args : A {
    float beta, scale;
};
template <class A, bool SL1>
using RoLossArgs = std::conditional_t<SL1, RoSl1Args<A>, A>;
template <class A>
inline RoSl1Args<A> ro_sl1_args(const A& a, float beta, float scale) {
    RoSl1Args<A> r;
    static_cast<A&>(r) = a;
    r.beta = beta;
    r.scale = scale;
    return r;
}

constexpr int RO_THREADS = 512;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_ROWS = 16;  // molecules per workgroup = the M of one MFMA tile

struct RoWeights {
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3;
};
struct RoSlabs {   // per-workgroup partial gradients: [n_wg][H*K1], [n_wg][H*H], [n_wg][3H] x 2, [n_wg][H+4]
    float *w1, *w2, *v1, *v2, *v3;
};

// what a thread derives from a site's arguments: its hash key, threshold and 1 / (1 - p)
struct RoSite {
    DropKey key;
    uint32_t thr;
    float inv;
};
// keep-scale of element row * H + c of a hidden site.  A lane's columns are l + 32 j, so it asks for the aligned pair
// that holds c (keep_scale2's contract: an even index; row * H is even) and takes its half.
__device__ __forceinline__ float ro_keep(const RoSite& s, int64_t row, int H, int c) {
    float k0, k1;
    keep_scale2(s.key, (uint64_t)row * (uint64_t)H + (uint64_t)(c & ~1), s.thr, s.inv, k0, k1);
    return (c & 1) ? k1 : k0;
}
// v *= keep of the float4 at row n, columns 4 cl .. 4 cl + 3 of [rows, C] (a pre-pool site; C % 4 == 0)
template <int C>
__device__ __forceinline__ void ro_mask4(const RoSite& s, int n, int cl, float4& v) {
    if (s.thr) keep_scale4(s.key, (uint64_t)n * (uint64_t)C + (uint64_t)(4 * cl), s.thr, s.inv, v);
}

// sum over the 32 lanes that share a row
__device__ __forceinline__ float ro_half_sum(float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// out[o][i] = sum_{m < 16} D[m][o] In[m][i] (both in LDS) -> this workgroup's slab [O][I] in global memory
template <int O, int I>
__device__ __forceinline__ void ro_outer_rows(const float* sD, int ldd, const float* sIn, int ldi, float* __restrict__ out,
                                              int wave, int lane) {
    const int r = lane & 15, q = lane >> 4;
    for (int t = wave; t < (O / 16) * (I / 16); t += RO_WAVES) {
        const int to = t / (I / 16), ti = t - to * (I / 16);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = mfma16(sD[(4 * q + j) * ldd + 16 * to + r], sIn[(4 * q + j) * ldi + 16 * ti + r], acc);
#pragma unroll
        for (int g = 0; g < 4; ++g) out[(int64_t)(16 * to + 4 * q + g) * I + 16 * ti + r] = acc[g];
    }
}

// in place: sZ <- a = relu(z + bias); sXH <- (a - mean) * rstd; sH <- sXH * gamma + beta; 32 lanes per row.
// DROP: sH <- keep . (sXH * gamma + beta), keep of hidden site `layer` at molecule row b0 + row
template <int H, bool DROP, class Sites>
__device__ __forceinline__ void ro_relu_ln_rows(float* sZ, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float* sXH, float* sH, float* sRstd, int ld,
                                                float eps, const Sites& ks, int layer, int b0) {
    constexpr int CPT = H / 32;
    const int row = threadIdx.x >> 5, l = threadIdx.x & 31;
    RoSite site{};
    if constexpr (DROP) site = ks.hidden(layer);
    float a[CPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        a[j] = fmaxf(sZ[row * ld + c] + bias[c], 0.f);
        s += a[j];
    }
    const float mu = ro_half_sum(s) * (1.0f / H);
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) v = fmaf(a[j] - mu, a[j] - mu, v);
    const float rstd = 1.0f / sqrtf(ro_half_sum(v) * (1.0f / H) + eps);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        const float xh = (a[j] - mu) * rstd;
        sZ[row * ld + c] = a[j];
        sXH[row * ld + c] = xh;
        if constexpr (DROP)
            sH[row * ld + c] = fmaf(xh, gamma[c], beta[c]) * ro_keep(site, b0 + row, H, c);
        else
            sH[row * ld + c] = fmaf(xh, gamma[c], beta[c]);
    }
    if (l == 0) sRstd[row] = rstd;
}

// ---- host side

struct RoPlan {   // the workspace of a launch over n_graphs molecules, K1 inputs of layer 1 (C, or 2C for the paired head)
    int n_wg;
    size_t off_w1, off_w2, off_v1, off_v2, off_v3, off_loss, off_discard, total;   // in floats
};

inline RoPlan ro_plan(int n_graphs, int K1, int H) {
    RoPlan p;
    p.n_wg = (n_graphs + RO_ROWS - 1) / RO_ROWS;
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
    p.off_w1 = take((size_t)p.n_wg * H * K1);
    p.off_w2 = take((size_t)p.n_wg * H * H);
    p.off_v1 = take((size_t)p.n_wg * 3 * H);
    p.off_v2 = take((size_t)p.n_wg * 3 * H);
    p.off_v3 = take((size_t)p.n_wg * (H + 4));
    p.off_loss = take((size_t)p.n_wg);
    p.off_discard = take(4);
    p.total = o;
    return p;
}

// The argument checks of a head's host function once its sizes are in range and n_graphs > 0.  The head passes what it found
// about its own pointers: `in_null` / `in_misaligned` for the rows, row lists and y, `out_null` / `out_misaligned` for the row
// gradients.  A missing pointer is EQH_ERR_ARG ahead of a misaligned one, first for the forward's arguments, then (target set)
// for the backward's; `need_bytes` is the plan's workspace.
inline int ro_check_args(bool in_null, bool in_misaligned, const float* const* weights, const float* target, int n_real,
                         bool out_null, bool out_misaligned, const float* loss, float* const* dweights, const void* workspace,
                         size_t workspace_bytes, size_t need_bytes, const int32_t* state) {
    if (in_null || !weights) return EQH_ERR_ARG;
    for (int i = 0; i < 10; ++i)
        if (!weights[i]) return EQH_ERR_ARG;
    if (in_misaligned || !eqh_aligned16(weights[0]) || !eqh_aligned16(weights[4])) return EQH_ERR_ALIGN;
    if (!target) return EQH_OK;
    if (n_real == 0 || !loss || out_null || !dweights || !workspace || !state) return EQH_ERR_ARG;
    for (int i = 0; i < 10; ++i)
        if (!dweights[i]) return EQH_ERR_ARG;
    if (out_misaligned || !eqh_aligned16(workspace)) return EQH_ERR_ALIGN;
    return workspace_bytes < need_bytes ? EQH_ERR_ARG : EQH_OK;
}

inline RoWeights ro_weights(const float* const* w) { return RoWeights{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9]}; }

// the slabs of a training launch in its workspace (inference: none)
inline RoSlabs ro_slabs(float* ws, const RoPlan& p, bool train) {
    if (!train) return RoSlabs{nullptr, nullptr, nullptr, nullptr, nullptr};
    return RoSlabs{ws + p.off_w1, ws + p.off_w2, ws + p.off_v1, ws + p.off_v2, ws + p.off_v3};
}

// parameter gradients: fixed-order sums over the workgroup slabs (deferred into the step's batched reduction when that is
// active)
inline int ro_reduce_head_slabs(const RoSlabs& slab, const RoPlan& p, int K1, int H, float* const* dweights, float* discard,
                                int accumulate, hipStream_t stream) {
    int rc = eqh_reduce_slabs_async(slab.w1, p.n_wg, (int64_t)H * K1, dweights[0], stream, accumulate);
    if (rc) return rc;
    rc = eqh_reduce_slabs_async(slab.w2, p.n_wg, (int64_t)H * H, dweights[4], stream, accumulate);
    if (rc) return rc;
    rc = eqh_reduce_slabs3_async(slab.v1, p.n_wg, 3 * (int64_t)H, dweights[1], dweights[2], dweights[3], H, H, accumulate,
                                 stream);
    if (rc) return rc;
    rc = eqh_reduce_slabs3_async(slab.v2, p.n_wg, 3 * (int64_t)H, dweights[5], dweights[6], dweights[7], H, H, accumulate,
                                 stream);
    if (rc) return rc;
    return eqh_reduce_slabs3_async(slab.v3, p.n_wg, (int64_t)H + 4, dweights[8], dweights[9], discard, H, 1, accumulate, stream);
}

// The drop entries' own arguments: 0 <= p < 1 (a NaN fails the comparison), checked first; a call without an active site belongs
// to the entry without dropout; an active site needs its seeds (`seeds_x`, `seeds_h`: whether the entry's pre-pool / hidden
// seeds are all there).
inline int ro_check_drop(float p_x, float p_h, bool seeds_x, bool seeds_h) {
    if (!(p_x >= 0.f && p_x < 1.f) || !(p_h >= 0.f && p_h < 1.f) || (p_x == 0.f && p_h == 0.f)) return EQH_ERR_ARG;
    if ((p_x > 0.f && !seeds_x) || (p_h > 0.f && !seeds_h)) return EQH_ERR_ARG;
    return EQH_OK;
}

}  // namespace
