// Readout head of every wrapper on the path, forward + loss + complete backward in ONE launch:
//
//   x_b   = sum_{n in molecule b} X[n, :]                     global_add_pool, equihnn_egnn.py:167 / mhnn.py:216
//   h1    = LN1(relu(W1 x + b1)),  h2 = LN2(relu(W2 h1 + b2))   MLP(C -> H -> H -> 1), mlp.py:91-99 (norm after ReLU)
//   y_b   = w3 . h2 + b3                                        equihnn_egnn.py:168-169 (.view(-1))
//   loss  = mean_{b < n_real} (y_b - t_b)^2                     F.mse_loss, main.py:49-63
//
// The design, the MFMA operand convention, the dropout elements and the loss ticket are readout_head.h's, shared with the paired
// tail's head (readout_pair.hip).  At the BASELINE batch this head is 257 rows: as separate launches (pool, 3 GEMMs, 2
// LayerNorms, loss, and their ~14 backward kernels) it cost ~150 us of a 1.73 ms step for ~75 MFLOP of work; every one of those
// launches sat at the in-graph floor.  This file's own phases:
//
//   pooling   wavefront w pools molecules 2w, 2w+1 side by side, eight rows deep, with clamped loads.
//   products  every weight tile is requested a phase ahead of its use (wt_tile_load / w_cols_load, then *_mma): the kernel is a
//             chain of short dependent phases on 17 workgroups, and every exposed memory latency is step time.
//   LDS       X, dX and ten H buffers [16][H + 4]; dZ2 and dZ1 have buffers of their own.
//   sums      [dbias | dgamma | dbeta] by one thread per (quantity, column).
//
// Round 6, measured with tools/readout_stamps.py (-DRH_STAMPS: s_memtime stamps of every phase): 26 us of the launch's 34 are
// the chain of phases itself -- pooling 5.4 us (rowptr -> rows -> LDS: two dependent round trips to memory), the layer products
// 3.2 + 1.7, the four LayerNorm phases ~0.9 each, the backward products 3.7 + 2.1, the weight-gradient slabs 4.0 -- and none of
// them shortens with fewer molecules per workgroup: the variant with FOUR molecules per workgroup (65 workgroups for a batch of
// 256, two wavefronts pooling one molecule) took 36.2 us against 34.1 (same box; the step 1.179 vs 1.172 ms) and left 65
// gradient slabs instead of 17 for the batched reduction (12.8 vs 9.4 us).  Dropped; in the graphed step the 17-workgroup launch
// is where the NEXT batch's index build runs on the idle CUs (trainer.GraphedTrainStep, signal point "readout").
//
// Training dropout (template flag DROP, entry hg_readout_mse_drop_f32): the same body with up to three sites (pre-pool, hidden
// 1, hidden 2).  The backward leaves the masked dh in LDS for the layer's dgamma and dbeta.  The p = 0 instantiations keep
// their argument block (RhArgs<false> is the `float eps` it replaces) and their statements.
#include "readout_head.h"

namespace {

#ifdef RH_STAMPS   // diagnostic build only (tools/readout_stamps.py): s_memtime stamps of the phases, wavefront 0 of every workgroup
__device__ unsigned long long* rh_stamp_buf = nullptr;
#define RH_STAMP(slot)                                                                                       \
    do {                                                                                                     \
        if (rh_stamp_buf && threadIdx.x == 0) rh_stamp_buf[(size_t)blockIdx.x * 32 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define RH_STAMP(slot) do { } while (0)
#endif

// The LayerNorms' eps and, with DROP, the dropout arguments: ONE kernel argument in the place of `float eps` (rowln.h's
// LnArgs does the same for the row kernels).
template <bool DROP>
struct RhArgs {
    float eps;
};
template <>
struct RhArgs<true> {
    float eps;
    uint32_t thr_x, thr_h;      // drop_threshold(p_x), drop_threshold(p_h); thr_x = 0 skips the pre-pool site
    float inv_x, inv_h;         // drop_inv_keep(.)
    const int64_t *seed_x, *seed_h1, *seed_h2;
};
// what a thread derives from them once: one hash key per site
template <bool DROP>
struct RhSites {
    __device__ explicit RhSites(const RhArgs<DROP>&) {}
};
template <>
struct RhSites<true> {
    RoSite x, h1, h2;
    __device__ explicit RhSites(const RhArgs<true>& a)
        : x{drop_key(a.thr_x ? (uint64_t)*a.seed_x : 0), a.thr_x, a.inv_x},
          h1{drop_key(a.thr_h ? (uint64_t)*a.seed_h1 : 0), a.thr_h, a.inv_h},
          h2{drop_key(a.thr_h ? (uint64_t)*a.seed_h2 : 0), a.thr_h, a.inv_h} {}
    __device__ __forceinline__ const RoSite& hidden(int layer) const { return layer == 1 ? h1 : h2; }
};

// out[m][n] = sum_k A[m][k] W[n][k]: A in LDS (16 rows, stride lda), W [N][K] row-major in global memory.
// The two halves are separate so that a tile's weights can be requested a phase ahead of their use.
template <int K>
__device__ __forceinline__ void wt_tile_load(const float* __restrict__ W, int t, int lane, float4 (&b)[K / 16]) {
    const float* wrow = W + (int64_t)(16 * t + (lane & 15)) * K + 4 * (lane >> 4);
#pragma unroll
    for (int s = 0; s < K / 16; ++s) b[s] = *reinterpret_cast<const float4*>(wrow + 16 * s);
}
template <int K>
__device__ __forceinline__ void wt_tile_mma(const float* sA, int lda, const float4 (&b)[K / 16], float* sOut, int ldo,
                                            int t, int lane) {
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < K / 16; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(sA + r * lda + 16 * s + 4 * q);
        acc = mfma16(a.x, b[s].x, acc);
        acc = mfma16(a.y, b[s].y, acc);
        acc = mfma16(a.z, b[s].z, acc);
        acc = mfma16(a.w, b[s].w, acc);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * t + r] = acc[g];
}

// out[m][i] = sum_o A[m][o] W[o][i]: A in LDS (stride lda), W [O][I] row-major in global memory
template <int O, int I>
__device__ __forceinline__ void w_cols_load(const float* __restrict__ W, int t, int lane, float (&b)[O / 4]) {
    const float* wcol = W + (int64_t)(4 * (lane >> 4)) * I + 16 * t + (lane & 15);
#pragma unroll
    for (int s = 0; s < O / 16; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[4 * s + j] = wcol[(int64_t)(16 * s + j) * I];
}
template <int O>
__device__ __forceinline__ void w_cols_mma(const float* sA, int lda, const float (&b)[O / 4], float* sOut, int ldo,
                                           int t, int lane) {
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < O / 16; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(sA + r * lda + 16 * s + 4 * q);
        acc = mfma16(a.x, b[4 * s + 0], acc);
        acc = mfma16(a.y, b[4 * s + 1], acc);
        acc = mfma16(a.z, b[4 * s + 2], acc);
        acc = mfma16(a.w, b[4 * s + 3], acc);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * t + r] = acc[g];
}

// dz = [a > 0] * rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)), dxh = dh * gamma; dh from sDH, or (sDH null)
// dh[m][c] = dy[m] * w3[c] for the last hidden layer.  DROP: dh is multiplied by the recomputed keep of hidden site `layer`
// first, and the masked dh is left in sDHm (the layer's parameter sums read it there; sDHm may be sDH: own elements only).
// (`layer` is a run-time argument, constant after inlining: as a template parameter it gave this helper two instantiations
// where the p = 0 kernel inlines one function twice, and that reordered the p = 0 instruction streams)
template <int H, bool DROP>
__device__ __forceinline__ void relu_ln_bwd_rows(const float* sDH, const float* __restrict__ w3, const float* sDy,
                                                 const float* sA, const float* sXH, const float* __restrict__ gamma,
                                                 const float* sRstd, float* sDZ, int ld, const RhSites<DROP>& ks, int layer,
                                                 int b0, float* sDHm) {
    constexpr int CPT = H / 32;
    const int row = threadIdx.x >> 5, l = threadIdx.x & 31;
    RoSite site{};
    if constexpr (DROP) site = ks.hidden(layer);
    float dxh[CPT], xh[CPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        float dh = sDH ? sDH[row * ld + c] : sDy[row] * w3[c];
        if constexpr (DROP) {
            dh *= ro_keep(site, b0 + row, H, c);
            sDHm[row * ld + c] = dh;
        }
        xh[j] = sXH[row * ld + c];
        dxh[j] = dh * gamma[c];
        s1 += dxh[j];
        s2 = fmaf(dxh[j], xh[j], s2);
    }
    s1 = ro_half_sum(s1) * (1.0f / H);
    s2 = ro_half_sum(s2) * (1.0f / H);
    const float rstd = sRstd[row];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        const float da = rstd * (dxh[j] - s1 - xh[j] * s2);
        sDZ[row * ld + c] = sA[row * ld + c] > 0.f ? da : 0.f;
    }
}

// this workgroup's [dbias | dgamma | dbeta] (3 H floats): column sums over the 16 rows, in row order
template <int H>
__device__ __forceinline__ void ln_param_sums(const float* sDH, const float* __restrict__ w3, const float* sDy,
                                              const float* sXH, const float* sDZ, int ld, float* __restrict__ out) {
    static_assert(3 * H <= RO_THREADS, "one thread per (quantity, column)");
    const int t = threadIdx.x;
    if (t >= 3 * H) return;
    const int which = t / H, c = t - which * H;
    float s = 0.f;
    if (which == 0) {
        for (int m = 0; m < RO_ROWS; ++m) s += sDZ[m * ld + c];
    } else {
        const float wc = sDH ? 0.f : w3[c];
        for (int m = 0; m < RO_ROWS; ++m) {
            const float dh = sDH ? sDH[m * ld + c] : sDy[m] * wc;
            s += which == 1 ? dh * sXH[m * ld + c] : dh;
        }
    }
    out[t] = s;
}

template <int C, int H>
struct RhLds {
    static constexpr int LX = C + 4, LH = H + 4;
    static constexpr int X = 0, DX = X + RO_ROWS * LX, A1 = DX + RO_ROWS * LX, XH1 = A1 + RO_ROWS * LH,
                         H1 = XH1 + RO_ROWS * LH, A2 = H1 + RO_ROWS * LH, XH2 = A2 + RO_ROWS * LH,
                         H2 = XH2 + RO_ROWS * LH, DZ2 = H2 + RO_ROWS * LH, DH1 = DZ2 + RO_ROWS * LH,
                         DZ1 = DH1 + RO_ROWS * LH, STAT = DZ1 + RO_ROWS * LH, VEC = STAT + 4 * RO_ROWS,
                         TOTAL = VEC + 7 * H + 4;   // VEC: b1 g1 be1 b2 g2 be2 w3 b3
};

template <int C, int H, bool DROP = false, bool SL1 = false>
__global__ void __launch_bounds__(RO_THREADS)
k_readout_mse(const float* __restrict__ X, const int* __restrict__ rowptr, int n_graphs, int n_real, RoWeights w,
              RoLossArgs<RhArgs<DROP>, SL1> ra, const float* __restrict__ target, float* __restrict__ y, float* __restrict__ loss,
              float* __restrict__ dX, RoSlabs slab, float* __restrict__ loss_part, int* __restrict__ state) {
    using L = RhLds<C, H>;
    constexpr int LX = L::LX, LH = L::LH;
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* sX = s_mem + L::X;
    float* sDX = s_mem + L::DX;
    float* sA1 = s_mem + L::A1;
    float* sXH1 = s_mem + L::XH1;
    float* sH1 = s_mem + L::H1;
    float* sA2 = s_mem + L::A2;
    float* sXH2 = s_mem + L::XH2;
    float* sH2 = s_mem + L::H2;
    float* sDZ2 = s_mem + L::DZ2;
    float* sDH1 = s_mem + L::DH1;
    float* sDZ1 = s_mem + L::DZ1;
    float* sR1 = s_mem + L::STAT;
    float* sR2 = sR1 + RO_ROWS;
    float* sDy = sR2 + RO_ROWS;
    float* sSq = sDy + RO_ROWS;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.x * RO_ROWS;
    const bool train = target != nullptr;
    const float eps = ra.eps;
    RH_STAMP(0);

    // ---- requests issued first: the small parameter vectors (to LDS) and this wavefront's tile of W1
    float* sV = s_mem + L::VEC;
    const float *vb1 = sV, *vg1 = sV + H, *vbe1 = sV + 2 * H, *vb2 = sV + 3 * H, *vg2 = sV + 4 * H,
                *vbe2 = sV + 5 * H, *vw3 = sV + 6 * H, *vb3 = sV + 7 * H;
    constexpr int VPT = (7 * H + RO_THREADS - 1) / RO_THREADS;
    float vreg[VPT];
    {
        const float* src[7] = {w.b1, w.g1, w.be1, w.b2, w.g2, w.be2, w.w3};
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int i = threadIdx.x + k * RO_THREADS;
            vreg[k] = i < 7 * H ? src[i / H][i % H] : 0.f;
        }
    }
    const float vb3_reg = w.b3[0];
    static_assert(H / 16 <= RO_WAVES && C / 16 <= 2 * RO_WAVES, "one H tile, two C tiles per wavefront");
    const bool has_h_tile = wave < H / 16;
    float4 bw1[C / 16];
    if (has_h_tile) wt_tile_load<C>(w.w1, wave, lane, bw1);
    const RhSites<DROP> ks(ra);     // (the seeds: three scalar loads behind the requests above)

    // ---- global_add_pool: wavefront w owns molecules 2w, 2w+1 of the tile; a row of X is C/4 float4 lanes, so
    // 64 / (C/4) atoms are read side by side, eight deep for each of the two molecules at once
    constexpr int LPR = C / 4, AP = 64 / LPR;
    static_assert(LPR <= 64 && 64 % LPR == 0, "C in {16..256}, power-of-two float4 lanes");
    const int sub = lane / LPR, cl = lane - sub * LPR;
    {
        const int m0 = b0 + 2 * wave, m1 = m0 + 1;
        int beg0 = 0, end0 = 0, beg1 = 0, end1 = 0;
        if (m0 < n_real) { beg0 = rowptr[m0]; end0 = rowptr[m0 + 1]; }
        if (m1 < n_real) { beg1 = rowptr[m1]; end1 = rowptr[m1 + 1]; }
        const int last0 = end0 > 0 ? end0 - 1 : 0, last1 = end1 > 0 ? end1 - 1 : 0;
        float4 acc0 = f4_zero(), acc1 = f4_zero();
        constexpr int DEEP = 8;   // rows in flight per molecule: a QM9 molecule (<= 29 atoms) takes <= 4 rounds
        for (int n0 = beg0 + sub, n1 = beg1 + sub; n0 < end0 || n1 < end1; n0 += DEEP * AP, n1 += DEEP * AP) {
            float4 v0[DEEP], v1[DEEP];
#pragma unroll
            for (int u = 0; u < DEEP; ++u) {
                const int a0 = n0 + u * AP, a1 = n1 + u * AP;
                v0[u] = *reinterpret_cast<const float4*>(X + (int64_t)(a0 < end0 ? a0 : last0) * C + 4 * cl);
                v1[u] = *reinterpret_cast<const float4*>(X + (int64_t)(a1 < end1 ? a1 : last1) * C + 4 * cl);
            }
#pragma unroll
            for (int u = 0; u < DEEP; ++u) {
                if (n0 + u * AP < end0) {
                    if constexpr (DROP) ro_mask4<C>(ks.x, n0 + u * AP, cl, v0[u]);
                    f4_add(acc0, v0[u]);
                }
                if (n1 + u * AP < end1) {
                    if constexpr (DROP) ro_mask4<C>(ks.x, n1 + u * AP, cl, v1[u]);
                    f4_add(acc1, v1[u]);
                }
            }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            acc0.x += __shfl_xor(acc0.x, off); acc0.y += __shfl_xor(acc0.y, off);
            acc0.z += __shfl_xor(acc0.z, off); acc0.w += __shfl_xor(acc0.w, off);
            acc1.x += __shfl_xor(acc1.x, off); acc1.y += __shfl_xor(acc1.y, off);
            acc1.z += __shfl_xor(acc1.z, off); acc1.w += __shfl_xor(acc1.w, off);
        }
        if (sub == 0) {
            *reinterpret_cast<float4*>(sX + (2 * wave) * LX + 4 * cl) = acc0;
            *reinterpret_cast<float4*>(sX + (2 * wave + 1) * LX + 4 * cl) = acc1;
        }
    }
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = threadIdx.x + k * RO_THREADS;
        if (i < 7 * H) sV[i] = vreg[k];
    }
    if (threadIdx.x == 0) sV[7 * H] = vb3_reg;
    RH_STAMP(1);
    __syncthreads();
    RH_STAMP(2);

    // ---- forward
    float4 bw2[H / 16];
    if (has_h_tile) {
        wt_tile_mma<C>(sX, LX, bw1, sA1, LH, wave, lane);
        wt_tile_load<H>(w.w2, wave, lane, bw2);          // in flight during LayerNorm 1
    }
    __syncthreads();
    RH_STAMP(3);
    ro_relu_ln_rows<H, DROP>(sA1, vb1, vg1, vbe1, sXH1, sH1, sR1, LH, eps, ks, 1, b0);
    __syncthreads();
    RH_STAMP(4);
    float cw2[H / 4];
    if (has_h_tile) {
        wt_tile_mma<H>(sH1, LH, bw2, sA2, LH, wave, lane);
        if (train) w_cols_load<H, H>(w.w2, wave, lane, cw2);   // for d h1, three phases ahead
    }
    __syncthreads();
    RH_STAMP(5);
    ro_relu_ln_rows<H, DROP>(sA2, vb2, vg2, vbe2, sXH2, sH2, sR2, LH, eps, ks, 2, b0);
    __syncthreads();
    RH_STAMP(6);
    {
        constexpr int CPT = H / 32;
        const int row = threadIdx.x >> 5, l = threadIdx.x & 31;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; ++j) s = fmaf(sH2[row * LH + l + 32 * j], vw3[l + 32 * j], s);
        s = ro_half_sum(s) + vb3[0];
        if (l == 0) {
            const int b = b0 + row;
            if (b < n_graphs) y[b] = s;
            float dy = 0.f, sq = 0.f;
            if (train && b < n_real) {
                const float d = s - target[b];
                if constexpr (SL1) {
                    float slope;
                    sl1_term_slope(d, ra.beta, ra.scale, sq, slope);
                    dy = slope / (float)n_real;
                } else {
                dy = 2.0f * d / (float)n_real;
                sq = d * d;
                }
            }
            sDy[row] = dy;
            sSq[row] = sq;
        }
    }
    __syncthreads();
    RH_STAMP(7);
    if (!train) return;

    // ---- backward
    const int64_t wg = blockIdx.x;
    // (DROP: the masked dh2 goes to sDZ1, which is free until the LayerNorm-1 backward two barriers on)
    relu_ln_bwd_rows<H, DROP>(nullptr, vw3, sDy, sA2, sXH2, vg2, sR2, sDZ2, LH, ks, 2, b0, sDZ1);
    {   // dw3 | db3 | pad, and the squared-error partial (SL1: the sum of the rows' loss terms), in row order
        float* v3 = slab.v3 + wg * (H + 4);
        const int t = threadIdx.x;
        if (t < H) {
            float s = 0.f;
            for (int m = 0; m < RO_ROWS; ++m) s = fmaf(sDy[m], sH2[m * LH + t], s);
            v3[t] = s;
        } else if (t == H) {
            float s = 0.f, e = 0.f;
            for (int m = 0; m < RO_ROWS; ++m) { s += sDy[m]; e += sSq[m]; }
            v3[H] = s;
            v3[H + 1] = 0.f; v3[H + 2] = 0.f; v3[H + 3] = 0.f;
            // agent-scope atomic store: visible to the other XCDs without a cache write-back; it has long
            // completed when this workgroup takes its ticket at the end of the kernel
            __hip_atomic_store(loss_part + wg, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    RH_STAMP(8);
    float cw1a[H / 4], cw1b[H / 4];   // W1 columns of this wavefront's (up to) two C tiles, for dx
    const bool has_c0 = wave < C / 16, has_c1 = wave + RO_WAVES < C / 16;
    if (has_h_tile) w_cols_mma<H>(sDZ2, LH, cw2, sDH1, LH, wave, lane);
    if (has_c0) w_cols_load<H, C>(w.w1, wave, lane, cw1a);
    if (has_c1) w_cols_load<H, C>(w.w1, wave + RO_WAVES, lane, cw1b);
    if constexpr (DROP) ln_param_sums<H>(sDZ1, nullptr, nullptr, sXH2, sDZ2, LH, slab.v2 + wg * 3 * H);
    else ln_param_sums<H>(nullptr, vw3, sDy, sXH2, sDZ2, LH, slab.v2 + wg * 3 * H);
    ro_outer_rows<H, H>(sDZ2, LH, sH1, LH, slab.w2 + wg * H * H, wave, lane);
    RH_STAMP(9);
    __syncthreads();
    RH_STAMP(10);
    relu_ln_bwd_rows<H, DROP>(sDH1, nullptr, nullptr, sA1, sXH1, vg1, sR1, sDZ1, LH, ks, 1, b0, sDH1);
    __syncthreads();
    RH_STAMP(11);
    if (has_c0) w_cols_mma<H>(sDZ1, LH, cw1a, sDX, LX, wave, lane);
    if (has_c1) w_cols_mma<H>(sDZ1, LH, cw1b, sDX, LX, wave + RO_WAVES, lane);
    __syncthreads();
    RH_STAMP(12);

    // ---- dX[n, :] = dx[molecule(n), :] (zero rows for the padding molecules b >= n_real: their dy is 0); DROP: times the
    // pre-pool keep of row n
    for (int mi = 2 * wave; mi < 2 * wave + 2; ++mi) {
        const int b = b0 + mi;
        if (b >= n_graphs) continue;
        const float4 g = *reinterpret_cast<const float4*>(sDX + mi * LX + 4 * cl);
        const int beg = rowptr[b], end = rowptr[b + 1];
        for (int n = beg + sub; n < end; n += AP) {
            float4 gn = g;
            if constexpr (DROP) ro_mask4<C>(ks.x, n, cl, gn);
            *reinterpret_cast<float4*>(dX + (int64_t)n * C + 4 * cl) = gn;
        }
    }

    RH_STAMP(13);
    // ---- the two large gradient slabs last: nothing in this kernel waits for them
    ln_param_sums<H>(sDH1, nullptr, nullptr, sXH1, sDZ1, LH, slab.v1 + wg * 3 * H);
    ro_outer_rows<H, C>(sDZ1, LH, sX, LX, slab.w1 + wg * (int64_t)H * C, wave, lane);
    RH_STAMP(14);

    // ---- loss = sum of the workgroups' partials / n_real, by the last workgroup to arrive, in workgroup order
    if (threadIdx.x == H) {   // the thread that stored this workgroup's partial: its store is ordered before its ticket
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        const int ticket = __hip_atomic_fetch_add(state, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            float e = 0.f;
            for (unsigned i = 0; i < gridDim.x; ++i)
                e += __hip_atomic_load(loss_part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            loss[0] = e / (float)n_real;
            __hip_atomic_store(state, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
    }
}

template <int C, int H, bool DROP, bool SL1>
int rh_launch(const float* x, const int32_t* rowptr, int n_graphs, int n_real, const RoWeights& w,
              const RoLossArgs<RhArgs<DROP>, SL1>& ra,
              const float* target, float* y, float* loss, float* dx, const RoSlabs& slab, float* loss_part, int* state,
              int n_wg, hipStream_t stream) {
    constexpr size_t lds = (size_t)RhLds<C, H>::TOTAL * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_readout_mse<C, H, DROP, SL1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return EQH_ERR_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_readout_mse<C, H, DROP, SL1>), dim3(n_wg), dim3(RO_THREADS), lds, stream, x, rowptr, n_graphs, n_real, w,
                       ra, target, y, loss, dx, slab, loss_part, state);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

}  // namespace

#ifdef RH_STAMPS
extern "C" int hg_readout_debug_stamps(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(rh_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? EQH_OK : EQH_ERR_LAUNCH;
}
#endif

extern "C" int hg_readout_mse_supported(int32_t C, int32_t H) {
    return (C == 64 || C == 128 || C == 256) && (H == 64 || H == 128);
}

extern "C" size_t hg_readout_mse_workspace_bytes(int32_t n_graphs, int32_t C, int32_t H) {
    if (n_graphs <= 0 || !hg_readout_mse_supported(C, H)) return 0;
    return ro_plan(n_graphs, C, H).total * sizeof(float);
}

namespace {

// hg_readout_mse_f32 (DROP = false) and hg_readout_mse_drop_f32 (DROP = true), and their hg_readout_sl1_* twins (SL1 = true):
// one host function
template <bool DROP, bool SL1>
int readout_mse(const float* x, const int32_t* rowptr, int32_t n_graphs, int32_t n_real, int32_t C, int32_t H,
                const float* const* weights, const RoLossArgs<RhArgs<DROP>, SL1>& ra, const float* target, float* y, float* loss, float* dx,
                float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes, int32_t* state,
                void* stream_) {
    if (n_graphs < 0 || n_real < 0 || n_real > n_graphs || !hg_readout_mse_supported(C, H)) return EQH_ERR_ARG;
    if (n_graphs == 0) return EQH_OK;
    const RoPlan p = ro_plan(n_graphs, C, H);
    int rc = ro_check_args(!x || !rowptr || !y, !eqh_aligned16(x), weights, target, n_real, !dx, !eqh_aligned16(dx), loss,
                           dweights, workspace, workspace_bytes, p.total * sizeof(float), state);
    if (rc) return rc;
    const bool train = target != nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* ws = static_cast<float*>(workspace);
    const RoWeights w = ro_weights(weights);
    const RoSlabs slab = ro_slabs(ws, p, train);
    float* loss_part = train ? ws + p.off_loss : nullptr;
    rc = EQH_ERR_ARG;
#define RH_CASE(CC, HH)                                                                                           \
    if (C == CC && H == HH)                                                                                       \
        rc = rh_launch<CC, HH, DROP, SL1>(x, rowptr, n_graphs, n_real, w, ra, target, y, loss, dx, slab, loss_part, \
                                          state, p.n_wg, stream);
    RH_CASE(64, 64) RH_CASE(64, 128) RH_CASE(128, 64) RH_CASE(128, 128) RH_CASE(256, 64) RH_CASE(256, 128)
#undef RH_CASE
    if (rc || !train) return rc;
    return ro_reduce_head_slabs(slab, p, C, H, dweights, ws + p.off_discard, accumulate, stream);
}

}  // namespace

extern "C" int hg_readout_mse_f32(const float* x, const int32_t* rowptr, int32_t n_graphs, int32_t n_real, int32_t C,
                                  int32_t H, const float* const* weights, float eps, const float* target, float* y,
                                  float* loss, float* dx, float* const* dweights, int32_t accumulate, void* workspace,
                                  size_t workspace_bytes, int32_t* state, void* stream_) {
    return readout_mse<false, false>(x, rowptr, n_graphs, n_real, C, H, weights, RhArgs<false>{eps}, target, y, loss, dx, dweights,
                              accumulate, workspace, workspace_bytes, state, stream_);
}

extern "C" int hg_readout_mse_drop_f32(const float* x, const int32_t* rowptr, int32_t n_graphs, int32_t n_real, int32_t C,
                                       int32_t H, const float* const* weights, float eps, const float* target, float* y,
                                       float* loss, float* dx, float* const* dweights, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, int32_t* state, float p_x, float p_h, const int64_t* seed_x,
                                       const int64_t* seed_h1, const int64_t* seed_h2, void* stream_) {
    if (int rc = ro_check_drop(p_x, p_h, seed_x != nullptr, seed_h1 && seed_h2)) return rc;
    const RhArgs<true> ra{eps, drop_threshold(p_x), drop_threshold(p_h), drop_inv_keep(p_x), drop_inv_keep(p_h),
                          seed_x, seed_h1, seed_h2};
    return readout_mse<true, false>(x, rowptr, n_graphs, n_real, C, H, weights, ra, target, y, loss, dx, dweights, accumulate,
                             workspace, workspace_bytes, state, stream_);
}

// The same two launches with the loss family of loss_family.h in the place of the squared error (SL1 forms of the kernel):
// beta >= 0 and scale > 0, both finite, checked with the entry's own arguments ahead of any launch.
extern "C" int hg_readout_sl1_f32(const float* x, const int32_t* rowptr, int32_t n_graphs, int32_t n_real, int32_t C,
                                  int32_t H, const float* const* weights, float eps, const float* target, float* y,
                                  float* loss, float* dx, float* const* dweights, int32_t accumulate, void* workspace,
                                  size_t workspace_bytes, int32_t* state, float beta, float scale, void* stream_) {
    if (!sl1_args_ok(beta, scale)) return EQH_ERR_ARG;
    return readout_mse<false, true>(x, rowptr, n_graphs, n_real, C, H, weights, ro_sl1_args(RhArgs<false>{eps}, beta, scale),
                                    target, y, loss, dx, dweights, accumulate, workspace, workspace_bytes, state, stream_);
}

extern "C" int hg_readout_sl1_drop_f32(const float* x, const int32_t* rowptr, int32_t n_graphs, int32_t n_real, int32_t C,
                                       int32_t H, const float* const* weights, float eps, const float* target, float* y,
                                       float* loss, float* dx, float* const* dweights, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, int32_t* state, float p_x, float p_h, const int64_t* seed_x,
                                       const int64_t* seed_h1, const int64_t* seed_h2, float beta, float scale,
                                       void* stream_) {
    if (!sl1_args_ok(beta, scale)) return EQH_ERR_ARG;
    if (int rc = ro_check_drop(p_x, p_h, seed_x != nullptr, seed_h1 && seed_h2)) return rc;
    const RhArgs<true> ra{eps, drop_threshold(p_x), drop_threshold(p_h), drop_inv_keep(p_x), drop_inv_keep(p_h),
                          seed_x, seed_h1, seed_h2};
    return readout_mse<true, true>(x, rowptr, n_graphs, n_real, C, H, weights, ro_sl1_args(ra, beta, scale), target, y, loss,
                                   dx, dweights, accumulate, workspace, workspace_bytes, state, stream_);
}
