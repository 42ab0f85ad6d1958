// Readout head of the paired tail (models._PairedBase: mhnn, egnn_equihnn, faformer_equihnn, visnet_equihnn), forward + loss +
// complete backward in ONE launch -- the head of readout_head.h for an input that is two pools side by side:
//
//   z_b   = [ sum_{n in molecule b} X[n, :] | sum_{m in molecule b, e_order[m] > 2} E[m, :] ]     mhnn.py:58,72 ([B, 2C])
//   h1    = LN1(relu(W1 z + b1)),  h2 = LN2(relu(W2 h1 + b2))     MLP(2C -> H -> H -> 1), H = 2 output_hidden, mlp.py:91-99
//   y_b   = w3 . h2 + b3,   loss = mean_{b < n_real} (y_b - t_b)^2
//
// The design, the MFMA operand convention, the dropout elements and the loss ticket are readout_head.h's, shared with
// k_readout_mse of readout.hip.  This file's own phases:
//
//   pooling   wavefront w pools molecules 2w, 2w+1: first their node rows (rowptr of the atom pool), then their hyperedge rows
//             through the hyperedge pool (rowptr + perm, a null perm is the identity, hg_pool_pair_fwd's convention): 64
//             entries are looked at side by side and a ballot picks the rows of order > 2; a hyperedge of order <= 2 (a
//             bond: all but about one per molecule) is never loaded.  dE is written the same way, 64 entries per round.
//   layer 1   K = 2C up to 512: W1 is read in K halves of 256 (a wavefront's two H tiles at H = 256 hold 128 registers of it at
//             a time, not 256); W1 is not requested ahead of the pooling phase as readout.hip does.
//   backward  dX [N, C] and dE [M, C] (rows of order <= 2 and of the padding molecules: exact zeros), dW1 [H, 2C].
//   LDS       readout.hip's layout (X, dX, ten H buffers) needs ~232 KB at (C, H) = (256, 256).  Here: X [16][2C + 4], SEVEN
//             H buffers [16][H + 4] (A, XH, H of both layers and dH1) -- dZ2 is formed in place over A2 and dZ1 in place over
//             A1 (the ReLU mask is the last read of A), and the pooled gradient dZ1 W1 [16][2C + 4] is written over the run
//             H1 | A2 | XH2 | H2, whose last readers (dW2's slab, the layer-2 parameter sums) are two barriers back.  156 944
//             bytes at (256, 256) of the 160 KB a workgroup can have; dW1's slab still goes last, nothing waits for it.
//
// Training dropout (template flag DROP, entry hg_readout_pair_mse_drop_f32): up to FOUR sites -- pre-pool x and pre-pool e (both
// p_x; element m C + c of E [M, C] for the latter), hidden 1, hidden 2 -- with the elements and the draw order of the launches
// this one replaces (_drop(x), _drop(e) after the last conv application, then the head's two hg_bias_relu_ln_drop_fwd).  The
// masked dh1 stays in the dH1 buffer for layer 1's dgamma / dbeta; layer 2's masked dh2 = keep . dy w3 has no buffer of its own
// and is recomputed (one hash per element) by the thread that sums its column.
#include "readout_head.h"

namespace {

struct RpPools {   // the two row sets and their per-molecule row lists
    const float* x;
    const int* rowptr;
    const float* e;
    const int* e_rowptr;
    const int* e_perm;      // null: identity
    const int64_t* e_order;
    int n_e;
};

template <bool DROP>
struct RpArgs {
    float eps;
};
template <>
struct RpArgs<true> {
    float eps;
    uint32_t thr_x, thr_h;      // drop_threshold(p_x), drop_threshold(p_h); 0 skips the site(s)
    float inv_x, inv_h;         // drop_inv_keep(.)
    const int64_t *seed_x, *seed_e, *seed_h1, *seed_h2;
};
template <bool DROP>
struct RpSites {
    __device__ explicit RpSites(const RpArgs<DROP>&) {}
};
// A site's hash key is derived where a phase needs it (one scalar load of the seed and the 64-bit mix, per wavefront), not once
// for the kernel: four keys held from the pooling phase to the dX / dE phase cost 12 scalar registers across every phase, and
// with them the (C, H) = (256, 256) instantiation spilled scalars.
template <>
struct RpSites<true> {
    const RpArgs<true>& a;
    __device__ explicit RpSites(const RpArgs<true>& a_) : a(a_) {}
    static __device__ __forceinline__ RoSite site(const int64_t* seed, uint32_t thr, float inv) {
        return RoSite{drop_key(thr ? (uint64_t)*seed : 0), thr, inv};
    }
    __device__ __forceinline__ RoSite x() const { return site(a.seed_x, a.thr_x, a.inv_x); }
    __device__ __forceinline__ RoSite e() const { return site(a.seed_e, a.thr_x, a.inv_x); }
    __device__ __forceinline__ RoSite hidden(int layer) const { return site(layer == 1 ? a.seed_h1 : a.seed_h2, a.thr_h, a.inv_h); }
};

// entry q of the hyperedge pool -> its row of E (or -1: a null entry) and whether its order is above 2
__device__ __forceinline__ int rp_he_row(const RpPools& in, int q, bool& high) {
    const int j = in.e_perm ? in.e_perm[q] : q;
    high = false;
    if (j < 0 || j >= in.n_e) return -1;
    high = in.e_order[j] > 2;
    return j;
}

// The sums of the node rows of molecules m0, m0 + 1 -> sOut[0][.], sOut[1][.] (C floats each, rows ld apart).  A row is C/4
// float4 lanes, 64 / (C/4) rows side by side, DEEP deep for both molecules at once; the lane groups are combined by xor
// shuffles, so the order of the sum is fixed.  Molecules >= n_real pool to zero.
template <int C, bool DROP>
__device__ __forceinline__ void rp_pool_nodes(const RpPools& in, int m0, int n_real, const RpSites<DROP>& ks, float* sOut, int ld,
                                              int lane) {
    constexpr int LPR = C / 4, AP = 64 / LPR;
    static_assert(LPR <= 64 && 64 % LPR == 0, "C in {16..256}, power-of-two float4 lanes");
    const int sub = lane / LPR, cl = lane - sub * LPR;
    const float* __restrict__ src = in.x;
    RoSite site{};
    if constexpr (DROP) site = ks.x();
    int beg0 = 0, end0 = 0, beg1 = 0, end1 = 0;
    if (m0 < n_real) { beg0 = in.rowptr[m0]; end0 = in.rowptr[m0 + 1]; }
    if (m0 + 1 < n_real) { beg1 = in.rowptr[m0 + 1]; end1 = in.rowptr[m0 + 2]; }
    float4 acc0 = f4_zero(), acc1 = f4_zero();
    constexpr int DEEP = 8;   // rows in flight per molecule: a QM9 molecule (<= 29 atoms) takes <= 4 rounds
    for (int n0 = beg0 + sub, n1 = beg1 + sub; n0 < end0 || n1 < end1; n0 += DEEP * AP, n1 += DEEP * AP) {
        float4 v0[DEEP], v1[DEEP];
#pragma unroll
        for (int u = 0; u < DEEP; ++u) {
            const int a0 = n0 + u * AP, a1 = n1 + u * AP;
            v0[u] = a0 < end0 ? *reinterpret_cast<const float4*>(src + (int64_t)a0 * C + 4 * cl) : f4_zero();
            v1[u] = a1 < end1 ? *reinterpret_cast<const float4*>(src + (int64_t)a1 * C + 4 * cl) : f4_zero();
        }
#pragma unroll
        for (int u = 0; u < DEEP; ++u) {
            if (n0 + u * AP < end0) {
                if constexpr (DROP) ro_mask4<C>(site, n0 + u * AP, cl, v0[u]);
                f4_add(acc0, v0[u]);
            }
            if (n1 + u * AP < end1) {
                if constexpr (DROP) ro_mask4<C>(site, n1 + u * AP, cl, v1[u]);
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
        *reinterpret_cast<float4*>(sOut + 4 * cl) = acc0;
        *reinterpret_cast<float4*>(sOut + ld + 4 * cl) = acc1;
    }
}

// The sum of the hyperedge rows of order > 2 of ONE molecule -> sOut[0 .. C).  As k_pool_pair_fwd does it: the 64 lanes look
// at 64 entries of the molecule's list side by side (entry -> row -> order: two dependent loads for the whole list, not per
// entry), a ballot leaves the mask of the rows that count -- about one per molecule: a bond is never loaded -- and those are
// added in entry order by the first C/4 lanes, whatever the mask: the sum is bitwise reproducible.
template <int C, bool DROP>
__device__ __forceinline__ void rp_pool_hyperedges(const RpPools& in, int m, int n_real, const RpSites<DROP>& ks, float* sOut,
                                                   int lane) {
    constexpr int LPR = C / 4;
    RoSite site{};
    if constexpr (DROP) site = ks.e();
    int beg = 0, end = 0;
    if (in.n_e > 0 && m < n_real) { beg = in.e_rowptr[m]; end = in.e_rowptr[m + 1]; }   // (n_e == 0: no e pointer is read)
    float4 acc = f4_zero();
    for (int q0 = beg; q0 < end; q0 += 64) {
        bool high = false;
        int j = -1;
        if (q0 + lane < end) j = rp_he_row(in, q0 + lane, high);
        unsigned long long live = __ballot(j >= 0 && high);
        while (live) {
            const int row = __shfl(j, __ffsll((long long)live) - 1);
            live &= live - 1;
            if (lane < LPR) {
                float4 v = *reinterpret_cast<const float4*>(in.e + (int64_t)row * C + 4 * lane);
                if constexpr (DROP) ro_mask4<C>(site, row, lane, v);
                f4_add(acc, v);
            }
        }
    }
    if (lane < LPR) *reinterpret_cast<float4*>(sOut + 4 * lane) = acc;
}

// out[m][n] = sum_k A[m][k] W[n][k]: A in LDS (16 rows, stride lda), W [N][K] row-major in global memory, for this wavefront's
// NT column tiles t = wave + 8 i.  K is walked in chunks of at most 256, so the weights in registers are NT * 64 at most.
template <int K, int NT>
__device__ __forceinline__ void rp_wt_product(const float* sA, int lda, const float* __restrict__ W, float* sOut, int ldo,
                                              int wave, int lane) {
    constexpr int KC = K < 256 ? K : 256;
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += KC) {
        float4 b[NT][KC / 16];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const float* wrow = W + (int64_t)(16 * (wave + RO_WAVES * i) + r) * K + k0 + 4 * q;
#pragma unroll
            for (int s = 0; s < KC / 16; ++s) b[i][s] = *reinterpret_cast<const float4*>(wrow + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < KC / 16; ++s) {
            const float4 a = *reinterpret_cast<const float4*>(sA + r * lda + k0 + 16 * s + 4 * q);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                acc[i] = mfma16(a.x, b[i][s].x, acc[i]);
                acc[i] = mfma16(a.y, b[i][s].y, acc[i]);
                acc[i] = mfma16(a.z, b[i][s].z, acc[i]);
                acc[i] = mfma16(a.w, b[i][s].w, acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * (wave + RO_WAVES * i) + r] = acc[i][g];
}

// out[m][i] = sum_o A[m][o] W[o][i]: A in LDS (stride lda), W [O][I] row-major in global memory, for the NT column tiles
// t = t0 + 8 i
template <int O, int I, int NT>
__device__ __forceinline__ void rp_w_cols_product(const float* sA, int lda, const float* __restrict__ W, float* sOut, int ldo,
                                                  int t0, int lane) {
    const int r = lane & 15, q = lane >> 4;
    float b[NT][O / 4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const float* wcol = W + (int64_t)(4 * q) * I + 16 * (t0 + RO_WAVES * i) + r;
#pragma unroll
        for (int s = 0; s < O / 16; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) b[i][4 * s + j] = wcol[(int64_t)(16 * s + j) * I];
    }
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < O / 16; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(sA + r * lda + 16 * s + 4 * q);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            acc[i] = mfma16(a.x, b[i][4 * s + 0], acc[i]);
            acc[i] = mfma16(a.y, b[i][4 * s + 1], acc[i]);
            acc[i] = mfma16(a.z, b[i][4 * s + 2], acc[i]);
            acc[i] = mfma16(a.w, b[i][4 * s + 3], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * (t0 + RO_WAVES * i) + r] = acc[i][g];
}

// dz = [a > 0] * rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)), dxh = dh * gamma, written OVER a (sAZ: each thread reads and
// writes its own elements).  dh comes from sDH, or (sDH null) dh[m][c] = dy[m] * w3[c] for the last hidden layer.  DROP: dh is
// multiplied by the recomputed keep of hidden site `layer` first, and where it came from sDH the masked value is put back there.
template <int H, bool DROP>
__device__ __forceinline__ void rp_relu_ln_bwd_rows(float* sDH, const float* __restrict__ w3, const float* sDy, float* sAZ,
                                                    const float* sXH, const float* __restrict__ gamma, const float* sRstd,
                                                    int ld, const RpSites<DROP>& ks, int layer, int b0) {
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
            if (sDH) sDH[row * ld + c] = dh;
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
        sAZ[row * ld + c] = sAZ[row * ld + c] > 0.f ? da : 0.f;
    }
}

// this workgroup's [dbias | dgamma | dbeta] (3 H floats): column sums over the 16 rows, in row order.  sDH null: the last
// hidden layer, dh[m][c] = dy[m] w3[c] -- times the keep of hidden site 2 under DROP, as rp_relu_ln_bwd_rows formed it.
template <int H, bool DROP>
__device__ __forceinline__ void rp_ln_param_sums(const float* sDH, const float* __restrict__ w3, const float* sDy,
                                                 const float* sXH, const float* sDZ, int ld, float* __restrict__ out,
                                                 const RpSites<DROP>& ks, int b0) {
    RoSite site{};
    if constexpr (DROP) {
        if (!sDH) site = ks.hidden(2);
    }
    for (int t = threadIdx.x; t < 3 * H; t += RO_THREADS) {
        const int which = t / H, c = t - which * H;
        float s = 0.f;
        if (which == 0) {
            for (int m = 0; m < RO_ROWS; ++m) s += sDZ[m * ld + c];
        } else {
            const float wc = sDH ? 0.f : w3[c];
            for (int m = 0; m < RO_ROWS; ++m) {
                float dh;
                if (sDH) {
                    dh = sDH[m * ld + c];
                } else {
                    dh = sDy[m] * wc;
                    if constexpr (DROP) dh *= ro_keep(site, b0 + m, H, c);
                }
                s += which == 1 ? dh * sXH[m * ld + c] : dh;
            }
        }
        out[t] = s;
    }
}

template <int C, int H>
struct RpLds {
    static constexpr int LX = 2 * C + 4, LH = H + 4, HB = RO_ROWS * LH;
    static constexpr int X = 0, A1 = X + RO_ROWS * LX, XH1 = A1 + HB, H1 = XH1 + HB, A2 = H1 + HB, XH2 = A2 + HB,
                         H2 = XH2 + HB, DH1 = H2 + HB, STAT = DH1 + HB, VEC = STAT + 4 * RO_ROWS,
                         TOTAL = VEC + 7 * H + 4;   // VEC: b1 g1 be1 b2 g2 be2 w3 b3
    static constexpr int DX = H1;   // the pooled gradient [16][LX] over H1 | A2 | XH2 | H2, all dead when it is formed
    static_assert(RO_ROWS * LX <= 4 * HB, "the pooled gradient fits the four H buffers it overwrites");
};

template <int C, int H, bool DROP = false, bool SL1 = false>
__global__ void __launch_bounds__(RO_THREADS)
k_readout_pair_mse(RpPools in, int n_graphs, int n_real, RoWeights w, RoLossArgs<RpArgs<DROP>, SL1> ra,
                   const float* __restrict__ target,
                   float* __restrict__ y, float* __restrict__ loss, float* __restrict__ dX, float* __restrict__ dE,
                   RoSlabs slab, float* __restrict__ loss_part, int* __restrict__ state) {
    using L = RpLds<C, H>;
    constexpr int LX = L::LX, LH = L::LH, K1 = 2 * C;
    constexpr int NT = H / (16 * RO_WAVES);          // H tiles per wavefront: 1 or 2
    static_assert(NT * 16 * RO_WAVES == H && H <= RO_THREADS - 1, "H in {128, 256}");
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* sX = s_mem + L::X;
    float* sA1 = s_mem + L::A1;      // a1, then dZ1
    float* sXH1 = s_mem + L::XH1;
    float* sH1 = s_mem + L::H1;
    float* sA2 = s_mem + L::A2;      // a2, then dZ2
    float* sXH2 = s_mem + L::XH2;
    float* sH2 = s_mem + L::H2;
    float* sDH1 = s_mem + L::DH1;
    float* sDX = s_mem + L::DX;
    float* sR1 = s_mem + L::STAT;
    float* sR2 = sR1 + RO_ROWS;
    float* sDy = sR2 + RO_ROWS;
    float* sSq = sDy + RO_ROWS;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.x * RO_ROWS;
    const bool train = target != nullptr;
    const float eps = ra.eps;

    // ---- the small parameter vectors (to LDS), requested first
    float* sV = s_mem + L::VEC;
    const float *vb1 = sV, *vg1 = sV + H, *vbe1 = sV + 2 * H, *vb2 = sV + 3 * H, *vg2 = sV + 4 * H, *vbe2 = sV + 5 * H,
                *vw3 = sV + 6 * H, *vb3 = sV + 7 * H;
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
    const RpSites<DROP> ks(ra);

    // ---- the two pools of molecules 2 wave, 2 wave + 1: node rows into columns [0, C), hyperedge rows into [C, 2C)
    rp_pool_nodes<C, DROP>(in, b0 + 2 * wave, n_real, ks, sX + (2 * wave) * LX, LX, lane);
    rp_pool_hyperedges<C, DROP>(in, b0 + 2 * wave, n_real, ks, sX + (2 * wave) * LX + C, lane);
    rp_pool_hyperedges<C, DROP>(in, b0 + 2 * wave + 1, n_real, ks, sX + (2 * wave + 1) * LX + C, lane);
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = threadIdx.x + k * RO_THREADS;
        if (i < 7 * H) sV[i] = vreg[k];
    }
    if (threadIdx.x == 0) sV[7 * H] = vb3_reg;
    __syncthreads();

    // ---- forward
    rp_wt_product<K1, NT>(sX, LX, w.w1, sA1, LH, wave, lane);
    __syncthreads();
    ro_relu_ln_rows<H, DROP>(sA1, vb1, vg1, vbe1, sXH1, sH1, sR1, LH, eps, ks, 1, b0);
    __syncthreads();
    rp_wt_product<H, NT>(sH1, LH, w.w2, sA2, LH, wave, lane);
    __syncthreads();
    ro_relu_ln_rows<H, DROP>(sA2, vb2, vg2, vbe2, sXH2, sH2, sR2, LH, eps, ks, 2, b0);
    __syncthreads();
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
    if (!train) return;

    // ---- backward
    const int64_t wg = blockIdx.x;
    rp_relu_ln_bwd_rows<H, DROP>(nullptr, vw3, sDy, sA2, sXH2, vg2, sR2, LH, ks, 2, b0);      // a2 -> dZ2
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
    rp_w_cols_product<H, H, NT>(sA2, LH, w.w2, sDH1, LH, wave, lane);                          // dh1 = dZ2 W2
    rp_ln_param_sums<H, DROP>(nullptr, vw3, sDy, sXH2, sA2, LH, slab.v2 + wg * 3 * H, ks, b0);
    ro_outer_rows<H, H>(sA2, LH, sH1, LH, slab.w2 + wg * H * H, wave, lane);
    __syncthreads();
    rp_relu_ln_bwd_rows<H, DROP>(sDH1, nullptr, nullptr, sA1, sXH1, vg1, sR1, LH, ks, 1, b0);  // a1 -> dZ1
    __syncthreads();
    {   // the pooled gradient dZ1 W1 [16][2C]: K1 / 16 column tiles, 1, 2 or 4 per wavefront, two at a time
        constexpr int TPW = K1 / (16 * RO_WAVES), NTX = TPW < 2 ? TPW : 2;
        static_assert(TPW * 16 * RO_WAVES == K1, "2C a multiple of 128");
#pragma unroll 1
        for (int g = 0; g < TPW / NTX; ++g)
            rp_w_cols_product<H, K1, NTX>(sA1, LH, w.w1, sDX, LX, wave + RO_WAVES * NTX * g, lane);
    }
    __syncthreads();

    // ---- dX[n, :] = dz[molecule(n), 0:C], dE[m, :] = dz[molecule(m), C:2C] or zero for order <= 2 (zero rows for the padding
    // molecules b >= n_real: their dy is 0); DROP: times the pre-pool keep of the row
    {
        constexpr int LPR = C / 4, AP = 64 / LPR;
        const int sub = lane / LPR, cl = lane - sub * LPR;
        RoSite site_x{}, site_e{};
        if constexpr (DROP) { site_x = ks.x(); site_e = ks.e(); }
        for (int mi = 2 * wave; mi < 2 * wave + 2; ++mi) {
            const int b = b0 + mi;
            if (b >= n_graphs) continue;
            const float4 gx = *reinterpret_cast<const float4*>(sDX + mi * LX + 4 * cl);
            const int beg = in.rowptr[b], end = in.rowptr[b + 1];
            for (int n = beg + sub; n < end; n += AP) {
                float4 gn = gx;
                if constexpr (DROP) ro_mask4<C>(site_x, n, cl, gn);
                *reinterpret_cast<float4*>(dX + (int64_t)n * C + 4 * cl) = gn;
            }
            if (in.n_e <= 0) continue;
            const float4 ge = *reinterpret_cast<const float4*>(sDX + mi * LX + C + 4 * cl);
            const int ebeg = in.e_rowptr[b], eend = in.e_rowptr[b + 1];
            for (int q0 = ebeg; q0 < eend; q0 += 64) {      // 64 entries side by side (entry -> row -> order), then AP rows at a time
                bool high = false;
                int j = -1;
                if (q0 + lane < eend) j = rp_he_row(in, q0 + lane, high);
                const int cnt = eend - q0 < 64 ? eend - q0 : 64;
                for (int i0 = 0; i0 < cnt; i0 += AP) {        // (uniform trip count: every lane takes part in the shuffles)
                    const int i = i0 + sub;
                    const int ji = __shfl(j, i & 63), hi = __shfl((int)high, i & 63);
                    if (i >= cnt || ji < 0) continue;
                    float4 gm = f4_zero();
                    if (hi) {
                        gm = ge;
                        if constexpr (DROP) ro_mask4<C>(site_e, ji, cl, gm);
                    }
                    *reinterpret_cast<float4*>(dE + (int64_t)ji * C + 4 * cl) = gm;
                }
            }
        }
    }

    // ---- the two large gradient slabs last: nothing in this kernel waits for them
    rp_ln_param_sums<H, DROP>(sDH1, nullptr, nullptr, sXH1, sA1, LH, slab.v1 + wg * 3 * H, ks, b0);
    ro_outer_rows<H, K1>(sA1, LH, sX, LX, slab.w1 + wg * (int64_t)H * K1, wave, lane);

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
int rp_launch(const RpPools& in, int n_graphs, int n_real, const RoWeights& w, const RoLossArgs<RpArgs<DROP>, SL1>& ra,
              const float* target, float* y, float* loss, float* dx, float* de, const RoSlabs& slab, float* loss_part, int* state, int n_wg,
              hipStream_t stream) {
    constexpr size_t lds = (size_t)RpLds<C, H>::TOTAL * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_readout_pair_mse<C, H, DROP, SL1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return EQH_ERR_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_readout_pair_mse<C, H, DROP, SL1>), dim3(n_wg), dim3(RO_THREADS), lds, stream, in, n_graphs, n_real, w, ra,
                       target, y, loss, dx, de, slab, loss_part, state);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

}  // namespace

extern "C" int hg_readout_pair_mse_supported(int32_t C, int32_t H) {
    return (C == 64 || C == 128 || C == 256) && (H == 128 || H == 256);
}

extern "C" size_t hg_readout_pair_mse_workspace_bytes(int32_t n_graphs, int32_t C, int32_t H) {
    if (n_graphs <= 0 || !hg_readout_pair_mse_supported(C, H)) return 0;
    return ro_plan(n_graphs, 2 * C, H).total * sizeof(float);
}

namespace {

// hg_readout_pair_mse_f32 (DROP = false) and hg_readout_pair_mse_drop_f32 (DROP = true), and their hg_readout_pair_sl1_* twins
// (SL1 = true): one host function
template <bool DROP, bool SL1>
int readout_pair_mse(const RpPools& in, int32_t n_graphs, int32_t n_real, int32_t C, int32_t H, const float* const* weights,
                     const RoLossArgs<RpArgs<DROP>, SL1>& ra, const float* target, float* y, float* loss, float* dx, float* de,
                     float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes, int32_t* state,
                     void* stream_) {
    if (n_graphs < 0 || n_real < 0 || n_real > n_graphs || in.n_e < 0 || !hg_readout_pair_mse_supported(C, H))
        return EQH_ERR_ARG;
    if (n_graphs == 0) return EQH_OK;
    const RoPlan p = ro_plan(n_graphs, 2 * C, H);
    int rc = ro_check_args(!in.x || !in.rowptr || !y || (in.n_e > 0 && (!in.e || !in.e_rowptr || !in.e_order)),
                           !eqh_aligned16(in.x) || !eqh_aligned16(in.e), weights, target, n_real, !dx || (in.n_e > 0 && !de),
                           !eqh_aligned16(dx) || !eqh_aligned16(de), loss, dweights, workspace, workspace_bytes,
                           p.total * sizeof(float), state);
    if (rc) return rc;
    const bool train = target != nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* ws = static_cast<float*>(workspace);
    const RoWeights w = ro_weights(weights);
    const RoSlabs slab = ro_slabs(ws, p, train);
    float* loss_part = train ? ws + p.off_loss : nullptr;
    rc = EQH_ERR_ARG;
#define RP_CASE(CC, HH)                                                                                               \
    if (C == CC && H == HH)                                                                                           \
        rc = rp_launch<CC, HH, DROP, SL1>(in, n_graphs, n_real, w, ra, target, y, loss, dx, de, slab, loss_part, state, p.n_wg, \
                                     stream);
    RP_CASE(64, 128) RP_CASE(64, 256) RP_CASE(128, 128) RP_CASE(128, 256) RP_CASE(256, 128) RP_CASE(256, 256)
#undef RP_CASE
    if (rc || !train) return rc;
    return ro_reduce_head_slabs(slab, p, 2 * C, H, dweights, ws + p.off_discard, accumulate, stream);
}

}  // namespace

extern "C" int hg_readout_pair_mse_f32(const float* x, const int32_t* rowptr, const float* e, const int32_t* e_rowptr,
                                       const int32_t* e_perm, const int64_t* e_order, int32_t n_e, int32_t n_graphs,
                                       int32_t n_real, int32_t C, int32_t H, const float* const* weights, float eps,
                                       const float* target, float* y, float* loss, float* dx, float* de,
                                       float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                       int32_t* state, void* stream_) {
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<false, false>(in, n_graphs, n_real, C, H, weights, RpArgs<false>{eps}, target, y, loss, dx, de, dweights,
                                   accumulate, workspace, workspace_bytes, state, stream_);
}

extern "C" int hg_readout_pair_mse_drop_f32(const float* x, const int32_t* rowptr, const float* e, const int32_t* e_rowptr,
                                            const int32_t* e_perm, const int64_t* e_order, int32_t n_e, int32_t n_graphs,
                                            int32_t n_real, int32_t C, int32_t H, const float* const* weights, float eps,
                                            const float* target, float* y, float* loss, float* dx, float* de,
                                            float* const* dweights, int32_t accumulate, void* workspace,
                                            size_t workspace_bytes, int32_t* state, float p_x, float p_h,
                                            const int64_t* seed_x, const int64_t* seed_e, const int64_t* seed_h1,
                                            const int64_t* seed_h2, void* stream_) {
    if (int rc = ro_check_drop(p_x, p_h, seed_x && seed_e, seed_h1 && seed_h2)) return rc;
    const RpArgs<true> ra{eps, drop_threshold(p_x), drop_threshold(p_h), drop_inv_keep(p_x), drop_inv_keep(p_h),
                          seed_x, seed_e, seed_h1, seed_h2};
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<true, false>(in, n_graphs, n_real, C, H, weights, ra, target, y, loss, dx, de, dweights, accumulate,
                                  workspace, workspace_bytes, state, stream_);
}

// The same two launches with the loss family of loss_family.h in the place of the squared error (SL1 forms of the kernel):
// beta >= 0 and scale > 0, both finite, checked with the entry's own arguments ahead of any launch.
extern "C" int hg_readout_pair_sl1_f32(const float* x, const int32_t* rowptr, const float* e, const int32_t* e_rowptr,
                                       const int32_t* e_perm, const int64_t* e_order, int32_t n_e, int32_t n_graphs,
                                       int32_t n_real, int32_t C, int32_t H, const float* const* weights, float eps,
                                       const float* target, float* y, float* loss, float* dx, float* de,
                                       float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                       int32_t* state, float beta, float scale, void* stream_) {
    if (!sl1_args_ok(beta, scale)) return EQH_ERR_ARG;
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<false, true>(in, n_graphs, n_real, C, H, weights, ro_sl1_args(RpArgs<false>{eps}, beta, scale),
                                         target, y, loss, dx, de, dweights, accumulate, workspace, workspace_bytes, state,
                                         stream_);
}

extern "C" int hg_readout_pair_sl1_drop_f32(const float* x, const int32_t* rowptr, const float* e, const int32_t* e_rowptr,
                                            const int32_t* e_perm, const int64_t* e_order, int32_t n_e, int32_t n_graphs,
                                            int32_t n_real, int32_t C, int32_t H, const float* const* weights, float eps,
                                            const float* target, float* y, float* loss, float* dx, float* de,
                                            float* const* dweights, int32_t accumulate, void* workspace,
                                            size_t workspace_bytes, int32_t* state, float p_x, float p_h,
                                            const int64_t* seed_x, const int64_t* seed_e, const int64_t* seed_h1,
                                            const int64_t* seed_h2, float beta, float scale, void* stream_) {
    if (!sl1_args_ok(beta, scale)) return EQH_ERR_ARG;
    if (int rc = ro_check_drop(p_x, p_h, seed_x && seed_e, seed_h1 && seed_h2)) return rc;
    const RpArgs<true> ra{eps, drop_threshold(p_x), drop_threshold(p_h), drop_inv_keep(p_x), drop_inv_keep(p_h),
                          seed_x, seed_e, seed_h1, seed_h2};
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<true, true>(in, n_graphs, n_real, C, H, weights, ro_sl1_args(ra, beta, scale), target, y, loss, dx,
                                        de, dweights, accumulate, workspace, workspace_bytes, state, stream_);
}
