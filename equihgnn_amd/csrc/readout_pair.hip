// Readout head of the paired tail (models._PairedBase: mhnn, egnn_equihnn, faformer_equihnn, visnet_equihnn), forward + loss +
// complete backward in ONE launch -- k_readout_mse of readout.hip for a head whose input is two pools side by side:
//
//   z_b   = [ sum_{n in molecule b} X[n, :] | sum_{m in molecule b, e_order[m] > 2} E[m, :] ]     mhnn.py:58,72 ([B, 2C])
//   h1    = LN1(relu(W1 z + b1)),  h2 = LN2(relu(W2 h1 + b2))     MLP(2C -> H -> H -> 1), H = 2 output_hidden, mlp.py:91-99
//   y_b   = w3 . h2 + b3,   loss = mean_{b < n_real} (y_b - t_b)^2
//
// As in readout.hip one workgroup of 512 threads owns 16 molecules (the M of the fp32 16 x 16 x 4 MFMA), the activations stay
// in LDS, every workgroup leaves one slab of every parameter gradient for the library's fixed-order reducer (deferred into the
// step's batched reduction when that is active), and nothing is atomic: the launch is bitwise reproducible.  What differs:
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
// MFMA operand convention: that of readout.hip (lane l: r = l & 15, q = l >> 4; four MFMAs share one float4 of K).
//
// Training dropout (template flag DROP, entry hg_readout_pair_mse_drop_f32): up to FOUR sites, keep = 0 or 1 / (1 - p) from
// drop_hash.h, seeds in device memory, nothing stored -- the elements and the draw order of the launches this one replaces
// (_drop(x), _drop(e) after the last conv application, then the head's two hg_bias_relu_ln_drop_fwd):
//   pre-pool x (p_x)  element n C + c of X [N, C];   pre-pool e (p_x)  element m C + c of E [M, C];
//   hidden 1, 2 (p_h) element b H + c, b the global molecule row.  LDS holds the masked h_i.  The masked dh1 stays in the dH1
//   buffer for layer 1's dgamma / dbeta; layer 2's masked dh2 = keep . dy w3 has no buffer of its own and is recomputed (one
//   hash per element) by the thread that sums its column.
#include "common.h"
#include "drop_hash.h"
#include "mfma.h"

namespace {

constexpr int RP_THREADS = 512;
constexpr int RP_WAVES = RP_THREADS / 64;
constexpr int RP_ROWS = 16;  // molecules per workgroup = the M of one MFMA tile

struct RpWeights {
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3;
};
struct RpSlabs {   // per-workgroup partial gradients: [n_wg][H*2C], [n_wg][H*H], [n_wg][3H] x 2, [n_wg][H+4]
    float *w1, *w2, *v1, *v2, *v3;
};
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
struct RpSite {
    DropKey key;
    uint32_t thr;
    float inv;
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
    static __device__ __forceinline__ RpSite site(const int64_t* seed, uint32_t thr, float inv) {
        return RpSite{drop_key(thr ? (uint64_t)*seed : 0), thr, inv};
    }
    __device__ __forceinline__ RpSite x() const { return site(a.seed_x, a.thr_x, a.inv_x); }
    __device__ __forceinline__ RpSite e() const { return site(a.seed_e, a.thr_x, a.inv_x); }
    __device__ __forceinline__ RpSite hidden(int layer) const { return site(layer == 1 ? a.seed_h1 : a.seed_h2, a.thr_h, a.inv_h); }
};
// keep-scale of element row * H + c of a hidden site (the aligned pair that holds c, its half: keep_scale2's contract)
__device__ __forceinline__ float rp_keep(const RpSite& s, int64_t row, int H, int c) {
    float k0, k1;
    keep_scale2(s.key, (uint64_t)row * (uint64_t)H + (uint64_t)(c & ~1), s.thr, s.inv, k0, k1);
    return (c & 1) ? k1 : k0;
}
// v *= keep of the float4 at row n, columns 4 cl .. 4 cl + 3 of [rows, C] (a pre-pool site; C % 4 == 0)
template <int C>
__device__ __forceinline__ void rp_mask4(const RpSite& s, int n, int cl, float4& v) {
    if (s.thr) keep_scale4(s.key, (uint64_t)n * (uint64_t)C + (uint64_t)(4 * cl), s.thr, s.inv, v);
}

// sum over the 32 lanes that share a row
__device__ __forceinline__ float rp_half_sum(float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

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
    RpSite site{};
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
                if constexpr (DROP) rp_mask4<C>(site, n0 + u * AP, cl, v0[u]);
                f4_add(acc0, v0[u]);
            }
            if (n1 + u * AP < end1) {
                if constexpr (DROP) rp_mask4<C>(site, n1 + u * AP, cl, v1[u]);
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
    RpSite site{};
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
                if constexpr (DROP) rp_mask4<C>(site, row, lane, v);
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
            const float* wrow = W + (int64_t)(16 * (wave + RP_WAVES * i) + r) * K + k0 + 4 * q;
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
        for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * (wave + RP_WAVES * i) + r] = acc[i][g];
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
        const float* wcol = W + (int64_t)(4 * q) * I + 16 * (t0 + RP_WAVES * i) + r;
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
        for (int g = 0; g < 4; ++g) sOut[(4 * q + g) * ldo + 16 * (t0 + RP_WAVES * i) + r] = acc[i][g];
}

// out[o][i] = sum_{m < 16} D[m][o] In[m][i] (both in LDS) -> this workgroup's slab [O][I] in global memory
template <int O, int I>
__device__ __forceinline__ void rp_outer_rows(const float* sD, int ldd, const float* sIn, int ldi, float* __restrict__ out,
                                              int wave, int lane) {
    const int r = lane & 15, q = lane >> 4;
    for (int t = wave; t < (O / 16) * (I / 16); t += RP_WAVES) {
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
template <int H, bool DROP>
__device__ __forceinline__ void rp_relu_ln_rows(float* sZ, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float* sXH, float* sH, float* sRstd, int ld,
                                                float eps, const RpSites<DROP>& ks, int layer, int b0) {
    constexpr int CPT = H / 32;
    const int row = threadIdx.x >> 5, l = threadIdx.x & 31;
    RpSite site{};
    if constexpr (DROP) site = ks.hidden(layer);
    float a[CPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        a[j] = fmaxf(sZ[row * ld + c] + bias[c], 0.f);
        s += a[j];
    }
    const float mu = rp_half_sum(s) * (1.0f / H);
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) v = fmaf(a[j] - mu, a[j] - mu, v);
    const float rstd = 1.0f / sqrtf(rp_half_sum(v) * (1.0f / H) + eps);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        const float xh = (a[j] - mu) * rstd;
        sZ[row * ld + c] = a[j];
        sXH[row * ld + c] = xh;
        if constexpr (DROP)
            sH[row * ld + c] = fmaf(xh, gamma[c], beta[c]) * rp_keep(site, b0 + row, H, c);
        else
            sH[row * ld + c] = fmaf(xh, gamma[c], beta[c]);
    }
    if (l == 0) sRstd[row] = rstd;
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
    RpSite site{};
    if constexpr (DROP) site = ks.hidden(layer);
    float dxh[CPT], xh[CPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = l + 32 * j;
        float dh = sDH ? sDH[row * ld + c] : sDy[row] * w3[c];
        if constexpr (DROP) {
            dh *= rp_keep(site, b0 + row, H, c);
            if (sDH) sDH[row * ld + c] = dh;
        }
        xh[j] = sXH[row * ld + c];
        dxh[j] = dh * gamma[c];
        s1 += dxh[j];
        s2 = fmaf(dxh[j], xh[j], s2);
    }
    s1 = rp_half_sum(s1) * (1.0f / H);
    s2 = rp_half_sum(s2) * (1.0f / H);
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
    RpSite site{};
    if constexpr (DROP) {
        if (!sDH) site = ks.hidden(2);
    }
    for (int t = threadIdx.x; t < 3 * H; t += RP_THREADS) {
        const int which = t / H, c = t - which * H;
        float s = 0.f;
        if (which == 0) {
            for (int m = 0; m < RP_ROWS; ++m) s += sDZ[m * ld + c];
        } else {
            const float wc = sDH ? 0.f : w3[c];
            for (int m = 0; m < RP_ROWS; ++m) {
                float dh;
                if (sDH) {
                    dh = sDH[m * ld + c];
                } else {
                    dh = sDy[m] * wc;
                    if constexpr (DROP) dh *= rp_keep(site, b0 + m, H, c);
                }
                s += which == 1 ? dh * sXH[m * ld + c] : dh;
            }
        }
        out[t] = s;
    }
}

template <int C, int H>
struct RpLds {
    static constexpr int LX = 2 * C + 4, LH = H + 4, HB = RP_ROWS * LH;
    static constexpr int X = 0, A1 = X + RP_ROWS * LX, XH1 = A1 + HB, H1 = XH1 + HB, A2 = H1 + HB, XH2 = A2 + HB,
                         H2 = XH2 + HB, DH1 = H2 + HB, STAT = DH1 + HB, VEC = STAT + 4 * RP_ROWS,
                         TOTAL = VEC + 7 * H + 4;   // VEC: b1 g1 be1 b2 g2 be2 w3 b3
    static constexpr int DX = H1;   // the pooled gradient [16][LX] over H1 | A2 | XH2 | H2, all dead when it is formed
    static_assert(RP_ROWS * LX <= 4 * HB, "the pooled gradient fits the four H buffers it overwrites");
};

template <int C, int H, bool DROP = false>
__global__ void __launch_bounds__(RP_THREADS)
k_readout_pair_mse(RpPools in, int n_graphs, int n_real, RpWeights w, RpArgs<DROP> ra, const float* __restrict__ target,
                   float* __restrict__ y, float* __restrict__ loss, float* __restrict__ dX, float* __restrict__ dE,
                   RpSlabs slab, float* __restrict__ loss_part, int* __restrict__ state) {
    using L = RpLds<C, H>;
    constexpr int LX = L::LX, LH = L::LH, K1 = 2 * C;
    constexpr int NT = H / (16 * RP_WAVES);          // H tiles per wavefront: 1 or 2
    static_assert(NT * 16 * RP_WAVES == H && H <= RP_THREADS - 1, "H in {128, 256}");
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
    float* sR2 = sR1 + RP_ROWS;
    float* sDy = sR2 + RP_ROWS;
    float* sSq = sDy + RP_ROWS;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.x * RP_ROWS;
    const bool train = target != nullptr;
    const float eps = ra.eps;

    // ---- the small parameter vectors (to LDS), requested first
    float* sV = s_mem + L::VEC;
    const float *vb1 = sV, *vg1 = sV + H, *vbe1 = sV + 2 * H, *vb2 = sV + 3 * H, *vg2 = sV + 4 * H, *vbe2 = sV + 5 * H,
                *vw3 = sV + 6 * H, *vb3 = sV + 7 * H;
    constexpr int VPT = (7 * H + RP_THREADS - 1) / RP_THREADS;
    float vreg[VPT];
    {
        const float* src[7] = {w.b1, w.g1, w.be1, w.b2, w.g2, w.be2, w.w3};
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int i = threadIdx.x + k * RP_THREADS;
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
        const int i = threadIdx.x + k * RP_THREADS;
        if (i < 7 * H) sV[i] = vreg[k];
    }
    if (threadIdx.x == 0) sV[7 * H] = vb3_reg;
    __syncthreads();

    // ---- forward
    rp_wt_product<K1, NT>(sX, LX, w.w1, sA1, LH, wave, lane);
    __syncthreads();
    rp_relu_ln_rows<H, DROP>(sA1, vb1, vg1, vbe1, sXH1, sH1, sR1, LH, eps, ks, 1, b0);
    __syncthreads();
    rp_wt_product<H, NT>(sH1, LH, w.w2, sA2, LH, wave, lane);
    __syncthreads();
    rp_relu_ln_rows<H, DROP>(sA2, vb2, vg2, vbe2, sXH2, sH2, sR2, LH, eps, ks, 2, b0);
    __syncthreads();
    {
        constexpr int CPT = H / 32;
        const int row = threadIdx.x >> 5, l = threadIdx.x & 31;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; ++j) s = fmaf(sH2[row * LH + l + 32 * j], vw3[l + 32 * j], s);
        s = rp_half_sum(s) + vb3[0];
        if (l == 0) {
            const int b = b0 + row;
            if (b < n_graphs) y[b] = s;
            float dy = 0.f, sq = 0.f;
            if (train && b < n_real) {
                const float d = s - target[b];
                dy = 2.0f * d / (float)n_real;
                sq = d * d;
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
    {   // dw3 | db3 | pad, and the squared-error partial (row order)
        float* v3 = slab.v3 + wg * (H + 4);
        const int t = threadIdx.x;
        if (t < H) {
            float s = 0.f;
            for (int m = 0; m < RP_ROWS; ++m) s = fmaf(sDy[m], sH2[m * LH + t], s);
            v3[t] = s;
        } else if (t == H) {
            float s = 0.f, e = 0.f;
            for (int m = 0; m < RP_ROWS; ++m) { s += sDy[m]; e += sSq[m]; }
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
    rp_outer_rows<H, H>(sA2, LH, sH1, LH, slab.w2 + wg * H * H, wave, lane);
    __syncthreads();
    rp_relu_ln_bwd_rows<H, DROP>(sDH1, nullptr, nullptr, sA1, sXH1, vg1, sR1, LH, ks, 1, b0);  // a1 -> dZ1
    __syncthreads();
    {   // the pooled gradient dZ1 W1 [16][2C]: K1 / 16 column tiles, 1, 2 or 4 per wavefront, two at a time
        constexpr int TPW = K1 / (16 * RP_WAVES), NTX = TPW < 2 ? TPW : 2;
        static_assert(TPW * 16 * RP_WAVES == K1, "2C a multiple of 128");
#pragma unroll 1
        for (int g = 0; g < TPW / NTX; ++g)
            rp_w_cols_product<H, K1, NTX>(sA1, LH, w.w1, sDX, LX, wave + RP_WAVES * NTX * g, lane);
    }
    __syncthreads();

    // ---- dX[n, :] = dz[molecule(n), 0:C], dE[m, :] = dz[molecule(m), C:2C] or zero for order <= 2 (zero rows for the padding
    // molecules b >= n_real: their dy is 0); DROP: times the pre-pool keep of the row
    {
        constexpr int LPR = C / 4, AP = 64 / LPR;
        const int sub = lane / LPR, cl = lane - sub * LPR;
        RpSite site_x{}, site_e{};
        if constexpr (DROP) { site_x = ks.x(); site_e = ks.e(); }
        for (int mi = 2 * wave; mi < 2 * wave + 2; ++mi) {
            const int b = b0 + mi;
            if (b >= n_graphs) continue;
            const float4 gx = *reinterpret_cast<const float4*>(sDX + mi * LX + 4 * cl);
            const int beg = in.rowptr[b], end = in.rowptr[b + 1];
            for (int n = beg + sub; n < end; n += AP) {
                float4 gn = gx;
                if constexpr (DROP) rp_mask4<C>(site_x, n, cl, gn);
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
                        if constexpr (DROP) rp_mask4<C>(site_e, ji, cl, gm);
                    }
                    *reinterpret_cast<float4*>(dE + (int64_t)ji * C + 4 * cl) = gm;
                }
            }
        }
    }

    // ---- the two large gradient slabs last: nothing in this kernel waits for them
    rp_ln_param_sums<H, DROP>(sDH1, nullptr, nullptr, sXH1, sA1, LH, slab.v1 + wg * 3 * H, ks, b0);
    rp_outer_rows<H, K1>(sA1, LH, sX, LX, slab.w1 + wg * (int64_t)H * K1, wave, lane);

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

struct RpPlan {
    int n_wg;
    size_t off_w1, off_w2, off_v1, off_v2, off_v3, off_loss, off_discard, total;   // in floats
};

RpPlan rp_plan(int n_graphs, int C, int H) {
    RpPlan p;
    p.n_wg = (n_graphs + RP_ROWS - 1) / RP_ROWS;
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
    p.off_w1 = take((size_t)p.n_wg * H * 2 * C);
    p.off_w2 = take((size_t)p.n_wg * H * H);
    p.off_v1 = take((size_t)p.n_wg * 3 * H);
    p.off_v2 = take((size_t)p.n_wg * 3 * H);
    p.off_v3 = take((size_t)p.n_wg * (H + 4));
    p.off_loss = take((size_t)p.n_wg);
    p.off_discard = take(4);
    p.total = o;
    return p;
}

template <int C, int H, bool DROP>
int rp_launch(const RpPools& in, int n_graphs, int n_real, const RpWeights& w, const RpArgs<DROP>& ra, const float* target,
              float* y, float* loss, float* dx, float* de, const RpSlabs& slab, float* loss_part, int* state, int n_wg,
              hipStream_t stream) {
    constexpr size_t lds = (size_t)RpLds<C, H>::TOTAL * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_readout_pair_mse<C, H, DROP>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return EQH_ERR_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL((k_readout_pair_mse<C, H, DROP>), dim3(n_wg), dim3(RP_THREADS), lds, stream, in, n_graphs, n_real, w, ra,
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
    return rp_plan(n_graphs, C, H).total * sizeof(float);
}

namespace {

// hg_readout_pair_mse_f32 (DROP = false) and hg_readout_pair_mse_drop_f32 (DROP = true): one host function
template <bool DROP>
int readout_pair_mse(const RpPools& in, int32_t n_graphs, int32_t n_real, int32_t C, int32_t H, const float* const* weights,
                     const RpArgs<DROP>& ra, const float* target, float* y, float* loss, float* dx, float* de,
                     float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes, int32_t* state,
                     void* stream_) {
    if (n_graphs < 0 || n_real < 0 || n_real > n_graphs || in.n_e < 0 || !hg_readout_pair_mse_supported(C, H))
        return EQH_ERR_ARG;
    if (n_graphs == 0) return EQH_OK;
    if (!in.x || !in.rowptr || !weights || !y) return EQH_ERR_ARG;
    if (in.n_e > 0 && (!in.e || !in.e_rowptr || !in.e_order)) return EQH_ERR_ARG;
    for (int i = 0; i < 10; ++i)
        if (!weights[i]) return EQH_ERR_ARG;
    if (!eqh_aligned16(in.x) || !eqh_aligned16(in.e) || !eqh_aligned16(weights[0]) || !eqh_aligned16(weights[4]))
        return EQH_ERR_ALIGN;
    const bool train = target != nullptr;
    if (train) {
        if (n_real == 0 || !loss || !dx || (in.n_e > 0 && !de) || !dweights || !workspace || !state) return EQH_ERR_ARG;
        for (int i = 0; i < 10; ++i)
            if (!dweights[i]) return EQH_ERR_ARG;
        if (!eqh_aligned16(dx) || !eqh_aligned16(de) || !eqh_aligned16(workspace)) return EQH_ERR_ALIGN;
        if (workspace_bytes < hg_readout_pair_mse_workspace_bytes(n_graphs, C, H)) return EQH_ERR_ARG;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const RpPlan p = rp_plan(n_graphs, C, H);
    float* ws = static_cast<float*>(workspace);
    RpWeights w{weights[0], weights[1], weights[2], weights[3], weights[4],
                weights[5], weights[6], weights[7], weights[8], weights[9]};
    RpSlabs slab{nullptr, nullptr, nullptr, nullptr, nullptr};
    float* loss_part = nullptr;
    if (train) {
        slab = RpSlabs{ws + p.off_w1, ws + p.off_w2, ws + p.off_v1, ws + p.off_v2, ws + p.off_v3};
        loss_part = ws + p.off_loss;
    }
    int rc = EQH_ERR_ARG;
#define RP_CASE(CC, HH)                                                                                               \
    if (C == CC && H == HH)                                                                                           \
        rc = rp_launch<CC, HH, DROP>(in, n_graphs, n_real, w, ra, target, y, loss, dx, de, slab, loss_part, state, p.n_wg, \
                                     stream);
    RP_CASE(64, 128) RP_CASE(64, 256) RP_CASE(128, 128) RP_CASE(128, 256) RP_CASE(256, 128) RP_CASE(256, 256)
#undef RP_CASE
    if (rc || !train) return rc;
    // parameter gradients: fixed-order sums over the workgroup slabs (deferred into the step's batched
    // reduction when that is active)
    rc = eqh_reduce_slabs_async(slab.w1, p.n_wg, (int64_t)H * 2 * C, dweights[0], stream, accumulate);
    if (rc) return rc;
    rc = eqh_reduce_slabs_async(slab.w2, p.n_wg, (int64_t)H * H, dweights[4], stream, accumulate);
    if (rc) return rc;
    rc = eqh_reduce_slabs3_async(slab.v1, p.n_wg, 3 * (int64_t)H, dweights[1], dweights[2], dweights[3], H, H, accumulate,
                                 stream);
    if (rc) return rc;
    rc = eqh_reduce_slabs3_async(slab.v2, p.n_wg, 3 * (int64_t)H, dweights[5], dweights[6], dweights[7], H, H, accumulate,
                                 stream);
    if (rc) return rc;
    return eqh_reduce_slabs3_async(slab.v3, p.n_wg, (int64_t)H + 4, dweights[8], dweights[9], ws + p.off_discard, H, 1,
                                   accumulate, stream);
}

}  // namespace

extern "C" int hg_readout_pair_mse_f32(const float* x, const int32_t* rowptr, const float* e, const int32_t* e_rowptr,
                                       const int32_t* e_perm, const int64_t* e_order, int32_t n_e, int32_t n_graphs,
                                       int32_t n_real, int32_t C, int32_t H, const float* const* weights, float eps,
                                       const float* target, float* y, float* loss, float* dx, float* de,
                                       float* const* dweights, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                       int32_t* state, void* stream_) {
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<false>(in, n_graphs, n_real, C, H, weights, RpArgs<false>{eps}, target, y, loss, dx, de, dweights,
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
    // 0 <= p < 1 (a NaN fails the comparison), checked first; a call without an active site belongs to hg_readout_pair_mse_f32
    if (!(p_x >= 0.f && p_x < 1.f) || !(p_h >= 0.f && p_h < 1.f) || (p_x == 0.f && p_h == 0.f)) return EQH_ERR_ARG;
    if ((p_x > 0.f && (!seed_x || !seed_e)) || (p_h > 0.f && (!seed_h1 || !seed_h2))) return EQH_ERR_ARG;
    const RpArgs<true> ra{eps, drop_threshold(p_x), drop_threshold(p_h), drop_inv_keep(p_x), drop_inv_keep(p_h),
                          seed_x, seed_e, seed_h1, seed_h2};
    const RpPools in{x, rowptr, e, e_rowptr, e_perm, e_order, n_e};
    return readout_pair_mse<true>(in, n_graphs, n_real, C, H, weights, ra, target, y, loss, dx, de, dweights, accumulate,
                                  workspace, workspace_bytes, state, stream_);
}
