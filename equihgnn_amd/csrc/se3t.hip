// SE(3)-Transformer front-end (se3_transformer_layer.py as equihnn_se3_transformer.py:37-45 configures it): edge basis,
// the radial contraction of one PairwiseConv re-associated, the 17-slot attention and NormSE3.
//
// The radial contraction.  As written (se3_transformer_layer.py:357-374, 283-288) every edge gets
//   R_e = reshape(W3 h_e + b3) [O, I, F],  kernel_e[(o, mo), (i, mi)] = sum_f R_e[o, i, f] B_e[mo, mi, f],
//   out_e[o, mo] = sum_(i, mi) kernel_e x_j[i, mi]
// with h_e [128] the radial trunk, B_e the basis and x_j the sender's features: F I O 128 multiply-adds and as many floats per
// edge.  Summing over i first gives a NODE-level product
//   G_j[q = (mi, f), c, o] = sum_i W3[(o, i, f), c] x_j[i, mi]        (a plain GEMM, [N mi, I] . [I, F 128 O])
//   out_e[mo, o] = sum_q B_e[mo, q] ( sum_c h_e[c] G_j[q, c, o] + GB_j[q, o] ),   GB_j = the same with b3 for W3
// and what is left per edge is a row product grouped by SENDER (the transposed neighbour CSR): the edges of sender j are
// the rows of a [deg, Q 128] operand B_e[mo, q] h_e[c] (formed in registers) against j's [Q 128, O] matrix, once per output
// component mo.  fp32 MFMA 16x16x4 as in rowgemm.hip; 16 edges per tile, 64 output columns per pass (four column tiles fed by
// one float4 of the node matrix).  Features are component-major: [*, m, C].
//
// Backward: with D_e[q, o] = sum_mo B_e[mo, q] dout_e[mo, o] (formed in registers)
//   dh_e[c] = sum_(q, o) D_e[q, o] G_j[q, c, o],  dG_j[q, c, o] = sum_e h_e[c] D_e[q, o],  dGB_j[q, o] = sum_e D_e[q, o];
// every dG_j tile is written by exactly one wavefront (no atomics).  B carries no gradient.
#include "act.h"
#include "common.h"
#include "mfma.h"
#include "wave.h"

#include <float.h>

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_MID = 128;          // width of the radial trunk
constexpr int ST_NB = 34;            // basis floats per edge: 1 + 3 + 3 + 27
constexpr int ST_SLOTS = 17;         // self + 16 neighbour slots

// ------------------------------------------------------------------------------------------------------------------
// edge basis
// ------------------------------------------------------------------------------------------------------------------
// qtab: Q_0(0,0) [1] | Q_1(0,1) [3x3] | Q_1(1,0) [3x3] | Q_0(1,1) [9] | Q_1(1,1) [9x3] | Q_2(1,1) [9x5]   (100 floats)
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_edge_basis(const float* __restrict__ pos, const int* __restrict__ nbr, int64_t N, int K, float radius,
                  const float* __restrict__ qtab, float* __restrict__ dist, float* __restrict__ maskf,
                  float* __restrict__ meanw, float* __restrict__ basis) {
    const int64_t total = N * K, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t n = e / K;
        const float px = pos[3 * n], py = pos[3 * n + 1], pz = pos[3 * n + 2];
        int cnt = 0;
        float rx = 0.f, ry = 0.f, rz = 0.f, d = INFINITY;
        for (int s = 0; s < K; ++s) {
            const int j = nbr[n * K + s];
            float ds = INFINITY, ax = 0.f, ay = 0.f, az = 0.f;
            if (j >= 0 && j < N) {                       // (an index outside the cloud reads as a slot beyond the radius)
                ax = px - pos[3 * (int64_t)j]; ay = py - pos[3 * (int64_t)j + 1]; az = pz - pos[3 * (int64_t)j + 2];
                ds = sqrtf((ax * ax + ay * ay) + az * az);
            }
            cnt += ds <= radius ? 1 : 0;
            if (n * K + s == e) { d = ds; rx = ax; ry = ay; rz = az; }
        }
        const bool in = d <= radius;
        dist[e] = d;
        maskf[e] = in ? 1.f : 0.f;
        meanw[e] = in ? 1.f / (float)(cnt > 1 ? cnt : 1) : 0.f;
        // direction in the reference's axes (get_spherical_from_cartesian: x, y, z = components 2, 0, 1); a zero vector reads
        // as (0, 1, 0), what atan2(0, 0) = 0 gives there
        float u0 = 0.f, u1 = 1.f, u2 = 0.f;
        if (d > 0.f && d < INFINITY) { u0 = rx / d; u1 = ry / d; u2 = rz / d; }
        const float cy = u0, cz = u1, cx = u2;
        const float y0 = 0.28209479177387814f;
        const float n1 = 0.4886025119029199f, n2 = 0.6307831305050401f, s3 = 1.7320508075688772f;
        const float y1[3] = {-n1 * cy, -n1 * cz, -n1 * cx};
        const float y2[5] = {n2 * s3 * cx * cy, n2 * s3 * cy * cz, n2 * (1.5f * cz * cz - 0.5f), n2 * s3 * cx * cz,
                             n2 * 0.5f * s3 * (cx * cx - cy * cy)};
        float* __restrict__ b = basis + e * ST_NB;
        b[0] = y0 * qtab[0];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[1 + a] = (y1[0] * qtab[1 + 3 * a] + y1[1] * qtab[2 + 3 * a]) + y1[2] * qtab[3 + 3 * a];
            b[4 + a] = (y1[0] * qtab[10 + 3 * a] + y1[1] * qtab[11 + 3 * a]) + y1[2] * qtab[12 + 3 * a];
        }
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const float* q1 = qtab + 28 + 3 * a;
            const float* q2 = qtab + 55 + 5 * a;
            b[7 + 3 * a] = y0 * qtab[19 + a];
            b[8 + 3 * a] = (y1[0] * q1[0] + y1[1] * q1[1]) + y1[2] * q1[2];
            b[9 + 3 * a] = ((y2[0] * q2[0] + y2[1] * q2[1]) + (y2[2] * q2[2] + y2[3] * q2[3])) + y2[4] * q2[4];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// pair: forward
// ------------------------------------------------------------------------------------------------------------------
// Ends one trip of a loop that carries MFMA accumulators.  hipcc (ROCm 7.2, gfx950) may rotate such accumulators through
// v_accvgpr_read at the loop head, and across the back edge it was seen to leave fewer than the 12 wait states that the
// result of an 8-pass MFMA needs before anything but the next MFMA's C operand reads it: the last accumulator row of the
// forward product came out one trip stale.  Sixteen wait states behind the trip's last MFMA make the loop right whatever
// the register allocator does; they cost 16 of a trip's >= 500 cycles.
__device__ __forceinline__ void st_mfma_drain() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7");
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ int st_entry(const int* __restrict__ perm, int pos, int end, int64_t E) {
    if (pos >= end) return -1;
    const int e = perm[pos];
    return (e >= 0 && e < E) ? e : -1;
}

// out[e, mo, o] = sum_q coef[e, mo, q] (h[e] . G[row, q, :, o] + GB[row, q, o]);  one wavefront per sender row, grid.y splits
// the 64-column blocks.  O a multiple of 16.
template <int MO>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_pair_fwd(const float* __restrict__ h, const float* __restrict__ G, const float* __restrict__ GB,
                const float* __restrict__ coef, int cstride, const int* __restrict__ rowptr, const int* __restrict__ perm,
                int R, int64_t E, int Q, int O, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r_ = lane & 15, q4 = lane >> 4;
    const int cblocks = (O + 63) >> 6;
    for (int row = blockIdx.x * ST_WAVES + wave; row < R; row += gridDim.x * ST_WAVES) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        const float* __restrict__ Gr = G + (int64_t)row * Q * ST_MID * O;
        const float* __restrict__ GBr = GB + (int64_t)row * Q * O;
        for (int g0 = beg; g0 < end; g0 += 16) {
            const int e_r = st_entry(perm, g0 + r_, end, E);
            int e_g[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) e_g[g] = __shfl(e_r, 4 * q4 + g, 64);
            // A padding lane (no edge, or a column past O) reads edge 0 / column 0 instead: the rows and columns of an MFMA
            // product are independent, what such a lane computes is never stored, and the loop stays free of branches.
            const float* __restrict__ hr = h + (int64_t)(e_r >= 0 ? e_r : 0) * ST_MID + 4 * q4;
            const float* __restrict__ cr = coef + (int64_t)(e_r >= 0 ? e_r : 0) * cstride;
            for (int cb = blockIdx.y; cb < cblocks; cb += gridDim.y) {
                const int col = cb * 64 + 4 * r_;
                const bool act = col < O;
                const int col_ld = act ? col : 0;
                f32x4 acc[MO][4];
#pragma unroll
                for (int mo = 0; mo < MO; ++mo)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mo][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int q = 0; q < Q; ++q) {
                    float cf[MO];
#pragma unroll
                    for (int mo = 0; mo < MO; ++mo) cf[mo] = cr[mo * Q + q];
                    const float* __restrict__ Gq = Gr + (int64_t)q * ST_MID * O + (int64_t)(4 * q4) * O + col_ld;
                    for (int t = 0; t < ST_MID / 16; ++t) {
                        const float4 z4 = *reinterpret_cast<const float4*>(hr + 16 * t);
                        const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float4 b = *reinterpret_cast<const float4*>(Gq + (int64_t)(16 * t + i) * O);
#pragma unroll
                            for (int mo = 0; mo < MO; ++mo) {
                                const float a = zv[i] * cf[mo];
                                acc[mo][0] = mfma16(a, b.x, acc[mo][0]);
                                acc[mo][1] = mfma16(a, b.y, acc[mo][1]);
                                acc[mo][2] = mfma16(a, b.z, acc[mo][2]);
                                acc[mo][3] = mfma16(a, b.w, acc[mo][3]);
                            }
                        }
                        st_mfma_drain();
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int e = e_g[g];
                    if (e < 0 || !act) continue;
                    const float* __restrict__ ce = coef + (int64_t)e * cstride;
#pragma unroll
                    for (int mo = 0; mo < MO; ++mo) {
                        float4 o = make_float4(acc[mo][0][g], acc[mo][1][g], acc[mo][2][g], acc[mo][3][g]);
                        for (int q = 0; q < Q; ++q)
                            f4_fma(o, *reinterpret_cast<const float4*>(GBr + (int64_t)q * O + col), ce[mo * Q + q]);
                        *reinterpret_cast<float4*>(out + ((int64_t)e * MO + mo) * O + col) = o;
                    }
                }
            }
        }
    }
}

// out[n, x] (+)= sum_s meanw[n, s] src[n K + s, x]  (x over MO * O): se3_transformer/utils.py::masked_mean with
// meanw = mask / max(count, 1)
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_pool(const float* __restrict__ src, const float* __restrict__ meanw, int64_t N, int K, int W, float* __restrict__ out,
            int accumulate) {
    const int64_t total = N * W, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t n = i / W;
        const int x = (int)(i - n * W);
        float a = 0.f;
        for (int s = 0; s < K; ++s) a = fmaf(meanw[n * K + s], src[(n * K + s) * W + x], a);
        out[i] = accumulate ? out[i] + a : a;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// pair: backward
// ------------------------------------------------------------------------------------------------------------------
// the output gradient of edge e, component mo, columns o .. o + 3 (pooled: meanw[e] * dout[receiver])
__device__ __forceinline__ float4 st_dsrc4(const float* __restrict__ dout, const float* __restrict__ meanw, int K, int MO,
                                           int O, int e, int mo, int o) {
    if (meanw) {
        const float w = meanw[e];
        float4 v = *reinterpret_cast<const float4*>(dout + ((int64_t)(e / K) * MO + mo) * O + o);
        v.x *= w; v.y *= w; v.z *= w; v.w *= w;
        return v;
    }
    return *reinterpret_cast<const float4*>(dout + ((int64_t)e * MO + mo) * O + o);
}
__device__ __forceinline__ float st_dsrc(const float* __restrict__ dout, const float* __restrict__ meanw, int K, int MO,
                                         int O, int e, int mo, int o) {
    if (meanw) return meanw[e] * dout[((int64_t)(e / K) * MO + mo) * O + o];
    return dout[((int64_t)e * MO + mo) * O + o];
}

// dh[e, c] = sum_(q, o) D_e[q, o] G[row, q, c, o];  grid.y splits the eight 16-wide tiles of c
template <int MO>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_pair_bwd_h(const float* __restrict__ G, const float* __restrict__ coef, int cstride, const int* __restrict__ rowptr,
                  const int* __restrict__ perm, int R, int64_t E, int Q, int O, const float* __restrict__ dout,
                  const float* __restrict__ meanw, int K, float* __restrict__ dh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r_ = lane & 15, q4 = lane >> 4;
    for (int row = blockIdx.x * ST_WAVES + wave; row < R; row += gridDim.x * ST_WAVES) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        const float* __restrict__ Gr = G + (int64_t)row * Q * ST_MID * O;
        for (int g0 = beg; g0 < end; g0 += 16) {
            const int e_r = st_entry(perm, g0 + r_, end, E);
            int e_g[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) e_g[g] = __shfl(e_r, 4 * q4 + g, 64);
            const int e_ld = e_r >= 0 ? e_r : 0;         // (a padding lane works on edge 0; its row of the product is not stored)
            const float* __restrict__ cr = coef + (int64_t)e_ld * cstride;
            for (int kt = blockIdx.y; kt < ST_MID / 16; kt += gridDim.y) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int q = 0; q < Q; ++q) {
                    float cf[MO];
#pragma unroll
                    for (int mo = 0; mo < MO; ++mo) cf[mo] = cr[mo * Q + q];
                    const float* __restrict__ Gk = Gr + ((int64_t)q * ST_MID + kt * 16 + r_) * O + 4 * q4;
                    for (int t = 0; t < (O >> 4); ++t) {
                        float4 d4 = f4_zero();
#pragma unroll
                        for (int mo = 0; mo < MO; ++mo)
                            f4_fma(d4, st_dsrc4(dout, meanw, K, MO, O, e_ld, mo, 16 * t + 4 * q4), cf[mo]);
                        const float4 w4 = *reinterpret_cast<const float4*>(Gk + 16 * t);
                        acc = mfma16(d4.x, w4.x, acc);
                        acc = mfma16(d4.y, w4.y, acc);
                        acc = mfma16(d4.z, w4.z, acc);
                        acc = mfma16(d4.w, w4.w, acc);
                        st_mfma_drain();
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (e_g[g] >= 0) dh[(int64_t)e_g[g] * ST_MID + kt * 16 + r_] = acc[g];
            }
        }
    }
}

// dG[row, q, c, o] = sum_e h[e, c] D_e[q, o] and dGB[row, q, o] = sum_e D_e[q, o];  grid.y splits the Q * 8 * (O / 16) tiles
template <int MO>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_pair_bwd_g(const float* __restrict__ h, const float* __restrict__ coef, int cstride, const int* __restrict__ rowptr,
                  const int* __restrict__ perm, int R, int64_t E, int Q, int O, const float* __restrict__ dout,
                  const float* __restrict__ meanw, int K, float* __restrict__ dG, float* __restrict__ dGB) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r_ = lane & 15, q4 = lane >> 4;
    const int ltiles = O >> 4, ntiles = Q * (ST_MID / 16) * ltiles;
    for (int row = blockIdx.x * ST_WAVES + wave; row < R; row += gridDim.x * ST_WAVES) {
        const int beg = rowptr[row], end = rowptr[row + 1];
        float* __restrict__ dGr = dG + (int64_t)row * Q * ST_MID * O;
        for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
            const int q = tile / ((ST_MID / 16) * ltiles), rem = tile - q * (ST_MID / 16) * ltiles;
            const int kt = rem / ltiles, lt = rem - kt * ltiles;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int g0 = beg; g0 < end; g0 += 16) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    // the edges are the product's inner dimension here, so a padding lane reads edge 0 and contributes zero
                    const int e = st_entry(perm, g0 + 4 * q4 + c, end, E);
                    const int e_ld = e >= 0 ? e : 0;
                    const float a = h[(int64_t)e_ld * ST_MID + kt * 16 + r_];
                    float b = 0.f;
#pragma unroll
                    for (int mo = 0; mo < MO; ++mo)
                        b = fmaf(coef[(int64_t)e_ld * cstride + mo * Q + q], st_dsrc(dout, meanw, K, MO, O, e_ld, mo, lt * 16 + r_), b);
                    acc = mfma16(e >= 0 ? a : 0.f, e >= 0 ? b : 0.f, acc);
                }
                st_mfma_drain();
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) dGr[((int64_t)q * ST_MID + kt * 16 + 4 * q4 + g) * O + lt * 16 + r_] = acc[g];
        }
        if (blockIdx.y == 0) {
            for (int x = lane; x < Q * O; x += 64) {
                const int q = x / O, o = x - q * O;
                float s = 0.f;
                for (int p = beg; p < end; ++p) {
                    const int e = st_entry(perm, p, end, E);
                    if (e < 0) continue;
#pragma unroll
                    for (int mo = 0; mo < MO; ++mo)
                        s = fmaf(coef[(int64_t)e * cstride + mo * Q + q], st_dsrc(dout, meanw, K, MO, O, e, mo, o), s);
                }
                dGB[(int64_t)row * Q * O + x] = s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// attention (one degree per call): 2 heads x 32 channels, a wavefront per atom, lane = channel
// ------------------------------------------------------------------------------------------------------------------
// sum over the 32 lanes of a head, in each of them
__device__ __forceinline__ float head_sum(float v) {
    v = row16_sum(v);
    return v + __shfl_xor(v, 16);
}

template <int M>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_attn_fwd(const float* __restrict__ q, const float* __restrict__ kself, const float* __restrict__ kedge,
                const float* __restrict__ vself, const float* __restrict__ vedge, const float* __restrict__ maskf, int64_t N,
                int K, float scale, float* __restrict__ out, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = lane >> 5, hl = lane & 31;
    for (int64_t n = (int64_t)blockIdx.x * ST_WAVES + wave; n < N; n += (int64_t)gridDim.x * ST_WAVES) {
        float qv[M], o[M];
#pragma unroll
        for (int m = 0; m < M; ++m) { qv[m] = q[(n * M + m) * 64 + lane]; o[m] = 0.f; }
        float lg[ST_SLOTS];
        float mx = -FLT_MAX;
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) {
            lg[s] = -FLT_MAX;
            if (s <= K) {
                const float* __restrict__ kp = s == 0 ? kself + n * M * 64 : kedge + (n * K + s - 1) * M * 64;
                float p = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) p = fmaf(qv[m], kp[m * 64 + lane], p);
                p = head_sum(p) * scale;
                if (s > 0 && maskf[n * K + s - 1] == 0.f) p = -FLT_MAX;      // masked_fill(~mask, -finfo.max)
                lg[s] = p;
                mx = fmaxf(mx, p);
                if (hl == s) logits[(n * 2 + head) * (K + 1) + s] = p;
            }
        }
        float den = 0.f;
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) {
            lg[s] = s <= K ? expf(lg[s] - mx) : 0.f;
            den += lg[s];
        }
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) {
            if (s <= K) {
                const float* __restrict__ vp = s == 0 ? vself + n * M * 64 : vedge + (n * K + s - 1) * M * 64;
                const float p = lg[s] / den;
#pragma unroll
                for (int m = 0; m < M; ++m) o[m] = fmaf(p, vp[m * 64 + lane], o[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) out[(n * M + m) * 64 + lane] = o[m];
    }
}

template <int M>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_attn_bwd(const float* __restrict__ q, const float* __restrict__ kself, const float* __restrict__ kedge,
                const float* __restrict__ vself, const float* __restrict__ vedge, const float* __restrict__ logits,
                const float* __restrict__ dout, int64_t N, int K, float scale, float* __restrict__ dq,
                float* __restrict__ dkself, float* __restrict__ dkedge, float* __restrict__ dvself,
                float* __restrict__ dvedge) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = lane >> 5;
    for (int64_t n = (int64_t)blockIdx.x * ST_WAVES + wave; n < N; n += (int64_t)gridDim.x * ST_WAVES) {
        float qv[M], dv[M], dqv[M];
#pragma unroll
        for (int m = 0; m < M; ++m) { qv[m] = q[(n * M + m) * 64 + lane]; dv[m] = dout[(n * M + m) * 64 + lane]; dqv[m] = 0.f; }
        // the softmax again, from the saved (masked) logits
        float p[ST_SLOTS], dp[ST_SLOTS];
        const float* __restrict__ lr = logits + (n * 2 + head) * (K + 1);
        float mx = -FLT_MAX, den = 0.f, dot = 0.f;
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) { p[s] = s <= K ? lr[s] : -FLT_MAX; mx = fmaxf(mx, p[s]); }
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) { p[s] = s <= K ? expf(p[s] - mx) : 0.f; den += p[s]; }
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) {
            p[s] /= den;
            dp[s] = 0.f;
            if (s <= K) {
                const int64_t off = s == 0 ? n * M * 64 : (n * K + s - 1) * M * 64;
                const float* __restrict__ vp = (s == 0 ? vself : vedge) + off;
                float* __restrict__ dvp = (s == 0 ? dvself : dvedge) + off;
                float a = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    a = fmaf(dv[m], vp[m * 64 + lane], a);
                    dvp[m * 64 + lane] = p[s] * dv[m];
                }
                dp[s] = head_sum(a);
                dot = fmaf(p[s], dp[s], dot);
            }
        }
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) {
            if (s <= K) {
                const float dl = p[s] * (dp[s] - dot) * scale;
                const int64_t off = s == 0 ? n * M * 64 : (n * K + s - 1) * M * 64;
                const float* __restrict__ kp = (s == 0 ? kself : kedge) + off;
                float* __restrict__ dkp = (s == 0 ? dkself : dkedge) + off;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    dqv[m] = fmaf(dl, kp[m * 64 + lane], dqv[m]);
                    dkp[m * 64 + lane] = dl * qv[m];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) dq[(n * M + m) * 64 + lane] = dqv[m];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// NormSE3 on [R, M, C] rows: out = GELU(t s_c) x / t, t = max(|x|_m, eps).  A thread per (row, channel).
// ------------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_norm_fwd(const float* __restrict__ x, const float* __restrict__ scale, int64_t R, int C, float eps,
                float* __restrict__ out) {
    const int c = blockIdx.y * ST_THREADS + threadIdx.x;
    if (c >= C) return;
    const float s = scale[c];
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        float v[M], ss = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) { v[m] = x[(r * M + m) * C + c]; ss = fmaf(v[m], v[m], ss); }
        const float t = fmaxf(sqrtf(ss), eps);
        const float g = gelu_erf(t * s);
#pragma unroll
        for (int m = 0; m < M; ++m) out[(r * M + m) * C + c] = g * (v[m] / t);
    }
}

template <int M>
__global__ void __launch_bounds__(ST_THREADS)
k_se3t_norm_bwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ dy, int64_t R, int C,
                float eps, float* __restrict__ dx, float* __restrict__ slab) {
    const int c = blockIdx.y * ST_THREADS + threadIdx.x;
    if (c >= C) return;
    const float s = scale[c];
    float ds = 0.f;
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        float v[M], d[M], ss = 0.f, dot = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            v[m] = x[(r * M + m) * C + c];
            d[m] = dy[(r * M + m) * C + c];
            ss = fmaf(v[m], v[m], ss);
        }
        const float nrm = sqrtf(ss);
        const bool open = nrm >= eps;                // clamp(min = eps) passes the gradient where norm >= eps
        const float t = open ? nrm : eps;
#pragma unroll
        for (int m = 0; m < M; ++m) dot = fmaf(d[m], v[m] / t, dot);      // dy . phase
        const float a = t * s, g = gelu_erf(a), gp = gelu_erf_grad(a);
        ds = fmaf(dot * gp, t, ds);
        // d out_m / d x_k = delta g / t + phase_m phase_k (g' s - g / t)   (second term only while the clamp is open)
        const float k2 = open ? dot * (gp * s - g / t) : 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) dx[(r * M + m) * C + c] = d[m] * (g / t) + (v[m] / t) * k2;
    }
    slab[(int64_t)blockIdx.x * C + c] = ds;
}

inline int st_norm_blocks(int64_t R) { return eqh_grid_for(R, 8, 256); }

}  // namespace

extern "C" int se3t_edge_basis(const float* pos, const int32_t* nbr, int64_t N, int32_t K, float radius, const float* qtab,
                               float* dist, float* maskf, float* meanw, float* basis, void* stream_) {
    if (N < 0 || K < 1 || K > 16 || N > INT32_MAX) return EQH_ERR_ARG;
    if (N == 0) return EQH_OK;
    if (!pos || !nbr || !qtab || !dist || !maskf || !meanw || !basis) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_se3t_edge_basis, dim3(eqh_grid_for(N * K, ST_THREADS, 1024)), dim3(ST_THREADS), 0, stream, pos, nbr,
                       N, (int)K, radius, qtab, dist, maskf, meanw, basis);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

static int st_pair_check(int64_t N, int64_t E, int32_t MO, int32_t Q, int32_t O, int32_t K, int32_t cstride) {
    if (N < 0 || E < 0 || N > INT32_MAX || E > INT32_MAX) return EQH_ERR_ARG;
    if ((MO != 1 && MO != 3) || (Q != 1 && Q != 3 && Q != 9) || cstride < MO * Q || K < 1 || K > 16) return EQH_ERR_ARG;
    if (O < 16 || (O & 15) || O > 1024) return EQH_ERR_RANGE;
    return EQH_OK;
}

extern "C" size_t se3t_pair_fwd_workspace_bytes(int64_t E, int32_t MO, int32_t O, int32_t pooled) {
    if (!pooled || E <= 0 || MO <= 0 || O <= 0) return 0;
    return (size_t)E * (size_t)MO * (size_t)O * sizeof(float);
}

extern "C" int se3t_pair_fwd(const float* h, const float* G, const float* GB, const float* coef, int32_t cstride,
                             const int32_t* rowptr, const int32_t* perm, int64_t N, int64_t E, int32_t MO, int32_t Q,
                             int32_t O, const float* meanw, int32_t K, float* out, int32_t accumulate, void* workspace,
                             size_t workspace_bytes, void* stream_) {
    int rc = st_pair_check(N, E, MO, Q, O, K, cstride);
    if (rc) return rc;
    if (N == 0 || E == 0) return EQH_OK;
    if (!h || !G || !GB || !coef || !rowptr || !perm || !out) return EQH_ERR_ARG;
    if (!eqh_aligned16(h) || !eqh_aligned16(G) || !eqh_aligned16(GB) || !eqh_aligned16(out)) return EQH_ERR_ALIGN;
    const bool pooled = meanw != nullptr;
    if (!pooled && accumulate) return EQH_ERR_ARG;
    if (pooled && (E != N * K || !workspace || !eqh_aligned16(workspace) ||
                   workspace_bytes < se3t_pair_fwd_workspace_bytes(E, MO, O, 1)))
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* edge_out = pooled ? static_cast<float*>(workspace) : out;
    const dim3 grid(eqh_grid_for(N, ST_WAVES, 2048), (O + 63) / 64 < 4 ? (O + 63) / 64 : 4);
    if (MO == 1)
        hipLaunchKernelGGL((k_se3t_pair_fwd<1>), grid, dim3(ST_THREADS), 0, stream, h, G, GB, coef, (int)cstride, rowptr, perm,
                           (int)N, E, (int)Q, (int)O, edge_out);
    else
        hipLaunchKernelGGL((k_se3t_pair_fwd<3>), grid, dim3(ST_THREADS), 0, stream, h, G, GB, coef, (int)cstride, rowptr, perm,
                           (int)N, E, (int)Q, (int)O, edge_out);
    EQH_CHECK_LAUNCH();
    if (pooled) {
        hipLaunchKernelGGL(k_se3t_pool, dim3(eqh_grid_for(N * MO * O, ST_THREADS, 2048)), dim3(ST_THREADS), 0, stream,
                           (const float*)edge_out, meanw, N, (int)K, (int)(MO * O), out, (int)accumulate);
        EQH_CHECK_LAUNCH();
    }
    return EQH_OK;
}

extern "C" int se3t_pair_bwd(const float* h, const float* G, const float* coef, int32_t cstride, const int32_t* rowptr,
                             const int32_t* perm, int64_t N, int64_t E, int32_t MO, int32_t Q, int32_t O, const float* dout,
                             const float* meanw, int32_t K, float* dh, float* dG, float* dGB, void* stream_) {
    int rc = st_pair_check(N, E, MO, Q, O, K, cstride);
    if (rc) return rc;
    if (N == 0) return EQH_OK;
    if (!h || !G || !coef || !rowptr || !perm || !dout || !dh || !dG || !dGB) return EQH_ERR_ARG;
    if (!eqh_aligned16(G) || !eqh_aligned16(dout)) return EQH_ERR_ALIGN;
    if (meanw && E != N * K) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int gx = eqh_grid_for(N, ST_WAVES, 2048);
    const int ntiles = Q * (ST_MID / 16) * (O / 16);
    const dim3 gh(gx, 4), gg(gx, ntiles < 8 ? ntiles : 8);
    if (MO == 1) {
        hipLaunchKernelGGL((k_se3t_pair_bwd_h<1>), gh, dim3(ST_THREADS), 0, stream, G, coef, (int)cstride, rowptr, perm, (int)N, E,
                           (int)Q, (int)O, dout, meanw, (int)K, dh);
        EQH_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_se3t_pair_bwd_g<1>), gg, dim3(ST_THREADS), 0, stream, h, coef, (int)cstride, rowptr, perm, (int)N, E,
                           (int)Q, (int)O, dout, meanw, (int)K, dG, dGB);
    } else {
        hipLaunchKernelGGL((k_se3t_pair_bwd_h<3>), gh, dim3(ST_THREADS), 0, stream, G, coef, (int)cstride, rowptr, perm, (int)N, E,
                           (int)Q, (int)O, dout, meanw, (int)K, dh);
        EQH_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_se3t_pair_bwd_g<3>), gg, dim3(ST_THREADS), 0, stream, h, coef, (int)cstride, rowptr, perm, (int)N, E,
                           (int)Q, (int)O, dout, meanw, (int)K, dG, dGB);
    }
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int se3t_attn_fwd(const float* q, const float* kself, const float* kedge, const float* vself, const float* vedge,
                             const float* maskf, int64_t N, int32_t K, int32_t M, float scale, float* out, float* logits,
                             void* stream_) {
    if (N < 0 || N > INT32_MAX || K < 1 || K > 16 || (M != 1 && M != 3)) return EQH_ERR_ARG;
    if (N == 0) return EQH_OK;
    if (!q || !kself || !kedge || !vself || !vedge || !maskf || !out || !logits) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(eqh_grid_for(N, ST_WAVES, 2048));
    if (M == 1)
        hipLaunchKernelGGL((k_se3t_attn_fwd<1>), grid, dim3(ST_THREADS), 0, stream, q, kself, kedge, vself, vedge, maskf, N, (int)K,
                           scale, out, logits);
    else
        hipLaunchKernelGGL((k_se3t_attn_fwd<3>), grid, dim3(ST_THREADS), 0, stream, q, kself, kedge, vself, vedge, maskf, N, (int)K,
                           scale, out, logits);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int se3t_attn_bwd(const float* q, const float* kself, const float* kedge, const float* vself, const float* vedge,
                             const float* logits, const float* dout, int64_t N, int32_t K, int32_t M, float scale, float* dq,
                             float* dkself, float* dkedge, float* dvself, float* dvedge, void* stream_) {
    if (N < 0 || N > INT32_MAX || K < 1 || K > 16 || (M != 1 && M != 3)) return EQH_ERR_ARG;
    if (N == 0) return EQH_OK;
    if (!q || !kself || !kedge || !vself || !vedge || !logits || !dout || !dq || !dkself || !dkedge || !dvself || !dvedge)
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(eqh_grid_for(N, ST_WAVES, 2048));
    if (M == 1)
        hipLaunchKernelGGL((k_se3t_attn_bwd<1>), grid, dim3(ST_THREADS), 0, stream, q, kself, kedge, vself, vedge, logits, dout, N,
                           (int)K, scale, dq, dkself, dkedge, dvself, dvedge);
    else
        hipLaunchKernelGGL((k_se3t_attn_bwd<3>), grid, dim3(ST_THREADS), 0, stream, q, kself, kedge, vself, vedge, logits, dout, N,
                           (int)K, scale, dq, dkself, dkedge, dvself, dvedge);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int se3t_norm_fwd(const float* x, const float* scale, int64_t R, int32_t M, int32_t C, float eps, float* out,
                             void* stream_) {
    if (R < 0 || C < 1 || (M != 1 && M != 3)) return EQH_ERR_ARG;
    if (R == 0) return EQH_OK;
    if (!x || !scale || !out) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(eqh_grid_for(R, 1, 4096), (C + ST_THREADS - 1) / ST_THREADS);
    if (M == 1)
        hipLaunchKernelGGL((k_se3t_norm_fwd<1>), grid, dim3(ST_THREADS), 0, stream, x, scale, R, (int)C, eps, out);
    else
        hipLaunchKernelGGL((k_se3t_norm_fwd<3>), grid, dim3(ST_THREADS), 0, stream, x, scale, R, (int)C, eps, out);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" size_t se3t_norm_bwd_workspace_bytes(int64_t R, int32_t C) {
    if (R < 0 || C <= 0) return 0;
    return (size_t)st_norm_blocks(R) * (size_t)C * sizeof(float);
}

extern "C" int se3t_norm_bwd(const float* x, const float* scale, const float* dy, int64_t R, int32_t M, int32_t C, float eps,
                             float* dx, float* dscale, void* workspace, size_t workspace_bytes, void* stream_) {
    if (R < 0 || C < 1 || (M != 1 && M != 3) || !dscale) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (R == 0) return eqh_zero_async(dscale, C, stream);
    if (!x || !scale || !dy || !dx || !workspace) return EQH_ERR_ARG;
    if (workspace_bytes < se3t_norm_bwd_workspace_bytes(R, C)) return EQH_ERR_ARG;
    const int blocks = st_norm_blocks(R);
    float* slab = static_cast<float*>(workspace);
    const dim3 grid(blocks, (C + ST_THREADS - 1) / ST_THREADS);
    if (M == 1)
        hipLaunchKernelGGL((k_se3t_norm_bwd<1>), grid, dim3(ST_THREADS), 0, stream, x, scale, dy, R, (int)C, eps, dx, slab);
    else
        hipLaunchKernelGGL((k_se3t_norm_bwd<3>), grid, dim3(ST_THREADS), 0, stream, x, scale, dy, R, (int)C, eps, dx, slab);
    EQH_CHECK_LAUNCH();
    return eqh_reduce_slabs_async(slab, blocks, C, dscale, stream, 0);
}
