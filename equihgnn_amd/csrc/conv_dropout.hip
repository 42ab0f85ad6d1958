// Training dropout of the hypergraph convs' hidden layers (mlp.py:91-99: Linear -> ReLU -> LayerNorm -> dropout) on the
// fused row kernels: the dropout forms of incidence.hip's three hidden-layer kernels, forward and backward.
//   dense rows       out[r]  = keep[r] . LN(relu(h_scale h[r] + pre_add[r] + bias))                      element r C + c
//   gathered reduce  out[r]  = reduce_{q in row r} keep[src] . LN(relu(h[src] + bias)),  src = col[q]    element src C + c
//   per incidence    out[r]  = reduce_{q in row r} keep[p] . LN(relu(pa[ia[p]] + qb[ib[p]])), p = perm[q] element p C + c
// keep is 0 or 1 / (1 - p): the hash of (seed in device memory, element index) of drop_hash.h -- the flat index of the
// tensor F.dropout would have been applied to ([R, C], [N, C] before the gather, [nnz, C]), so the decisions are those of
// faf_dropout_add on that tensor.  No mask is stored: the backward recomputes h, mean, rstd and the keep decisions.
// Mapping, LayerNorm arithmetic and slab reduction are those of incidence.hip (rowln.h, row.h, wave.h); these kernels are
// a file of their own so that the code objects of the p = 0 kernels stay as they are.
//
// With a mask between beta and the sum, beta no longer factors out of the reduction (its term is beta * sum keep): the
// forward accumulates keep * fma(gamma, xhat, beta) per entry, and the per-incidence backward produces d beta itself
// (slab next to d gamma's) instead of leaving it to a column sum of the output gradient.
#include "common.h"
#include "drop_hash.h"
#include "rowln.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

// keep-scales of row `row` of a [., C] tensor (elements row * C + c), in the Row layout
template <int NV>
__device__ __forceinline__ void keep_row(const DropKey& key, int64_t row, int C, int lane, uint32_t threshold,
                                         float inv_keep, Row<NV>& k) {
    const uint64_t base = (uint64_t)row * (uint64_t)C;      // C % 4 == 0: every float4 group starts at a multiple of 4
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        k.v[i] = make_float4(1.f, 1.f, 1.f, 1.f);
        keep_scale4(key, base + (uint64_t)c, threshold, inv_keep, k.v[i]);
    }
}

template <int NV>
__device__ __forceinline__ void fetch_row(const float* __restrict__ base, int64_t o, int C, int lane, Row<NV>& u) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        u.v[i] = (c < C) ? *reinterpret_cast<const float4*>(base + o * C + c) : f4_zero();
    }
}

// acc += keep . (gamma * x + beta)
template <int NV>
__device__ __forceinline__ void add_kept(Row<NV>& acc, const Row<NV>& x, const Row<NV>& gam, const Row<NV>& bet,
                                         const Row<NV>& k) {
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

// the LayerNorm + ReLU backward of one row: d = the (masked) gradient of the LayerNorm's output, x = xhat; returns the
// gradient of the pre-activation in dx and adds d, d * xhat to the d beta / d gamma accumulators
template <int NV, bool PARAMS>
__device__ __forceinline__ void ln_relu_bwd(const Row<NV>& d_in, const Row<NV>& x, const Row<NV>& gam, unsigned pos,
                                            float rstd, float inv_c, Row<NV>& a_dg, Row<NV>& a_dbeta, Row<NV>& dx) {
    Row<NV> g;
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float4 d = d_in.v[i];
        if (PARAMS) {
            f4_add(a_dbeta.v[i], d);
            a_dg.v[i].x = fmaf(d.x, x.v[i].x, a_dg.v[i].x); a_dg.v[i].y = fmaf(d.y, x.v[i].y, a_dg.v[i].y);
            a_dg.v[i].z = fmaf(d.z, x.v[i].z, a_dg.v[i].z); a_dg.v[i].w = fmaf(d.w, x.v[i].w, a_dg.v[i].w);
        }
        d.x *= gam.v[i].x; d.y *= gam.v[i].y; d.z *= gam.v[i].z; d.w *= gam.v[i].w;
        g.v[i] = d;
        m1 += (d.x + d.y) + (d.z + d.w);
        m2 += (d.x * x.v[i].x + d.y * x.v[i].y) + (d.z * x.v[i].z + d.w * x.v[i].w);
    }
    wave_sum2(m1, m2);
    m1 *= inv_c;
    m2 *= inv_c;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const unsigned b = pos >> (4 * i);
        dx.v[i].x = (b & 1u) ? rstd * (g.v[i].x - m1 - x.v[i].x * m2) : 0.f;
        dx.v[i].y = (b & 2u) ? rstd * (g.v[i].y - m1 - x.v[i].y * m2) : 0.f;
        dx.v[i].z = (b & 4u) ? rstd * (g.v[i].z - m1 - x.v[i].z * m2) : 0.f;
        dx.v[i].w = (b & 8u) ? rstd * (g.v[i].w - m1 - x.v[i].w * m2) : 0.f;
    }
}

// the workgroup's NW wavefronts' copies of one accumulator row -> one slab row [C], summed in wavefront order
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
// (a) dense rows
// ------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_rowln_drop_fwd(const float* __restrict__ h, const float* __restrict__ bias, const float* __restrict__ gamma,
                 const float* __restrict__ beta, float* __restrict__ out, int n_rows, int C, float eps,
                 const float* __restrict__ pre_add, float h_scale, const int64_t* __restrict__ seed_ptr, uint32_t threshold,
                 float inv_keep) {
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> bias_row;
    fetch_row<NV>(bias, 0, C, lane, bias_row);
    for (int r = blockIdx.x * WAVES + wave; r < n_rows; r += gridDim.x * WAVES) {
        Row<NV> x, hr, k;
        unsigned pos;
        float rstd;
        fetch_row<NV>(h, r, C, lane, hr);
        if (pre_add) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (lane + 64 * i) * 4;
                const float4 a = (c < C) ? *reinterpret_cast<const float4*>(pre_add + (int64_t)r * C + c) : f4_zero();
                hr.v[i] = make_float4(fmaf(h_scale, hr.v[i].x, a.x), fmaf(h_scale, hr.v[i].y, a.y),
                                      fmaf(h_scale, hr.v[i].z, a.z), fmaf(h_scale, hr.v[i].w, a.w));
            }
        }
        norm_pair<NV, true>(hr, bias_row, C, lane, inv_c, eps, x, pos, &rstd);
        keep_row<NV>(key, r, C, lane, threshold, inv_keep, k);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < C) {
                const float4 g = *reinterpret_cast<const float4*>(gamma + c);
                const float4 b = *reinterpret_cast<const float4*>(beta + c);
                float4 o;
                o.x = k.v[i].x * fmaf(g.x, x.v[i].x, b.x); o.y = k.v[i].y * fmaf(g.y, x.v[i].y, b.y);
                o.z = k.v[i].z * fmaf(g.z, x.v[i].z, b.z); o.w = k.v[i].w * fmaf(g.w, x.v[i].w, b.w);
                *reinterpret_cast<float4*>(out + (int64_t)r * C + c) = o;
            }
        }
    }
}

// slab layout per workgroup: [dbias | dgamma | dbeta], each C floats (as k_rowln_bwd)
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_rowln_drop_bwd(const float* __restrict__ h, const float* __restrict__ bias, const float* __restrict__ gamma,
                 const float* __restrict__ dy, float* __restrict__ dh, float* __restrict__ slab, int n_rows, int C, float eps,
                 float* __restrict__ acc_out, int acc_first, const float* __restrict__ pre_add, float h_scale,
                 const int64_t* __restrict__ seed_ptr, uint32_t threshold, float inv_keep) {
    __shared__ float4 s_red[THREADS];
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> gam, bias_row, a_db, a_dg, a_dbeta;
    fetch_row<NV>(gamma, 0, C, lane, gam);
    fetch_row<NV>(bias, 0, C, lane, bias_row);
#pragma unroll
    for (int i = 0; i < NV; ++i) a_db.v[i] = a_dg.v[i] = a_dbeta.v[i] = f4_zero();
    // rows r, r + stride, ...: the operands of the next row are in flight while this one is normalised
    const int stride = gridDim.x * WAVES;
    int r = blockIdx.x * WAVES + wave;
    Row<NV> nh, nd;
    auto fetch = [&](int row) {
        const int rr = row < n_rows ? row : n_rows - 1;
        fetch_row<NV>(h, rr, C, lane, nh);
        if (pre_add) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (lane + 64 * i) * 4;
                const float4 a = (c < C) ? *reinterpret_cast<const float4*>(pre_add + (int64_t)rr * C + c) : f4_zero();
                nh.v[i] = make_float4(fmaf(h_scale, nh.v[i].x, a.x), fmaf(h_scale, nh.v[i].y, a.y),
                                      fmaf(h_scale, nh.v[i].z, a.z), fmaf(h_scale, nh.v[i].w, a.w));
            }
        }
        fetch_row<NV>(dy, rr, C, lane, nd);
    };
    if (r < n_rows) fetch(r);
    for (; r < n_rows; r += stride) {
        const Row<NV> ch = nh;
        Row<NV> cd = nd;
        fetch(r + stride);
        Row<NV> x, k, dx;
        unsigned pos;
        float rstd;
        norm_pair<NV, true>(ch, bias_row, C, lane, inv_c, eps, x, pos, &rstd);
        keep_row<NV>(key, r, C, lane, threshold, inv_keep, k);
#pragma unroll
        for (int i = 0; i < NV; ++i) { cd.v[i].x *= k.v[i].x; cd.v[i].y *= k.v[i].y; cd.v[i].z *= k.v[i].z; cd.v[i].w *= k.v[i].w; }
        ln_relu_bwd<NV, true>(cd, x, gam, pos, rstd, inv_c, a_dg, a_dbeta, dx);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (lane + 64 * i) * 4;
            f4_add(a_db.v[i], dx.v[i]);
            if (c < C) *reinterpret_cast<float4*>(dh + (int64_t)r * C + c) = dx.v[i];
            if (acc_out && c < C) {              // the same gradient summed over several applications of the layer
                float4 t = dx.v[i];
                if (!acc_first) f4_add(t, *reinterpret_cast<const float4*>(acc_out + (int64_t)r * C + c));
                *reinterpret_cast<float4*>(acc_out + (int64_t)r * C + c) = t;
            }
        }
    }
    float* __restrict__ sl = slab + (int64_t)blockIdx.x * 3 * C;
    slab_store<NV, WAVES>(s_red, sl, C, a_db);
    slab_store<NV, WAVES>(s_red, sl + C, C, a_dg);
    slab_store<NV, WAVES>(s_red, sl + 2 * C, C, a_dbeta);
}

// ------------------------------------------------------------------------------------------------
// (b) gathered reduction: the decision belongs to the SOURCE row
// ------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_gather_ln_drop_fwd(const float* __restrict__ h, const float* __restrict__ bias, const int* __restrict__ rowptr,
                     const int* __restrict__ col, const float* __restrict__ gamma, const float* __restrict__ beta,
                     float* __restrict__ out, int n_rows, int C, int mean, float eps, const int64_t* __restrict__ seed_ptr,
                     uint32_t threshold, float inv_keep) {
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> bias_row, gam, bet;
    fetch_row<NV>(bias, 0, C, lane, bias_row);
    fetch_row<NV>(gamma, 0, C, lane, gam);
    fetch_row<NV>(beta, 0, C, lane, bet);
    for (int r = blockIdx.x * WAVES + wave; r < n_rows; r += gridDim.x * WAVES) {
        const int beg = rowptr[r], end = rowptr[r + 1];
        Row<NV> acc;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc.v[i] = f4_zero();
        auto add_norm = [&](const Row<NV>& u, int o) {
            Row<NV> x, k;
            unsigned pos;
            float rstd;
            norm_pair<NV>(u, bias_row, C, lane, inv_c, eps, x, pos, &rstd);
            keep_row<NV>(key, o, C, lane, threshold, inv_keep, k);
            add_kept<NV>(acc, x, gam, bet, k);
        };
        for (int q0 = beg; q0 < end; q0 += 64) {
            const int cnt = (end - q0 < 64) ? (end - q0) : 64;
            const int my_o = (lane < cnt) ? col[q0 + lane] : 0;
            for (int j = 0; j < cnt; j += 4) {               // four entries' rows in flight together
                Row<NV> u0, u1, u2, u3;
                const int last = cnt - 1;
                const int o0 = __builtin_amdgcn_readlane(my_o, j);
                const int o1 = __builtin_amdgcn_readlane(my_o, (j + 1 < cnt) ? j + 1 : last);
                const int o2 = __builtin_amdgcn_readlane(my_o, (j + 2 < cnt) ? j + 2 : last);
                const int o3 = __builtin_amdgcn_readlane(my_o, (j + 3 < cnt) ? j + 3 : last);
                fetch_row<NV>(h, o0, C, lane, u0);
                fetch_row<NV>(h, o1, C, lane, u1);
                fetch_row<NV>(h, o2, C, lane, u2);
                fetch_row<NV>(h, o3, C, lane, u3);
                add_norm(u0, o0);
                if (j + 1 < cnt) add_norm(u1, o1);
                if (j + 2 < cnt) add_norm(u2, o2);
                if (j + 3 < cnt) add_norm(u3, o3);
            }
        }
        store_reduced<NV>(out, r, C, lane, acc, end - beg, mean);
    }
}

// Backward: every entry of source row v shares v's statistics AND v's keep decisions, so
//   dh[v] = LNbwd_v( keep[v] . sum_{q in row v of the TRANSPOSED CSR} w[q] * dout[col[q]] )
// as k_gather_ln_bwd with the mask applied to the gathered sum.  Slab: [dbias | dgamma | dbeta].
constexpr int GL_WAVES = 8;
template <int NV>
__global__ void __launch_bounds__(GL_WAVES * 64)
k_gather_ln_drop_bwd(const float* __restrict__ h, const float* __restrict__ bias, const float* __restrict__ gamma,
                     const float* __restrict__ dout, const int* __restrict__ t_rowptr, const int* __restrict__ t_col,
                     const float* __restrict__ t_w, float* __restrict__ dh, float* __restrict__ slab, int n_rows, int C,
                     float eps, int rows_per_wave, const int64_t* __restrict__ seed_ptr, uint32_t threshold, float inv_keep) {
    __shared__ float4 s_red[GL_WAVES * 64];
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> gam, a_db, a_dg, a_dbeta, bias_row;
    fetch_row<NV>(gamma, 0, C, lane, gam);
    fetch_row<NV>(bias, 0, C, lane, bias_row);
#pragma unroll
    for (int i = 0; i < NV; ++i) a_db.v[i] = a_dg.v[i] = a_dbeta.v[i] = f4_zero();
    const int64_t s_beg64 = (int64_t)(blockIdx.x * GL_WAVES + wave) * rows_per_wave;   // rows_per_wave <= 64
    const int s_beg = (s_beg64 < n_rows) ? (int)s_beg64 : n_rows;
    const int s_end = (s_beg + rows_per_wave < n_rows) ? s_beg + rows_per_wave : n_rows;
    if (s_beg < s_end) {
        const int p_beg = t_rowptr[s_beg];
        const int my_rend = (s_beg + lane < s_end) ? t_rowptr[s_beg + lane + 1] : 0;   // lane i: end of row s_beg + i
        const int p_end = t_rowptr[s_end];
        Row<NV> nh;
        fetch_row<NV>(h, s_beg, C, lane, nh);
        int q0 = p_beg;
        int cnt = (p_end - q0 < 64) ? (p_end - q0) : 64;
        int my_c = (lane < cnt) ? t_col[q0 + lane] : 0;
        float my_w = (t_w && lane < cnt) ? t_w[q0 + lane] : 1.0f;
        int q = p_beg;
        for (int row = s_beg; row < s_end; ++row) {
            const int rend = __builtin_amdgcn_readlane(my_rend, row - s_beg);
            const Row<NV> ch = nh;
            fetch_row<NV>(h, row + 1 < s_end ? row + 1 : row, C, lane, nh);
            Row<NV> dsum;
#pragma unroll
            for (int i = 0; i < NV; ++i) dsum.v[i] = f4_zero();
            while (q < rend) {
                if (q - q0 >= 64) {     // next chunk of the range's entries
                    q0 += 64;
                    cnt = (p_end - q0 < 64) ? (p_end - q0) : 64;
                    my_c = (lane < cnt) ? t_col[q0 + lane] : 0;
                    my_w = (t_w && lane < cnt) ? t_w[q0 + lane] : 1.0f;
                }
                // up to four of the row's entries in flight together (those past the row / chunk end re-read the last
                // valid one with weight 0)
                const int j = q - q0;
                int lim = rend - q0;
                if (lim > cnt) lim = cnt;
                const int n = (lim - j < 4) ? lim - j : 4;
                Row<NV> d0, d1, d2, d3;
                const int j1 = (n > 1) ? j + 1 : j, j2 = (n > 2) ? j + 2 : j, j3 = (n > 3) ? j + 3 : j;
                fetch_row<NV>(dout, __builtin_amdgcn_readlane(my_c, j), C, lane, d0);
                fetch_row<NV>(dout, __builtin_amdgcn_readlane(my_c, j1), C, lane, d1);
                fetch_row<NV>(dout, __builtin_amdgcn_readlane(my_c, j2), C, lane, d2);
                fetch_row<NV>(dout, __builtin_amdgcn_readlane(my_c, j3), C, lane, d3);
                const float w0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j));
                const float w1 = (n > 1) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j1)) : 0.f;
                const float w2 = (n > 2) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j2)) : 0.f;
                const float w3 = (n > 3) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j3)) : 0.f;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    f4_fma(dsum.v[i], d0.v[i], w0);
                    f4_fma(dsum.v[i], d1.v[i], w1);
                    f4_fma(dsum.v[i], d2.v[i], w2);
                    f4_fma(dsum.v[i], d3.v[i], w3);
                }
                q += n;
            }
            Row<NV> x, k, dx;
            unsigned pos;
            float rstd;
            norm_pair<NV>(ch, bias_row, C, lane, inv_c, eps, x, pos, &rstd);
            keep_row<NV>(key, row, C, lane, threshold, inv_keep, k);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                dsum.v[i].x *= k.v[i].x; dsum.v[i].y *= k.v[i].y; dsum.v[i].z *= k.v[i].z; dsum.v[i].w *= k.v[i].w;
            }
            ln_relu_bwd<NV, true>(dsum, x, gam, pos, rstd, inv_c, a_dg, a_dbeta, dx);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (lane + 64 * i) * 4;
                f4_add(a_db.v[i], dx.v[i]);
                if (c < C) *reinterpret_cast<float4*>(dh + (int64_t)row * C + c) = dx.v[i];
            }
        }
    }
    float* __restrict__ sl = slab + (int64_t)blockIdx.x * 3 * C;
    slab_store<NV, GL_WAVES>(s_red, sl, C, a_db);
    slab_store<NV, GL_WAVES>(s_red, sl + C, C, a_dg);
    slab_store<NV, GL_WAVES>(s_red, sl + 2 * C, C, a_dbeta);
}

// ------------------------------------------------------------------------------------------------
// (c) per incidence: the decision belongs to the incidence, i.e. to its position p in ia / ib -- whatever CSR order a
// kernel walks, it looks the position up in that CSR's perm
// ------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_inc_drop_fwd(const float* __restrict__ pa, const float* __restrict__ qb, const int* __restrict__ ia,
               const int* __restrict__ ib, const int* __restrict__ rowptr, const int* __restrict__ perm,
               const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out, int n_rows, int C,
               int mean, float eps, const int64_t* __restrict__ seed_ptr, uint32_t threshold, float inv_keep) {
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> gam, bet;
    fetch_row<NV>(gamma, 0, C, lane, gam);
    fetch_row<NV>(beta, 0, C, lane, bet);
    for (int r = blockIdx.x * WAVES + wave; r < n_rows; r += gridDim.x * WAVES) {
        const int beg = rowptr[r], end = rowptr[r + 1];
        Row<NV> acc;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc.v[i] = f4_zero();
        for (int q0 = beg; q0 < end; q0 += 64) {
            const int cnt = (end - q0 < 64) ? (end - q0) : 64;
            int my_a = 0, my_b = 0, my_p = 0;
            if (lane < cnt) {
                my_p = perm[q0 + lane];
                my_a = ia[my_p];
                my_b = ib[my_p];
            }
            for (int j = 0; j < cnt; ++j) {
                Row<NV> u, w, x, k;
                unsigned pos;
                float rstd;
                fetch_row<NV>(pa, __builtin_amdgcn_readlane(my_a, j), C, lane, u);
                fetch_row<NV>(qb, __builtin_amdgcn_readlane(my_b, j), C, lane, w);
                norm_pair<NV>(u, w, C, lane, inv_c, eps, x, pos, &rstd);
                keep_row<NV>(key, __builtin_amdgcn_readlane(my_p, j), C, lane, threshold, inv_keep, k);
                add_kept<NV>(acc, x, gam, bet, k);
            }
        }
        store_reduced<NV>(out, r, C, lane, acc, end - beg, mean);
    }
}

// the output row is one operand's own index: (rowptr, col) describes the rows, perm gives the incidences' positions
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_inc_drop_fwd_col(const float* __restrict__ pa, const float* __restrict__ qb, const int* __restrict__ rowptr,
                   const int* __restrict__ col, const int* __restrict__ perm, int row_is_a, const float* __restrict__ gamma,
                   const float* __restrict__ beta, float* __restrict__ out, int n_rows, int C, int mean, float eps,
                   const int64_t* __restrict__ seed_ptr, uint32_t threshold, float inv_keep) {
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    const float* __restrict__ own = row_is_a ? pa : qb;      // the operand indexed by the output row
    const float* __restrict__ oth = row_is_a ? qb : pa;      // the operand indexed by the CSR's col
    Row<NV> gam, bet;
    fetch_row<NV>(gamma, 0, C, lane, gam);
    fetch_row<NV>(beta, 0, C, lane, bet);
    for (int r = blockIdx.x * WAVES + wave; r < n_rows; r += gridDim.x * WAVES) {
        const int beg = rowptr[r], end = rowptr[r + 1];
        Row<NV> acc, mine;
        fetch_row<NV>(own, r, C, lane, mine);                // once per row (it does not wait for the index chain)
#pragma unroll
        for (int i = 0; i < NV; ++i) acc.v[i] = f4_zero();
        auto add_norm = [&](const Row<NV>& w, int p) {
            Row<NV> x, k;
            unsigned pos;
            float rstd;
            norm_pair<NV>(mine, w, C, lane, inv_c, eps, x, pos, &rstd);
            keep_row<NV>(key, p, C, lane, threshold, inv_keep, k);
            add_kept<NV>(acc, x, gam, bet, k);
        };
        for (int q0 = beg; q0 < end; q0 += 64) {
            const int cnt = (end - q0 < 64) ? (end - q0) : 64;
            const int my_o = (lane < cnt) ? col[q0 + lane] : 0;
            const int my_p = (lane < cnt) ? perm[q0 + lane] : 0;
            for (int j = 0; j < cnt; j += 4) {               // four entries' rows in flight together
                Row<NV> w0, w1, w2, w3;
                const int last = cnt - 1;
                const int j1 = (j + 1 < cnt) ? j + 1 : last, j2 = (j + 2 < cnt) ? j + 2 : last, j3 = (j + 3 < cnt) ? j + 3 : last;
                fetch_row<NV>(oth, __builtin_amdgcn_readlane(my_o, j), C, lane, w0);
                fetch_row<NV>(oth, __builtin_amdgcn_readlane(my_o, j1), C, lane, w1);
                fetch_row<NV>(oth, __builtin_amdgcn_readlane(my_o, j2), C, lane, w2);
                fetch_row<NV>(oth, __builtin_amdgcn_readlane(my_o, j3), C, lane, w3);
                add_norm(w0, __builtin_amdgcn_readlane(my_p, j));
                if (j + 1 < cnt) add_norm(w1, __builtin_amdgcn_readlane(my_p, j1));
                if (j + 2 < cnt) add_norm(w2, __builtin_amdgcn_readlane(my_p, j2));
                if (j + 3 < cnt) add_norm(w3, __builtin_amdgcn_readlane(my_p, j3));
            }
        }
        store_reduced<NV>(out, r, C, lane, acc, end - beg, mean);
    }
}

// One side of the backward (see inc_bwd_body of incidence.hip: a wavefront owns a range of consecutive rows of the CSR
// keyed by the operand whose gradient it produces).  The upstream gradient of incidence p is w . keep[p] . ds[okey[p]];
// the side keyed by ia also accumulates d gamma and d beta: slab [dgamma | dbeta] per workgroup.
template <int NV, bool PARAMS, bool SIDE_A>
__device__ __forceinline__ void
inc_drop_bwd_body(const int block, float4* s_g, const DropKey& key, uint32_t threshold, float inv_keep,
                  const float* __restrict__ pa, const float* __restrict__ qb, const int* __restrict__ ia,
                  const int* __restrict__ ib, const int* __restrict__ side_rowptr, const int* __restrict__ side_perm,
                  const int* __restrict__ okey, const int* __restrict__ orowptr, const float* __restrict__ ds,
                  const float* __restrict__ gamma, float* __restrict__ dside, float* __restrict__ slab, int n_side_rows,
                  int C, int mean, float eps, int rows_per_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_c = 1.0f / (float)C;
    Row<NV> gam, dgam, dbet;
    fetch_row<NV>(gamma, 0, C, lane, gam);
#pragma unroll
    for (int i = 0; i < NV; ++i) dgam.v[i] = dbet.v[i] = f4_zero();
    const int64_t s_beg64 = (int64_t)(block * WAVES + wave) * rows_per_wave;
    const int s_beg = (s_beg64 < n_side_rows) ? (int)s_beg64 : n_side_rows;
    const int s_end = (s_beg + rows_per_wave < n_side_rows) ? s_beg + rows_per_wave : n_side_rows;
    if (s_beg < s_end) {
        const int p_beg = side_rowptr[s_beg], p_end = side_rowptr[s_end];
        int cur_row = s_beg;  // row whose sum `acc` is building
        Row<NV> acc;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc.v[i] = f4_zero();
        auto flush_until = [&](int row) {  // rows [cur_row, row) are complete (empty ones store zeros)
            for (; cur_row < row; ++cur_row) {
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int c = (lane + 64 * i) * 4;
                    if (c < C) *reinterpret_cast<float4*>(dside + (int64_t)cur_row * C + c) = acc.v[i];
                    acc.v[i] = f4_zero();
                }
            }
        };
        for (int q0 = p_beg; q0 < p_end; q0 += 64) {
            const int cnt = (p_end - q0 < 64) ? (p_end - q0) : 64;
            int my_a = 0, my_b = 0, my_r = 0, my_p = 0;
            float my_w = 1.0f;
            if (lane < cnt) {
                my_p = side_perm[q0 + lane];
                my_a = ia[my_p];
                my_b = ib[my_p];
                my_r = okey[my_p];
                const int deg = orowptr[my_r + 1] - orowptr[my_r];
                my_w = (mean && deg > 1) ? 1.0f / (float)deg : 1.0f;
            }
            Row<NV> nu, nw, nd;  // operands of the next incidence
            fetch_row<NV>(pa, __builtin_amdgcn_readlane(my_a, 0), C, lane, nu);
            fetch_row<NV>(qb, __builtin_amdgcn_readlane(my_b, 0), C, lane, nw);
            fetch_row<NV>(ds, __builtin_amdgcn_readlane(my_r, 0), C, lane, nd);
            for (int j = 0; j < cnt; ++j) {
                const Row<NV> cu = nu, cw = nw;
                Row<NV> d = nd;
                const int a_j = __builtin_amdgcn_readlane(my_a, j), b_j = __builtin_amdgcn_readlane(my_b, j);
                const int p_j = __builtin_amdgcn_readlane(my_p, j);
                const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j));
                {
                    const int jn = (j + 1 < cnt) ? j + 1 : j;  // the last one re-reads itself
                    fetch_row<NV>(pa, __builtin_amdgcn_readlane(my_a, jn), C, lane, nu);
                    fetch_row<NV>(qb, __builtin_amdgcn_readlane(my_b, jn), C, lane, nw);
                    fetch_row<NV>(ds, __builtin_amdgcn_readlane(my_r, jn), C, lane, nd);
                }
                flush_until(SIDE_A ? a_j : b_j);
                Row<NV> x, k, dx;
                unsigned pos;
                float rstd;
                norm_pair<NV>(cu, cw, C, lane, inv_c, eps, x, pos, &rstd);
                keep_row<NV>(key, p_j, C, lane, threshold, inv_keep, k);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    d.v[i].x *= w * k.v[i].x; d.v[i].y *= w * k.v[i].y; d.v[i].z *= w * k.v[i].z; d.v[i].w *= w * k.v[i].w;
                }
                ln_relu_bwd<NV, PARAMS>(d, x, gam, pos, rstd, inv_c, dgam, dbet, dx);
#pragma unroll
                for (int i = 0; i < NV; ++i) f4_add(acc.v[i], dx.v[i]);
            }
        }
        flush_until(s_end);
    }
    if (PARAMS) {
        float* __restrict__ sl = slab + (int64_t)block * 2 * C;
        slab_store<NV, WAVES>(s_g, sl, C, dgam);
        slab_store<NV, WAVES>(s_g, sl + C, C, dbet);
    }
}

// both sides in ONE launch: workgroups [0, blocks_a) take the side keyed by ia, the rest the side keyed by ib
template <int NV>
__global__ void __launch_bounds__(THREADS)
k_inc_drop_bwd_both(const float* __restrict__ pa, const float* __restrict__ qb, const int* __restrict__ ia,
                    const int* __restrict__ ib, const int* __restrict__ a_rowptr, const int* __restrict__ a_perm,
                    const int* __restrict__ b_rowptr, const int* __restrict__ b_perm, const int* __restrict__ okey,
                    const int* __restrict__ orowptr, const float* __restrict__ ds, const float* __restrict__ gamma,
                    float* __restrict__ dpa, float* __restrict__ dqb, float* __restrict__ slab, int n_a_rows, int n_b_rows,
                    int blocks_a, int C, int mean, float eps, int rpw_a, int rpw_b, const int64_t* __restrict__ seed_ptr,
                    uint32_t threshold, float inv_keep) {
    __shared__ float4 s_g[THREADS];
    const DropKey key = drop_key(threshold ? (uint64_t)*seed_ptr : 0);
    if ((int)blockIdx.x < blocks_a)
        inc_drop_bwd_body<NV, true, true>((int)blockIdx.x, s_g, key, threshold, inv_keep, pa, qb, ia, ib, a_rowptr, a_perm,
                                          okey, orowptr, ds, gamma, dpa, slab, n_a_rows, C, mean, eps, rpw_a);
    else
        inc_drop_bwd_body<NV, false, false>((int)blockIdx.x - blocks_a, s_g, key, threshold, inv_keep, pa, qb, ia, ib,
                                            b_rowptr, b_perm, okey, orowptr, ds, gamma, dqb, nullptr, n_b_rows, C, mean,
                                            eps, rpw_b);
}

// grids: those of the p = 0 kernels (incidence.hip)
inline int rowln_blocks(int64_t rows) { return eqh_grid_for(rows, WAVES * 4, rows > 65536 ? 2048 : 256); }
inline int bwd_rpw(int64_t rows) {
    const int64_t r = (rows + 2047) / 2048;
    return (int)(r < 1 ? 1 : r);
}
inline int bwd_blocks(int64_t rows) {
    const int64_t per_block = (int64_t)bwd_rpw(rows) * WAVES;
    const int64_t b = (rows + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b);
}
inline int gl_rpw(int64_t rows) { const int64_t r = (rows + 8191) / 8192; return r > 64 ? 64 : (r < 1 ? 1 : (int)r); }
inline int gl_blocks(int64_t rows) {
    const int64_t per_block = (int64_t)gl_rpw(rows) * GL_WAVES;
    const int64_t b = (rows + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b);
}

int check(int64_t rows, int C, float p) {
    if (rows < 0 || C <= 0 || !(p >= 0.f) || !(p < 1.f)) return EQH_ERR_ARG;
    if ((C & 3) || C > 1024) return EQH_ERR_ALIGN;
    if (rows >= ((int64_t)1 << 31) - 1) return EQH_ERR_RANGE;
    return EQH_OK;
}

int zero3(float* a, float* b, float* c, int C, hipStream_t stream) {
    if (eqh_zero_async(a, C, stream) || eqh_zero_async(b, C, stream)) return EQH_ERR_LAUNCH;
    return c ? eqh_zero_async(c, C, stream) : EQH_OK;
}

}  // namespace

extern "C" int hg_bias_relu_ln_drop_fwd(const float* h, float h_scale, const float* pre_add, const float* bias,
                                        const float* gamma, const float* beta, int64_t n_rows, int32_t C, float eps, float p,
                                        const int64_t* seed, float* out, void* stream_) {
    int rc = check(n_rows, C, p);
    if (rc) return rc;
    if (n_rows == 0) return EQH_OK;
    if (!h || !bias || !gamma || !beta || !out || (!pre_add && h_scale != 1.0f) || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(h) || !eqh_aligned16(bias) || !eqh_aligned16(gamma) || !eqh_aligned16(beta) || !eqh_aligned16(out) ||
        !eqh_aligned16(pre_add))
        return EQH_ERR_ALIGN;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_rowln_drop_fwd<NV>), dim3(eqh_grid_for(n_rows, WAVES, 4096)), dim3(THREADS), 0, stream, h, bias,
                           gamma, beta, out, (int)n_rows, (int)C, eps, pre_add, h_scale, seed, drop_threshold(p),
                           drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return EQH_OK;
    });
}

extern "C" size_t hg_bias_relu_ln_drop_bwd_workspace_bytes(int64_t n_rows, int32_t C) {
    if (n_rows < 0 || C <= 0) return 0;
    return (size_t)rowln_blocks(n_rows) * 3 * (size_t)C * sizeof(float);
}

extern "C" int hg_bias_relu_ln_drop_bwd(const float* h, float h_scale, const float* pre_add, const float* bias,
                                        const float* gamma, const float* dy, int64_t n_rows, int32_t C, float eps, float p,
                                        const int64_t* seed, float* dh, float* dbias, float* dgamma, float* dbeta,
                                        int32_t accumulate, void* workspace, size_t workspace_bytes, float* acc_out,
                                        int32_t acc_first, void* stream_) {
    int rc = check(n_rows, C, p);
    if (rc) return rc;
    if (!dbias || !dgamma || !dbeta || (!pre_add && h_scale != 1.0f)) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_rows == 0) return accumulate ? EQH_OK : zero3(dbias, dgamma, dbeta, C, stream);
    if (!h || !bias || !gamma || !dy || !dh || !workspace || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(h) || !eqh_aligned16(dy) || !eqh_aligned16(dh) || !eqh_aligned16(workspace) || !eqh_aligned16(bias) ||
        !eqh_aligned16(gamma) || !eqh_aligned16(pre_add) || !eqh_aligned16(acc_out))
        return EQH_ERR_ALIGN;
    if (workspace_bytes < hg_bias_relu_ln_drop_bwd_workspace_bytes(n_rows, C)) return EQH_ERR_ARG;
    const int blocks = rowln_blocks(n_rows);
    float* slab = static_cast<float*>(workspace);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_rowln_drop_bwd<NV>), dim3(blocks), dim3(THREADS), 0, stream, h, bias, gamma, dy, dh, slab,
                           (int)n_rows, (int)C, eps, acc_out, (int)acc_first, pre_add, h_scale, seed, drop_threshold(p),
                           drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return eqh_reduce_slabs3_async(slab, blocks, 3 * (int64_t)C, dbias, dgamma, dbeta, C, C, accumulate, stream);
    });
}

extern "C" int hg_gather_ln_reduce_drop_fwd(const float* h, const float* bias, const float* gamma, const float* beta,
                                            const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t C,
                                            int32_t mean, float eps, float p, const int64_t* seed, float* out, void* stream_) {
    int rc = check(n_rows, C, p);
    if (rc) return rc;
    if (n_rows == 0) return EQH_OK;
    if (!h || !bias || !gamma || !beta || !rowptr || !col || !out || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(h) || !eqh_aligned16(bias) || !eqh_aligned16(gamma) || !eqh_aligned16(beta) || !eqh_aligned16(out))
        return EQH_ERR_ALIGN;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_gather_ln_drop_fwd<NV>), dim3(eqh_grid_for(n_rows, WAVES, 4096)), dim3(THREADS), 0, stream, h,
                           bias, rowptr, col, gamma, beta, out, (int)n_rows, (int)C, (int)mean, eps, seed, drop_threshold(p),
                           drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return EQH_OK;
    });
}

extern "C" size_t hg_gather_ln_reduce_drop_bwd_workspace_bytes(int64_t n_src_rows, int32_t C) {
    if (n_src_rows < 0 || C <= 0) return 0;
    return (size_t)gl_blocks(n_src_rows) * 3 * (size_t)C * sizeof(float);
}

extern "C" int hg_gather_ln_reduce_drop_bwd(const float* h, const float* bias, const float* gamma, const float* dout,
                                            const int32_t* t_rowptr, const int32_t* t_col, const float* t_w,
                                            int64_t n_src_rows, int32_t C, float eps, float p, const int64_t* seed, float* dh,
                                            float* dbias, float* dgamma, float* dbeta, int32_t accumulate, void* workspace,
                                            size_t workspace_bytes, void* stream_) {
    int rc = check(n_src_rows, C, p);
    if (rc) return rc;
    if (!dbias || !dgamma || !dbeta) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_src_rows == 0) return accumulate ? EQH_OK : zero3(dbias, dgamma, dbeta, C, stream);
    if (!h || !bias || !gamma || !dout || !t_rowptr || !t_col || !dh || !workspace || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(h) || !eqh_aligned16(dout) || !eqh_aligned16(dh) || !eqh_aligned16(workspace) || !eqh_aligned16(bias) ||
        !eqh_aligned16(gamma))
        return EQH_ERR_ALIGN;
    if (workspace_bytes < hg_gather_ln_reduce_drop_bwd_workspace_bytes(n_src_rows, C)) return EQH_ERR_ARG;
    const int blocks = gl_blocks(n_src_rows);
    float* slab = static_cast<float*>(workspace);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_gather_ln_drop_bwd<NV>), dim3(blocks), dim3(GL_WAVES * 64), 0, stream, h, bias, gamma, dout,
                           t_rowptr, t_col, t_w, dh, slab, (int)n_src_rows, (int)C, eps, gl_rpw(n_src_rows), seed,
                           drop_threshold(p), drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return eqh_reduce_slabs3_async(slab, blocks, 3 * (int64_t)C, dbias, dgamma, dbeta, C, C, accumulate, stream);
    });
}

extern "C" int hg_incidence_ln_reduce_drop_fwd(const float* pa, const float* qb, const int32_t* ia, const int32_t* ib,
                                               const int32_t* rowptr, const int32_t* perm, const float* gamma,
                                               const float* beta, int64_t n_rows, int32_t C, int32_t mean, float eps, float p,
                                               const int64_t* seed, float* out, void* stream_) {
    int rc = check(n_rows, C, p);
    if (rc) return rc;
    if (n_rows == 0) return EQH_OK;
    if (!pa || !qb || !ia || !ib || !rowptr || !perm || !gamma || !beta || !out || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(pa) || !eqh_aligned16(qb) || !eqh_aligned16(gamma) || !eqh_aligned16(beta) || !eqh_aligned16(out))
        return EQH_ERR_ALIGN;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_inc_drop_fwd<NV>), dim3(eqh_grid_for(n_rows, WAVES, 4096)), dim3(THREADS), 0, stream, pa, qb, ia,
                           ib, rowptr, perm, gamma, beta, out, (int)n_rows, (int)C, (int)mean, eps, seed, drop_threshold(p),
                           drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return EQH_OK;
    });
}

extern "C" int hg_incidence_ln_reduce_drop_fwd_col(const float* pa, const float* qb, const int32_t* rowptr,
                                                   const int32_t* col, const int32_t* perm, int32_t row_is_a,
                                                   const float* gamma, const float* beta, int64_t n_rows, int32_t C,
                                                   int32_t mean, float eps, float p, const int64_t* seed, float* out,
                                                   void* stream_) {
    int rc = check(n_rows, C, p);
    if (rc) return rc;
    if (n_rows == 0) return EQH_OK;
    if (!pa || !qb || !rowptr || !col || !perm || !gamma || !beta || !out || (p > 0.f && !seed)) return EQH_ERR_ARG;
    if (!eqh_aligned16(pa) || !eqh_aligned16(qb) || !eqh_aligned16(gamma) || !eqh_aligned16(beta) || !eqh_aligned16(out))
        return EQH_ERR_ALIGN;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_inc_drop_fwd_col<NV>), dim3(eqh_grid_for(n_rows, WAVES, 4096)), dim3(THREADS), 0, stream, pa, qb,
                           rowptr, col, perm, (int)row_is_a, gamma, beta, out, (int)n_rows, (int)C, (int)mean, eps, seed,
                           drop_threshold(p), drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return EQH_OK;
    });
}

extern "C" size_t hg_incidence_ln_reduce_drop_bwd_workspace_bytes(int64_t n_a_rows, int32_t C) {
    if (n_a_rows < 0 || C <= 0) return 0;
    return (size_t)bwd_blocks(n_a_rows) * 2 * (size_t)C * sizeof(float);
}

extern "C" int hg_incidence_ln_reduce_drop_bwd(const float* pa, const float* qb, const int32_t* ia, const int32_t* ib,
                                               const int32_t* a_rowptr, const int32_t* a_perm, int64_t n_a_rows,
                                               const int32_t* b_rowptr, const int32_t* b_perm, int64_t n_b_rows,
                                               const int32_t* okey, const int32_t* orowptr, const float* ds,
                                               const float* gamma, int32_t C, int32_t mean, float eps, float p,
                                               const int64_t* seed, float* dpa, float* dqb, float* dgamma, float* dbeta,
                                               int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = check(n_a_rows, C, p);
    if (rc) return rc;
    rc = check(n_b_rows, C, p);
    if (rc) return rc;
    if (!dgamma || !dbeta || !gamma) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_a_rows == 0 && n_b_rows == 0) return accumulate ? EQH_OK : zero3(dgamma, dbeta, nullptr, C, stream);
    if (!pa || !qb || !ia || !ib || !a_rowptr || !a_perm || !b_rowptr || !b_perm || !okey || !orowptr || !ds || !dpa || !dqb ||
        !workspace || (p > 0.f && !seed))
        return EQH_ERR_ARG;
    if (!eqh_aligned16(pa) || !eqh_aligned16(qb) || !eqh_aligned16(gamma) || !eqh_aligned16(ds) || !eqh_aligned16(dpa) ||
        !eqh_aligned16(dqb) || !eqh_aligned16(workspace))
        return EQH_ERR_ALIGN;
    if (workspace_bytes < hg_incidence_ln_reduce_drop_bwd_workspace_bytes(n_a_rows, C)) return EQH_ERR_ARG;
    float* slab = static_cast<float*>(workspace);
    const int blocks_a = bwd_blocks(n_a_rows);
    return dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_inc_drop_bwd_both<NV>), dim3(blocks_a + bwd_blocks(n_b_rows)), dim3(THREADS), 0, stream, pa, qb,
                           ia, ib, a_rowptr, a_perm, b_rowptr, b_perm, okey, orowptr, ds, gamma, dpa, dqb, slab, (int)n_a_rows,
                           (int)n_b_rows, blocks_a, (int)C, (int)mean, eps, bwd_rpw(n_a_rows), bwd_rpw(n_b_rows), seed,
                           drop_threshold(p), drop_inv_keep(p));
        EQH_CHECK_LAUNCH();
        return eqh_reduce_slabs3_async(slab, blocks_a, 2 * (int64_t)C, dgamma, dbeta, nullptr, C, C, accumulate, stream);
    });
}
