// Edge messages of the 2-D baselines (baseline_2d.py:19-73: GINConv / GCNConv, PyG flow source_to_target,
// aggregation "add") without the [E, C] bond-embedding tensor and without atomics.
//
//   GIN: out_i = (1 + eps) x_i + sum_{e: dst(e)=i} relu(x[src_e] + bond(e))
//   GCN: out_i = sum_{e: dst(e)=i} norm_e relu(x[src_e] + bond(e)) + relu(x_i + root) / deg_i
//        deg_i = #{e: src(e)=i} + 1 (degree(row), counted on SOURCES), norm_e = deg^-1/2[src] deg^-1/2[dst]
//
// bond(e) = sum_f table[code_f(e)]: the <= 4 bond tables (<= 16 rows, ogb BondEncoder) are summed on the fly -- from LDS
// in the forward; the backward, whose LDS holds the gradient partials, reads them from global memory (15.6 KB at C = 300,
// cache-resident).  The
// per-entry codes (one int32, 8 bits per column) are written once per batch in CSR order by hg_edge_codes, so a
// message costs one index load and one row gather.
//
// Row-to-lane mapping (both kernels): a row of C floats is C4 = C / 4 float4 lanes, and a 256-thread workgroup packs
// P = 256 / C4 such lane groups back to back (group g = tid / C4); the leftover 256 - P C4 threads idle.  At C = 300
// (C4 = 75) this is 3 rows per workgroup and 225 of 256 lanes busy (88 %); a group may straddle two wavefronts, which
// costs nothing because each group's gathers are one contiguous 16-byte-per-lane run.  The alternative of one
// wavefront per row leaves 53 of 128 lane-slots idle at C = 300 (59 %), and 16-lane groups with a loop over 5 float4
// per lane re-issue every index load five times.  Every lane keeps exactly one float4 of the row, so the backward
// pass can keep its per-lane bond-gradient partials in LDS slots that no other lane touches.
//
// Forward walks the CSR of incoming edges (by dst) in ascending edge id -- the order of PyG's scatter-add -- and the
// self term is added after the sum, as GINConv / GCNConv do.  Backward walks the CSR of outgoing edges (by src):
//   dx_j = sum_{e: src(e)=j} w_e [x_j + bond(e) > 0] dout[dst_e] + d self_j
// with the ReLU mask recomputed (no pre-activation is stored; no symmetry of the graph is assumed).  The same per-edge
// product is the gradient of bond(e): it is added to the lane's LDS partial of each selected table row; at the end
// of a workgroup the P groups' partials are combined in group order into one slab per workgroup, and the slabs are
// summed in workgroup order by the common slab reducer (optionally inside the deferred-reduction window).  The last
// slab row carries d root (GCN, per channel) or d eps (GIN, element 0; the workgroup's channels summed in order).
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_F = 4;
constexpr int MAX_T = 16;
constexpr int BWD_ROWS_PER_BLOCK = 32;
constexpr int BWD_MAX_BLOCKS = 2048;

__device__ __forceinline__ float4 f4_relu_add(const float4& a, const float4& b) {
    return make_float4(fmaxf(a.x + b.x, 0.f), fmaxf(a.y + b.y, 0.f), fmaxf(a.z + b.z, 0.f), fmaxf(a.w + b.w, 0.f));
}
__device__ __forceinline__ void f4_add_scaled(float4& acc, const float4& v, float w) {   // acc + (w * v): two roundings
    acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
}
__device__ __forceinline__ float4 f4_masked(const float4& pre, const float4& g, float w) {   // w [pre > 0] g
    return make_float4(pre.x > 0.f ? w * g.x : 0.f, pre.y > 0.f ? w * g.y : 0.f, pre.z > 0.f ? w * g.z : 0.f,
                       pre.w > 0.f ? w * g.w : 0.f);
}
__device__ __forceinline__ float inv_sqrt_deg(const int32_t* __restrict__ rowptr, int64_t i) {
    return 1.f / sqrtf((float)(rowptr[i + 1] - rowptr[i] + 1));
}

struct Codes { int off[MAX_F]; int dim[MAX_F]; };

__global__ void __launch_bounds__(THREADS)
k_edge_codes(const int64_t* __restrict__ attr, int F, Codes cd, const int32_t* __restrict__ eid, int64_t nnz,
             int32_t* __restrict__ code) {
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < nnz; q += stride) {
        const int64_t e = eid[q];
        int32_t c = 0;
        for (int f = 0; f < F; ++f) {
            int64_t a = attr[e * F + f];
            a = a < 0 ? 0 : (a >= cd.dim[f] ? cd.dim[f] - 1 : a);   // ogb's tables would raise; never read outside
            c |= (int32_t)(cd.off[f] + a) << (8 * f);
        }
        code[q] = c;
    }
}

// bond row of one edge from LDS (forward) or global memory (backward): 0 + t_0 + t_1 + ... as ogb sums
template <typename P4>
__device__ __forceinline__ float4 bond_row(P4 tab, int32_t code, int F, int C4, int c) {
    float4 b = f4_zero();
    for (int f = 0; f < F; ++f) f4_add(b, tab[((code >> (8 * f)) & 255) * C4 + c]);
    return b;
}

template <bool GCN>
__global__ void __launch_bounds__(THREADS)
k_edge_msg_fwd(const float4* __restrict__ x, const float4* __restrict__ tables, int T, int F,
               const int32_t* __restrict__ in_rowptr, const int32_t* __restrict__ in_src,
               const int32_t* __restrict__ in_code, const int32_t* __restrict__ out_rowptr,
               const float* __restrict__ eps, const float4* __restrict__ root, int64_t N, int C4,
               float4* __restrict__ out) {
    extern __shared__ float4 s_tab[];
    for (int i = threadIdx.x; i < T * C4; i += THREADS) s_tab[i] = tables[i];
    __syncthreads();
    const int P = THREADS / C4, g = threadIdx.x / C4, c = threadIdx.x - g * C4;
    if (g >= P) return;
    const float one_eps = GCN ? 0.f : 1.f + eps[0];
    const float4 rt = GCN ? root[c] : f4_zero();
    for (int64_t i = (int64_t)blockIdx.x * P + g; i < N; i += (int64_t)gridDim.x * P) {
        const int q0 = in_rowptr[i], q1 = in_rowptr[i + 1];
        const float dis_i = GCN ? inv_sqrt_deg(out_rowptr, i) : 1.f;
        float4 acc = f4_zero();
        for (int q = q0; q < q1; ++q) {
            const int64_t j = in_src[q];
            if ((uint64_t)j >= (uint64_t)N) continue;     // (never in a valid batch: no read outside x)
            const float4 m = f4_relu_add(x[j * C4 + c], bond_row(s_tab, F > 0 ? in_code[q] : 0, F, C4, c));
            if (GCN) f4_add_scaled(acc, m, inv_sqrt_deg(out_rowptr, j) * dis_i);
            else f4_add(acc, m);
        }
        const float4 xi = x[i * C4 + c];
        float4 o;
        if (GCN) {
            const float deg = (float)(out_rowptr[i + 1] - out_rowptr[i] + 1);
            const float4 s = f4_relu_add(xi, rt);
            o = make_float4(acc.x + s.x / deg, acc.y + s.y / deg, acc.z + s.z / deg, acc.w + s.w / deg);
        } else {
            o = make_float4(one_eps * xi.x + acc.x, one_eps * xi.y + acc.y, one_eps * xi.z + acc.z,
                            one_eps * xi.w + acc.w);
        }
        out[i * C4 + c] = o;
    }
}

// grid = n_blocks; block b owns source rows [b R, (b + 1) R) and writes its table partials [T, C] to slab_t + b T C and its
// d root / d eps partial [C] to slab_e + b C (two regions: the tables' reduction may accumulate and be deferred, d root /
// d eps is always reduced at once)
template <bool GCN>
__global__ void __launch_bounds__(THREADS)
k_edge_msg_bwd(const float4* __restrict__ x, const float4* __restrict__ tables, int T, int F,
               const int32_t* __restrict__ out_rowptr, const int32_t* __restrict__ out_dst,
               const int32_t* __restrict__ out_code, const float* __restrict__ eps, const float4* __restrict__ root,
               const float4* __restrict__ dout, int64_t N, int C4, int64_t rows_per_block, float4* __restrict__ dx,
               float4* __restrict__ slab_t, float4* __restrict__ slab_e) {
    extern __shared__ float4 s_part[];          // [P][T + 1][C4]
    const int P = THREADS / C4, g = threadIdx.x / C4, c = threadIdx.x - g * C4;
    const int TE = T + 1;
    for (int i = threadIdx.x; i < P * TE * C4; i += THREADS) s_part[i] = f4_zero();
    __syncthreads();
    if (g < P) {
        float4* part = s_part + (int64_t)g * TE * C4 + c;
        const float one_eps = GCN ? 0.f : 1.f + eps[0];
        const float4 rt = GCN ? root[c] : f4_zero();
        float4 extra = f4_zero();
        const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
        const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
        for (int64_t j = r0 + g; j < r1; j += P) {
            const int q0 = out_rowptr[j], q1 = out_rowptr[j + 1];
            const float4 xj = x[j * C4 + c];
            const float dis_j = GCN ? 1.f / sqrtf((float)(q1 - q0 + 1)) : 1.f;
            float4 acc = f4_zero();
            for (int q = q0; q < q1; ++q) {
                const int64_t i = out_dst[q];
                if ((uint64_t)i >= (uint64_t)N) continue;
                const int32_t code = F > 0 ? out_code[q] : 0;
                const float w = GCN ? inv_sqrt_deg(out_rowptr, i) * dis_j : 1.f;
                float4 pre = xj;
                f4_add(pre, bond_row(tables, code, F, C4, c));
                const float4 gq = f4_masked(pre, dout[i * C4 + c], w);
                f4_add(acc, gq);
                for (int f = 0; f < F; ++f) f4_add(part[((code >> (8 * f)) & 255) * C4], gq);
            }
            const float4 dj = dout[j * C4 + c];
            if (GCN) {
                const float deg = (float)(q1 - q0 + 1);
                const float4 pre = make_float4(xj.x + rt.x, xj.y + rt.y, xj.z + rt.z, xj.w + rt.w);
                const float4 s = make_float4(pre.x > 0.f ? dj.x / deg : 0.f, pre.y > 0.f ? dj.y / deg : 0.f,
                                             pre.z > 0.f ? dj.z / deg : 0.f, pre.w > 0.f ? dj.w / deg : 0.f);
                f4_add(extra, s);
                f4_add(acc, s);
            } else {
                extra.x += xj.x * dj.x; extra.y += xj.y * dj.y; extra.z += xj.z * dj.z; extra.w += xj.w * dj.w;
                f4_add_scaled(acc, dj, one_eps);
            }
            dx[j * C4 + c] = acc;
        }
        part[T * C4] = extra;
    }
    __syncthreads();
    // the P groups' partials, combined in group order
    float4* out_t = slab_t + (int64_t)blockIdx.x * T * C4;
    float4* out_e = slab_e + (int64_t)blockIdx.x * C4;
    for (int k = threadIdx.x; k < TE * C4; k += THREADS) {
        float4 s = s_part[k];
        for (int h = 1; h < P; ++h) f4_add(s, s_part[(int64_t)h * TE * C4 + k]);
        if (k < T * C4) out_t[k] = s;
        else if (GCN) out_e[k - T * C4] = s;
        else s_part[k] = s;                            // (group 0's slot: read back below for d eps)
    }
    if (!GCN) {
        __syncthreads();
        if (threadIdx.x == 0) {
            float e = 0.f;
            for (int k = 0; k < C4; ++k) {
                const float4 v = s_part[T * C4 + k];
                e += ((v.x + v.y) + (v.z + v.w));
            }
            out_e[0] = make_float4(e, 0.f, 0.f, 0.f);
        }
        for (int k = 1 + threadIdx.x; k < C4; k += THREADS) out_e[k] = f4_zero();
    }
}

int bwd_blocks(int64_t N) {
    const int64_t b = (N + BWD_ROWS_PER_BLOCK - 1) / BWD_ROWS_PER_BLOCK;
    return (int)(b < 1 ? 1 : (b > BWD_MAX_BLOCKS ? BWD_MAX_BLOCKS : b));
}

int check_common(const float* x, const float* tables, int32_t T, int32_t F, int64_t N, int32_t C, int32_t mode,
                 const float* eps, const float* root) {
    if (N < 0 || C <= 0 || T < 0 || T > MAX_T || F < 0 || F > MAX_F || (F > 0 && T < 1)) return EQH_ERR_ARG;
    if (mode != 0 && mode != 1) return EQH_ERR_ARG;
    if (C % 4 || C / 4 > THREADS) return C % 4 ? EQH_ERR_ALIGN : EQH_ERR_ARG;
    if (N >= INT32_MAX) return EQH_ERR_RANGE;
    if (!x || (T > 0 && !tables) || (mode == 0 && !eps) || (mode == 1 && !root)) return EQH_ERR_ARG;
    if (!eqh_aligned16(x) || (tables && !eqh_aligned16(tables)) || (root && !eqh_aligned16(root))) return EQH_ERR_ALIGN;
    return EQH_OK;
}

}  // namespace

extern "C" int hg_edge_codes(const int64_t* edge_attr, int32_t F, const int32_t* off_host, int32_t T,
                             const int32_t* eid, int64_t nnz, int32_t* code, void* stream_) {
    if (nnz < 0 || F < 0 || F > MAX_F || T < 0 || T > MAX_T || (nnz > 0 && (!eid || !code || (F > 0 && !edge_attr))))
        return EQH_ERR_ARG;
    if (F > 0 && !off_host) return EQH_ERR_ARG;
    Codes cd{};
    for (int f = 0; f < F; ++f) {
        const int end = f + 1 < F ? off_host[f + 1] : T;
        cd.off[f] = off_host[f];
        cd.dim[f] = end - off_host[f];
        if (cd.off[f] < 0 || cd.dim[f] < 1 || end > T) return EQH_ERR_ARG;
    }
    if (nnz == 0) return EQH_OK;
    hipLaunchKernelGGL(k_edge_codes, dim3(eqh_grid_for(nnz, THREADS, 4096)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream_), edge_attr, F, cd, eid, nnz, code);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int hg_edge_msg_fwd(int32_t mode, const float* x, const float* tables, int32_t T, int32_t F,
                               const int32_t* in_rowptr, const int32_t* in_src, const int32_t* in_code,
                               const int32_t* out_rowptr, const float* eps, const float* root, int64_t N, int32_t C,
                               float* out, void* stream_) {
    int rc = check_common(x, tables, T, F, N, C, mode, eps, root);
    if (rc) return rc;
    if (N == 0) return EQH_OK;
    if (!in_rowptr || !in_src || (F > 0 && !in_code) || !out || (mode == 1 && !out_rowptr)) return EQH_ERR_ARG;
    if (!eqh_aligned16(out)) return EQH_ERR_ALIGN;
    const int C4 = C / 4, P = THREADS / C4;
    const int grid = eqh_grid_for(N, P, 16384);
    const size_t lds = (size_t)(T > 0 ? T : 1) * C4 * sizeof(float4);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    auto x4 = reinterpret_cast<const float4*>(x);
    auto t4 = reinterpret_cast<const float4*>(tables);
    auto r4 = reinterpret_cast<const float4*>(root);
    auto o4 = reinterpret_cast<float4*>(out);
    if (mode == 1)
        hipLaunchKernelGGL(k_edge_msg_fwd<true>, dim3(grid), dim3(THREADS), lds, stream, x4, t4, T, F, in_rowptr,
                           in_src, in_code, out_rowptr, eps, r4, N, C4, o4);
    else
        hipLaunchKernelGGL(k_edge_msg_fwd<false>, dim3(grid), dim3(THREADS), lds, stream, x4, t4, T, F, in_rowptr,
                           in_src, in_code, out_rowptr, eps, r4, N, C4, o4);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" size_t hg_edge_msg_bwd_workspace_bytes(int64_t N, int32_t C, int32_t T) {
    if (N < 0 || C <= 0 || T < 0) return 0;
    return (size_t)bwd_blocks(N) * (size_t)(T + 1) * (size_t)C * sizeof(float);
}

extern "C" int hg_edge_msg_bwd(int32_t mode, const float* x, const float* tables, int32_t T, int32_t F,
                               const int32_t* out_rowptr, const int32_t* out_dst, const int32_t* out_code,
                               const float* eps, const float* root, const float* dout, int64_t N, int32_t C,
                               float* dx, float* dtables, float* dextra, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, void* stream_) {
    int rc = check_common(x, tables, T, F, N, C, mode, eps, root);
    if (rc) return rc;
    if (!out_rowptr || !out_dst || (F > 0 && !out_code) || !dout || !dx || (T > 0 && !dtables) || !dextra)
        return EQH_ERR_ARG;
    if (!eqh_aligned16(dout) || !eqh_aligned16(dx)) return EQH_ERR_ALIGN;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (N == 0) {   // no rows: the parameter gradients are zero
        rc = accumulate ? EQH_OK : eqh_zero_async(dtables, (int64_t)T * C, stream);
        return rc ? rc : eqh_zero_async(dextra, C, stream);
    }
    const int blocks = bwd_blocks(N);
    if (!workspace || workspace_bytes < hg_edge_msg_bwd_workspace_bytes(N, C, T)) return EQH_ERR_ARG;
    const int C4 = C / 4, P = THREADS / C4;
    const int64_t rows_per_block = (N + blocks - 1) / blocks;
    const size_t lds = (size_t)P * (T + 1) * C4 * sizeof(float4);
    if (lds > 65536) return EQH_ERR_ARG;        // (T <= 13, the ogb bond tables, fits at every C)
    auto x4 = reinterpret_cast<const float4*>(x);
    auto t4 = reinterpret_cast<const float4*>(tables);
    auto r4 = reinterpret_cast<const float4*>(root);
    auto d4 = reinterpret_cast<const float4*>(dout);
    auto dx4 = reinterpret_cast<float4*>(dx);
    auto s4 = reinterpret_cast<float4*>(workspace);                 // [blocks][T][C4] table partials
    auto e4 = s4 + (int64_t)blocks * T * C4;                         // [blocks][C4] d root / d eps partials
    if (mode == 1)
        hipLaunchKernelGGL(k_edge_msg_bwd<true>, dim3(blocks), dim3(THREADS), lds, stream, x4, t4, T, F, out_rowptr,
                           out_dst, out_code, eps, r4, d4, N, C4, rows_per_block, dx4, s4, e4);
    else
        hipLaunchKernelGGL(k_edge_msg_bwd<false>, dim3(blocks), dim3(THREADS), lds, stream, x4, t4, T, F, out_rowptr,
                           out_dst, out_code, eps, r4, d4, N, C4, rows_per_block, dx4, s4, e4);
    EQH_CHECK_LAUNCH();
    // fixed-order reductions of the workgroup partials: dextra overwritten at once; dtables overwritten, or added to
    // (deferred inside a deferral window) with accumulate
    rc = eqh_reduce_slabs_async(reinterpret_cast<const float*>(e4), blocks, C, dextra, stream, 0);
    if (rc || T == 0) return rc;
    return eqh_reduce_slabs_async(static_cast<const float*>(workspace), blocks, (int64_t)T * C, dtables, stream, accumulate);
}
