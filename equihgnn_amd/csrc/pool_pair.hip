// Paired read-out of the models that pool nodes AND high-order hyperedges (equihnn_fa_former.py:99-101, mhnn.py:58,72):
//
//   out[b, 0:C]  = sum of the x rows of molecule b                         (global_add_pool(x, batch))
//   out[b, C:2C] = sum of the e rows of molecule b whose e_order > 2       (global_add_pool(e[e_order > 2], he_batch))
//
// written side by side into the [B, 2C] input of the output MLP: one launch instead of a mask tensor, an [M, C] multiply,
// two segment reduces and a concatenation, and one launch instead of four on the way back.
//
// HBM-bound.  Forward: one wavefront per (molecule, half) segment, the row in registers as row.h lays it out (float4 per
// lane, 1 KiB per load instruction at C = 256).  The 64 lanes first read the segment's entries -- and, for the hyperedge
// half, their e_order -- side by side; a ballot leaves the mask of the rows that count, and only those are loaded, up to
// four in flight, each address wave-uniform.  A bond hyperedge (order 2: all but about one per molecule) is therefore never
// read.  Rows are added in entry order whatever the mask: the sum is bitwise reproducible.  No atomics, no LDS.
// Backward: a row gather, dx[i] = dout[batch[i], 0:C], de[j] = dout[mol[j], C:2C] or zero; every row is written.
// Algorithmic bytes: forward 4C (N + M') + 4 (N + M) + 8 M + 8 (B + 1) + 8 C B (M' <= M rows of order > 2),
// backward 4C (N + M) written + 4 (N + M) + 8 M + 8 C B read.
#include "row.h"
#include "wave.h"

namespace {

constexpr int WAVES = 4;        // wavefronts (segments) per workgroup
constexpr int IN_FLIGHT = 4;    // source rows loaded before the first add

template <int NV>
__global__ void __launch_bounds__(64 * WAVES)
k_pool_pair_fwd(const float* __restrict__ x, const int* __restrict__ x_rowptr, const int* __restrict__ x_perm, int n_x,
                const float* __restrict__ e, const int* __restrict__ e_rowptr, const int* __restrict__ e_perm,
                const int64_t* __restrict__ e_order, int n_e, float* __restrict__ out, int64_t B, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t s = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); s < 2 * B; s += stride) {
        const bool he = s >= B;
        const int64_t b = he ? s - B : s;
        const float* __restrict__ src = he ? e : x;
        const int* __restrict__ rowptr = he ? e_rowptr : x_rowptr;
        const int* __restrict__ perm = he ? e_perm : x_perm;
        const int n_src = he ? n_e : n_x;
        Row<NV> acc;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc.v[i] = f4_zero();
        const int beg = n_src > 0 ? rowptr[b] : 0, end = n_src > 0 ? rowptr[b + 1] : 0;
        for (int q0 = beg; q0 < end; q0 += 64) {
            // lane l looks at entry q0 + l: its source row, or -1 for a null / out-of-range entry and a hyperedge of order <= 2
            int j = -1;
            if (q0 + lane < end) {
                j = perm ? perm[q0 + lane] : q0 + lane;
                if (j < 0 || j >= n_src || (he && e_order[j] <= 2)) j = -1;
            }
            unsigned long long live = __ballot(j >= 0);
            while (live) {
                int row[IN_FLIGHT];
#pragma unroll
                for (int u = 0; u < IN_FLIGHT; ++u) {
                    row[u] = -1;
                    if (live) {
                        row[u] = __float_as_int(bcast(__int_as_float(j), __ffsll(live) - 1));
                        live &= live - 1;
                    }
                }
                Row<NV> v[IN_FLIGHT];   // (an empty slot of the last group: a row of width 0, which load_row holds as zeros)
#pragma unroll
                for (int u = 0; u < IN_FLIGHT; ++u)
                    load_row<NV>(src + (int64_t)(row[u] < 0 ? 0 : row[u]) * C, 0, row[u] < 0 ? 0 : C, lane, v[u]);
#pragma unroll
                for (int u = 0; u < IN_FLIGHT; ++u)
#pragma unroll
                    for (int i = 0; i < NV; ++i) f4_add(acc.v[i], v[u].v[i]);
            }
        }
        float* __restrict__ dst = out + b * 2 * C + (he ? C : 0);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < C) *reinterpret_cast<float4*>(dst + c) = acc.v[i];
        }
    }
}

// Rows 0 .. n_x - 1 are dx's, the next n_e are de's.  A row is covered by 1 << lpr_log2 lanes (the power of two >= C / 4,
// at most 64), each moving one float4 per 4 << lpr_log2 channels.
__global__ void __launch_bounds__(256)
k_pool_pair_bwd(const float* __restrict__ dout, const int* __restrict__ x_mol, int64_t n_x, const int* __restrict__ e_mol,
                const int64_t* __restrict__ e_order, int64_t n_e, float* __restrict__ dx, float* __restrict__ de, int64_t B,
                int C, int lpr_log2) {
    const int lpr = 1 << lpr_log2;
    const int sl = threadIdx.x & (lpr - 1);
    const int64_t rows_per_block = 256 >> lpr_log2;
    for (int64_t r = (int64_t)blockIdx.x * rows_per_block + (threadIdx.x >> lpr_log2); r < n_x + n_e;
         r += (int64_t)gridDim.x * rows_per_block) {
        const bool he = r >= n_x;
        const int64_t i = he ? r - n_x : r;
        int mol = he ? e_mol[i] : x_mol[i];
        if (mol >= B || (he && e_order[i] <= 2)) mol = -1;     // (a negative molecule id is a null row already)
        const float* __restrict__ src = dout + (int64_t)(mol < 0 ? 0 : mol) * 2 * C + (he ? C : 0);
        float* __restrict__ dst = (he ? de : dx) + i * C;
        for (int c = sl * 4; c < C; c += lpr * 4)
            *reinterpret_cast<float4*>(dst + c) = mol < 0 ? f4_zero() : *reinterpret_cast<const float4*>(src + c);
    }
}

constexpr int64_t MAX_ROWS = ((int64_t)1 << 31) - 1;   // rows and CSR entries are int32

int check_common(const void* a, const void* b, int64_t n_x, int64_t n_e, int64_t B, int32_t C) {
    if (n_x < 0 || n_e < 0 || B < 0 || C <= 0) return EQH_ERR_ARG;
    if ((C & 3) || !eqh_aligned16(a) || !eqh_aligned16(b)) return EQH_ERR_ALIGN;
    if (C > 1024 || n_x >= MAX_ROWS || n_e >= MAX_ROWS || B >= MAX_ROWS / 2) return EQH_ERR_RANGE;
    return EQH_OK;
}

}  // namespace

extern "C" int hg_pool_pair_fwd(const float* x, const int32_t* x_rowptr, const int32_t* x_perm, int64_t n_x, const float* e,
                                const int32_t* e_rowptr, const int32_t* e_perm, const int64_t* e_order, int64_t n_e,
                                float* out, int64_t B, int32_t C, void* stream_) {
    if (const int rc = check_common(x, out, n_x, n_e, B, C)) return rc;
    if (B == 0) return EQH_OK;
    if (!out || (n_x > 0 && (!x || !x_rowptr)) || (n_e > 0 && (!e || !e_rowptr || !e_order))) return EQH_ERR_ARG;
    if (!eqh_aligned16(e)) return EQH_ERR_ALIGN;
    const int grid = eqh_grid_for(2 * B, WAVES, 256 * 16);      // grid-stride past 4096 workgroups
    return dispatch_nv(C, [&](auto nv) {
        hipLaunchKernelGGL((k_pool_pair_fwd<decltype(nv)::value>), dim3(grid), dim3(64 * WAVES), 0,
                           static_cast<hipStream_t>(stream_), x, x_rowptr, x_perm, (int)n_x, e, e_rowptr, e_perm, e_order,
                           (int)n_e, out, B, C);
        EQH_CHECK_LAUNCH();
        return (int)EQH_OK;
    });
}

extern "C" int hg_pool_pair_bwd(const float* dout, const int32_t* x_mol, int64_t n_x, const int32_t* e_mol,
                                const int64_t* e_order, int64_t n_e, float* dx, float* de, int64_t B, int32_t C,
                                void* stream_) {
    if (const int rc = check_common(dout, dx, n_x, n_e, B, C)) return rc;
    if (n_x + n_e == 0) return EQH_OK;
    if ((n_x > 0 && (!dx || !x_mol)) || (n_e > 0 && (!de || !e_mol || !e_order)) || (B > 0 && !dout)) return EQH_ERR_ARG;
    if (!eqh_aligned16(de)) return EQH_ERR_ALIGN;
    int lpr_log2 = 0;
    while (lpr_log2 < 6 && (4 << lpr_log2) < C) ++lpr_log2;
    const int grid = eqh_grid_for(n_x + n_e, 256 >> lpr_log2, 256 * 16);
    hipLaunchKernelGGL(k_pool_pair_bwd, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream_), dout, x_mol, n_x, e_mol,
                       e_order, n_e, dx, de, B, C, lpr_log2);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}
