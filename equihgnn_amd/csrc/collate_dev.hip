// Batch assembly from a store that lives in device memory (batch.DeviceMolStore / DeviceGraphStore): the bytes hb_collate /
// gb_collate (collate.hip, host code) write for the same store, idx and extents, produced by two capturable launches -- no
// host thread, no pinned staging, no host-to-device block per batch.
//
//   k_scan  ONE workgroup of 256 threads walks the B molecules in chunks of 256 with a running carry (the pattern of
//           csr_build.hip's block_exclusive_scan, int64 and K columns at once): per molecule the exclusive prefix of each
//           count column and the first source row, into the workspace; totals and the status word into out_counts.
//   k_fill  one work item per output element; a node row, incidence or hyperedge row finds its molecule by binary search in
//           the prefix (10 steps at B = 1024, all L1 / L2 hits: 8 KiB per column), so consecutive lanes store consecutive
//           elements whatever the molecule sizes are.  The item ranges of the fields are rounded up to the block size, so a
//           workgroup never straddles two fields.  No atomics; every element of every field has exactly one writer.
//
// Workspace: int64 [2 K][B + 1] -- prefix[k][0..B] (prefix[k][B] = the total), then start[k][0..B).
#include "common.h"

namespace {

constexpr int CD_THREADS = 256;
constexpr int CD_WAVES = CD_THREADS / EQH_WAVE;
constexpr int CD_GRID_CAP = 2048;

template <int K>
struct ScanArgs {
    const int64_t* idx;
    const int64_t* off[K];
    int64_t B, n_mols;
    int64_t ext[K];          // PN, PM, PZ  /  PN, PE
    int strict[K];           // padded: extent k must EXCEED its total (the padding molecule's own row)
    int padded;
    int64_t* ws;
    int64_t* out_counts;
};

// exclusive prefixes of K int64 values per thread over the block, and the block totals
template <int K>
__device__ __forceinline__ void block_scan_k(const int64_t (&v)[K], int64_t (&ex)[K], int64_t (&total)[K],
                                             int64_t (*wave_sum)[CD_WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int64_t inc = v[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wave_sum[k][wave] = inc;
        ex[k] = inc - v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int64_t base = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < CD_WAVES; ++w) {
            const int64_t s = wave_sum[k][w];
            if (w < wave) base += s;
            tot += s;
        }
        ex[k] += base;
        total[k] = tot;
    }
    __syncthreads();
}

template <int K>
__global__ void __launch_bounds__(CD_THREADS) k_scan(const ScanArgs<K> a) {
    __shared__ int64_t wave_sum[K][CD_WAVES];
    const int64_t B = a.B, ld = B + 1;
    int64_t carry[K];
#pragma unroll
    for (int k = 0; k < K; ++k) carry[k] = 0;
    int bad = 0;
    for (int64_t c0 = 0; c0 < B; c0 += CD_THREADS) {
        const int64_t b = c0 + threadIdx.x;
        int64_t cnt[K], start[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cnt[k] = start[k] = 0;
        if (b < B) {
            const int64_t m = a.idx[b];
            if (m >= 0 && m < a.n_mols) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    start[k] = a.off[k][m];
                    cnt[k] = a.off[k][m + 1] - start[k];
                    if (cnt[k] < 0) cnt[k] = 0;     // (offsets are checked before the upload; never index backwards)
                }
            } else {
                bad = 1;
            }
        }
        int64_t ex[K], total[K];
        block_scan_k<K>(cnt, ex, total, wave_sum);
        if (b < B) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                a.ws[k * ld + b] = carry[k] + ex[k];
                a.ws[(K + k) * ld + b] = start[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) carry[k] += total[k];
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        int misfit = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            a.ws[k * ld + B] = carry[k];
            a.ws[(K + k) * ld + B] = 0;
            a.out_counts[k] = carry[k];
            if (a.padded ? (a.strict[k] ? a.ext[k] <= carry[k] : a.ext[k] < carry[k]) : a.ext[k] != carry[k]) misfit = 1;
        }
        a.out_counts[K] = (bad ? 1 : 0) | (misfit ? 2 : 0);
        if (K < 3) a.out_counts[3] = 0;
    }
}

// the molecule that owns output row `row` (row < prefix[B]): the smallest b with prefix[b + 1] > row
__device__ __forceinline__ int64_t owner_of(const int64_t* __restrict__ prefix, int64_t B, int64_t row) {
    int64_t lo = 0, hi = B - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (prefix[mid + 1] <= row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a / b for non-negative operands: 64-bit division is a long software sequence on the vector ALU; every extent of a real batch
// fits 31 bits, where the quotient is one multiply-high (constant b) or a short 32-bit sequence
__device__ __forceinline__ int64_t div_nn(int64_t a, int64_t b) {
    return (((a | b) >> 31) == 0) ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

__host__ __device__ __forceinline__ int64_t round_up(int64_t v) { return (v + CD_THREADS - 1) / CD_THREADS * CD_THREADS; }

__global__ void __launch_bounds__(CD_THREADS) k_fill_h(const HbCollateDev q) {
    const int64_t B = q.B, ld = B + 1;
    const int64_t* __restrict__ ws = static_cast<const int64_t*>(q.workspace);
    const int64_t *pre_n = ws, *pre_h = ws + ld, *pre_z = ws + 2 * ld;
    const int64_t *st_n = ws + 3 * ld, *st_h = ws + 4 * ld, *st_z = ws + 5 * ld;
    const int64_t N = pre_n[B], M = pre_h[B], Z = pre_z[B];
    const int64_t PN = q.PN, PM = q.PM, PZ = q.PZ, PB = B + (q.padded ? 1 : 0);
    // item ranges, each rounded up to the block: x elements, pos elements, batch rows, incidences, hyperedge rows, molecules
    const int64_t s1 = round_up(PN * 9), s2 = s1 + round_up(PN * 3), s3 = s2 + round_up(PN), s4 = s3 + round_up(PZ),
                  s5 = s4 + round_up(PM), s6 = s5 + round_up(PB);
    for (int64_t t0 = (int64_t)blockIdx.x * CD_THREADS; t0 < s6; t0 += (int64_t)gridDim.x * CD_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        if (t0 < s1) {
            if (t < PN * 9) {
                const int64_t row = div_nn(t, 9), col = t - row * 9;
                int64_t val = 0;
                if (row < N) {
                    const int64_t b = owner_of(pre_n, B, row);
                    val = q.x[(st_n[b] + (row - pre_n[b])) * 9 + col];
                }
                q.out_x[t] = val;
            }
        } else if (t0 < s2) {
            const int64_t i = t - s1;
            if (i < PN * 3) {
                const int64_t row = div_nn(i, 3), col = i - row * 3;
                float val;
                if (row < N) {
                    const int64_t b = owner_of(pre_n, B, row);
                    val = q.pos[(st_n[b] + (row - pre_n[b])) * 3 + col];
                } else {
                    val = col == 0 ? 1.0e4f + 10.0f * (float)(row - N) : 0.f;
                }
                q.out_pos[i] = val;
            }
        } else if (t0 < s3) {
            const int64_t row = t - s2;
            if (row < PN) q.out_batch[row] = row < N ? owner_of(pre_n, B, row) : B;
        } else if (t0 < s4) {
            const int64_t i = t - s3;
            if (i < PZ) {
                int64_t vv = -1, ee = -1;
                if (i < Z) {
                    const int64_t b = owner_of(pre_z, B, i);
                    const int64_t src = st_z[b] + (i - pre_z[b]);
                    vv = q.v[src] + pre_n[b];
                    ee = q.e[src] + pre_h[b];
                }
                q.out_edge_index0[i] = vv;
                q.out_edge_index1[i] = ee;
            }
        } else if (t0 < s5) {
            const int64_t j = t - s4;
            if (j < PM) {
                int64_t attr = 0, order = 0;
                if (j < M) {
                    const int64_t b = owner_of(pre_h, B, j);
                    const int64_t src = st_h[b] + (j - pre_h[b]);
                    attr = q.edge_attr[src];
                    order = q.e_order[src];
                }
                q.out_edge_attr[j] = attr;
                q.out_e_order[j] = order;
            }
        } else {
            const int64_t b = t - s5;
            if (b < PB) {
                int64_t ne = PM - M;        // the padding molecule's
                float yy = 0.f;
                if (b < B) {
                    ne = pre_h[b + 1] - pre_h[b];
                    const int64_t m = q.idx[b];
                    if (m >= 0 && m < q.n_mols) yy = q.y[m];
                }
                q.out_n_e[b] = ne;
                q.out_y[b] = yy;
            }
        }
    }
}

__global__ void __launch_bounds__(CD_THREADS) k_fill_g(const GbCollateDev q) {
    const int64_t B = q.B, ld = B + 1, F = q.F;
    const int64_t* __restrict__ ws = static_cast<const int64_t*>(q.workspace);
    const int64_t *pre_n = ws, *pre_e = ws + ld, *st_n = ws + 2 * ld, *st_e = ws + 3 * ld;
    const int64_t N = pre_n[B], E = pre_e[B];
    const int64_t PN = q.PN, PE = q.PE, PB = B + (q.padded ? 1 : 0);
    const int64_t pn = PN - N > 0 ? PN - N : 1;       // (a misfit is reported by the scan; never divide by zero)
    // item ranges: x elements, batch rows, edges (both rows of edge_index), edge_attr elements, molecules
    const int64_t s1 = round_up(PN * 9), s2 = s1 + round_up(PN), s3 = s2 + round_up(PE), s4 = s3 + round_up(PE * F),
                  s5 = s4 + round_up(PB);
    for (int64_t t0 = (int64_t)blockIdx.x * CD_THREADS; t0 < s5; t0 += (int64_t)gridDim.x * CD_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        if (t0 < s1) {
            if (t < PN * 9) {
                const int64_t row = div_nn(t, 9), col = t - row * 9;
                int64_t val = 0;
                if (row < N) {
                    const int64_t b = owner_of(pre_n, B, row);
                    val = q.x[(st_n[b] + (row - pre_n[b])) * 9 + col];
                }
                q.out_x[t] = val;
            }
        } else if (t0 < s2) {
            const int64_t row = t - s1;
            if (row < PN) q.out_batch[row] = row < N ? owner_of(pre_n, B, row) : B;
        } else if (t0 < s3) {
            const int64_t i = t - s2;
            if (i < PE) {
                int64_t s, d;
                if (i < E) {
                    const int64_t b = owner_of(pre_e, B, i);
                    const int64_t src = st_e[b] + (i - pre_e[b]);
                    s = q.src[src] + pre_n[b];
                    d = q.dst[src] + pre_n[b];
                } else {                    // a ring over the padded atoms (pn == 1: self-loops)
                    const int64_t k = i - E;
                    s = N + (k - div_nn(k, pn) * pn);
                    d = N + (k + 1 - div_nn(k + 1, pn) * pn);
                }
                q.out_edge_index[i] = s;
                q.out_edge_index[PE + i] = d;
            }
        } else if (t0 < s4) {
            const int64_t i = t - s3;
            if (i < PE * F) {
                const int64_t row = div_nn(i, F), col = i - row * F;
                int64_t val = 0;
                if (row < E) {
                    const int64_t b = owner_of(pre_e, B, row);
                    val = q.edge_attr[(st_e[b] + (row - pre_e[b])) * F + col];
                }
                q.out_edge_attr[i] = val;
            }
        } else {
            const int64_t b = t - s4;
            if (b < PB) {
                float yy = 0.f;
                if (b < B) {
                    const int64_t m = q.idx[b];
                    if (m >= 0 && m < q.n_mols) yy = q.y[m];
                }
                q.out_y[b] = yy;
            }
        }
    }
}

}  // namespace

extern "C" int64_t hb_collate_dev_workspace_bytes(int64_t B) {
    return 6 * ((B < 0 ? 0 : B) + 1) * (int64_t)sizeof(int64_t);
}

extern "C" int64_t gb_collate_dev_workspace_bytes(int64_t B) {
    return 4 * ((B < 0 ? 0 : B) + 1) * (int64_t)sizeof(int64_t);
}

extern "C" int hb_collate_dev(const HbCollateDev* q, void* stream_) {
    if (!q || q->B < 0 || q->n_mols < 0 || q->PN < 0 || q->PM < 0 || q->PZ < 0 || !q->out_counts) return EQH_ERR_ARG;
    const int64_t B = q->B, PB = B + (q->padded ? 1 : 0);
    if (B > 0 && (!q->idx || !q->node_off || !q->he_off || !q->inc_off || !q->y)) return EQH_ERR_ARG;
    const struct { const void* p; int64_t extent; } need[] = {
        {q->out_x, q->PN}, {q->out_pos, q->PN}, {q->out_batch, q->PN}, {q->out_edge_index0, q->PZ},
        {q->out_edge_index1, q->PZ}, {q->out_edge_attr, q->PM}, {q->out_e_order, q->PM}, {q->out_n_e, PB}, {q->out_y, PB}};
    for (const auto& a : need)
        if (!a.p && a.extent > 0) return EQH_ERR_ARG;
    if (!q->workspace || q->workspace_bytes < hb_collate_dev_workspace_bytes(B)) return EQH_ERR_ARG;
    // the padding molecule needs a node and a hyperedge of its own, whatever the batch holds
    if (q->padded && (q->PN < 1 || q->PM < 1)) return EQH_ERR_RANGE;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ScanArgs<3> s{q->idx, {q->node_off, q->he_off, q->inc_off}, B, q->n_mols, {q->PN, q->PM, q->PZ}, {1, 1, 0},
                  q->padded ? 1 : 0, static_cast<int64_t*>(q->workspace), q->out_counts};
    hipLaunchKernelGGL(k_scan<3>, dim3(1), dim3(CD_THREADS), 0, stream, s);
    EQH_CHECK_LAUNCH();
    const int64_t items = round_up(q->PN * 9) + round_up(q->PN * 3) + round_up(q->PN) + round_up(q->PZ) + round_up(q->PM) +
                          round_up(PB);
    if (items > 0) {
        hipLaunchKernelGGL(k_fill_h, dim3(eqh_grid_for(items, CD_THREADS, CD_GRID_CAP)), dim3(CD_THREADS), 0, stream, *q);
        EQH_CHECK_LAUNCH();
    }
    return EQH_OK;
}

extern "C" int gb_collate_dev(const GbCollateDev* q, void* stream_) {
    if (!q || q->B < 0 || q->n_mols < 0 || q->F < 0 || q->PN < 0 || q->PE < 0 || !q->out_counts) return EQH_ERR_ARG;
    const int64_t B = q->B, PB = B + (q->padded ? 1 : 0);
    if (B > 0 && (!q->idx || !q->node_off || !q->edge_off || !q->y)) return EQH_ERR_ARG;
    const struct { const void* p; int64_t extent; } need[] = {
        {q->out_x, q->PN}, {q->out_batch, q->PN}, {q->out_edge_index, q->PE}, {q->out_edge_attr, q->PE * q->F}, {q->out_y, PB}};
    for (const auto& a : need)
        if (!a.p && a.extent > 0) return EQH_ERR_ARG;
    if (!q->workspace || q->workspace_bytes < gb_collate_dev_workspace_bytes(B)) return EQH_ERR_ARG;
    if (q->padded && q->PN < 1) return EQH_ERR_RANGE;      // the padding molecule needs an atom of its own
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ScanArgs<2> s{q->idx, {q->node_off, q->edge_off}, B, q->n_mols, {q->PN, q->PE}, {1, 0}, q->padded ? 1 : 0,
                  static_cast<int64_t*>(q->workspace), q->out_counts};
    hipLaunchKernelGGL(k_scan<2>, dim3(1), dim3(CD_THREADS), 0, stream, s);
    EQH_CHECK_LAUNCH();
    const int64_t items = round_up(q->PN * 9) + round_up(q->PN) + round_up(q->PE) + round_up(q->PE * q->F) + round_up(PB);
    if (items > 0) {
        hipLaunchKernelGGL(k_fill_g, dim3(eqh_grid_for(items, CD_THREADS, CD_GRID_CAP)), dim3(CD_THREADS), 0, stream, *q);
        EQH_CHECK_LAUNCH();
    }
    return EQH_OK;
}
