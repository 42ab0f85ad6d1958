// ViSNet front-end (visnet_layer.py: Distance / ExpNormalSmearing / Sphere, NeighborEmbedding, EdgeEmbedding, ViS_MP) on
// a static radius graph, without atomics and without any [E, 8, C] tensor.
//
// Graph.  vis_radius_graph keeps, for every target atom i, the first K = 16 atoms j of i's molecule (ascending index, i
// itself included) whose fp32 squared distance, summed x, y, z, is strictly below r^2 -- torch_cluster's radius_graph
// (loop = True, max_num_neighbors = 16).  Edge e = i K + s is the s-th kept source of i: slot[e] = j, or -1 past cnt[i].
// Edges are thus ordered by target, then by source, and E_cap = K N is a static shape.  Atoms at index >= n_real (the
// dummy molecule of a padded batch) keep only their self-loop.  The transposed graph (edges by source) lives in the same
// per-molecule slot range: the src_cnt[j] edges of source j are src_eid[src_start[j] ...], ascending edge id.
//
// Per-slot geometry (no gradient: pos does not require one): r (0 for a self-loop), C(r) the cosine cutoff, the 32
// ExpNormalSmearing RBFs and the 8 real spherical harmonics (lmax 2) of the normalised edge vector pos[j] - pos[i] (all
// 0 for a self-loop, whose vector is not normalised).  Empty slots hold zeros and every kernel skips them: they
// contribute exactly 0 forward and backward, and every per-edge gradient row of an empty slot is written as 0.
//
// Row-to-lane mapping: one wavefront (64 lanes) per row; lane l owns channels l, l + 64, ... (C / 64 of them, at most
// 8: C = 64 is one channel per lane, C = 256 four).  Sums over a target's edges run in slot order inside the lane; sums
// over a source's edges run in the by-source order.  Per-head sums (8 heads of D = C / 8 channels) go through LDS, each
// head summed by one lane in channel order.  Every result is bitwise reproducible.
//
// Activations of the edge projections (silu of dk_proj, dv_proj, s_proj, f_proj) are applied inside the kernels on the
// raw Linear outputs, and their derivative is folded into the returned edge gradients.
#include "act.h"
#include "common.h"

namespace {

constexpr int K = 16;          // max_num_neighbors
constexpr int NRBF = 32;
constexpr int NSH = 8;         // (lmax + 1)^2 - 1
constexpr int HEADS = 8;
constexpr int LANES = 64;
constexpr int MAXV = 8;        // channels per lane: C <= 512
constexpr int GRID_CAP = 16384;

// SiLU as x * sigmoid_exact(x): a division, then a product (two roundings)
__device__ __forceinline__ float silu_exact(float x) { return x * sigmoid_exact(x); }
__device__ __forceinline__ float dsilu(float x) {
    const float s = sigmoid_exact(x);
    return s * (1.f + x * (1.f - s));
}

__device__ __forceinline__ int n_real_of(const int32_t* n_real, int64_t N) { return n_real ? n_real[0] : (int)N; }

// ---------------------------------------------------------------------------------------------------------------------
// graph
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_vis_radius(const float* __restrict__ pos, const int32_t* __restrict__ batch, const int32_t* __restrict__ pool_rowptr,
             const int32_t* __restrict__ n_real, int64_t N, float r2, int32_t* __restrict__ slot,
             int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t* sl = slot + i * K;
    int n = 0;
    if (i >= n_real_of(n_real, N)) {
        sl[n++] = (int32_t)i;
    } else {
        const int b = batch[i];
        const int a0 = pool_rowptr[b], a1 = pool_rowptr[b + 1];
        const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
        for (int j = a0; j < a1 && n < K; ++j) {
            const float dx = pos[3 * (int64_t)j] - xi, dy = pos[3 * (int64_t)j + 1] - yi, dz = pos[3 * (int64_t)j + 2] - zi;
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            if (d2 < r2) sl[n++] = j;
        }
    }
    cnt[i] = n;
    for (int s = n; s < K; ++s) sl[s] = -1;
}

// one thread per slot
__global__ void __launch_bounds__(256)
k_vis_geom(const float* __restrict__ pos, const int32_t* __restrict__ slot, const float* __restrict__ means,
           const float* __restrict__ betas, int64_t E, float cutoff, float* __restrict__ r_out,
           float* __restrict__ cut_out, float* __restrict__ rbf, float* __restrict__ sh) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t i = e / K;
    const int j = slot[e];
    float w = 0.f, c = 0.f;
    float v[NSH];
    for (int m = 0; m < NSH; ++m) v[m] = 0.f;
    if (j >= 0) {
        if (j != i) {
            const float x = pos[3 * (int64_t)j] - pos[3 * i], y = pos[3 * (int64_t)j + 1] - pos[3 * i + 1],
                        z = pos[3 * (int64_t)j + 2] - pos[3 * i + 2];
            w = sqrtf(x * x + y * y + z * z);
            const float ux = x / w, uy = y / w, uz = z / w;
            const float s3 = 1.7320508075688772f;
            v[0] = ux; v[1] = uy; v[2] = uz;
            v[3] = s3 * ux * uz;
            v[4] = s3 * ux * uy;
            v[5] = uy * uy - 0.5f * (ux * ux + uz * uz);
            v[6] = s3 * uy * uz;
            v[7] = s3 / 2.f * (uz * uz - ux * ux);
        }
        c = w < cutoff ? 0.5f * (cosf(w * 3.14159265358979323846f / cutoff) + 1.f) : 0.f;
    }
    r_out[e] = w;
    cut_out[e] = c;
    const float alpha = 5.f / cutoff;
    const float ex = expf(alpha * (-w));
    for (int k = 0; k < NRBF; ++k) {
        const float t = ex - means[k];
        rbf[e * NRBF + k] = j >= 0 ? c * expf(-betas[k] * (t * t)) : 0.f;
    }
    for (int m = 0; m < NSH; ++m) sh[e * NSH + m] = v[m];
}

__global__ void __launch_bounds__(256)
k_vis_src_count(const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, const int32_t* __restrict__ batch,
                const int32_t* __restrict__ pool_rowptr, const int32_t* __restrict__ n_real, int64_t N,
                int32_t* __restrict__ src_cnt) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    if (j >= n_real_of(n_real, N)) { src_cnt[j] = 1; return; }
    const int b = batch[j];
    const int a0 = pool_rowptr[b], a1 = pool_rowptr[b + 1];
    int n = 0;
    for (int i = a0; i < a1; ++i) {
        const int c = cnt[i];
        for (int s = 0; s < c; ++s) n += slot[(int64_t)i * K + s] == j;
    }
    src_cnt[j] = n;
}

__global__ void __launch_bounds__(256)
k_vis_src_fill(const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, const int32_t* __restrict__ batch,
               const int32_t* __restrict__ pool_rowptr, const int32_t* __restrict__ n_real, int64_t N,
               const int32_t* __restrict__ src_cnt, int32_t* __restrict__ src_start, int32_t* __restrict__ src_eid) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    if (j >= n_real_of(n_real, N)) {
        src_start[j] = (int32_t)(j * K);
        src_eid[j * K] = (int32_t)(j * K);
        return;
    }
    const int b = batch[j];
    const int a0 = pool_rowptr[b], a1 = pool_rowptr[b + 1];
    int start = a0 * K;
    for (int q = a0; q < j; ++q) start += src_cnt[q];
    src_start[j] = start;
    int n = 0;
    for (int i = a0; i < a1; ++i) {
        const int c = cnt[i];
        for (int s = 0; s < c; ++s)
            if (slot[(int64_t)i * K + s] == j) src_eid[start + n++] = i * K + s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// neighbour embedding: y_i = sum_{j != i} x_j (W_e C(r_e));  W = distance_proj(rbf)
// ---------------------------------------------------------------------------------------------------------------------
#define VIS_ROWS(row, N) for (int64_t row = blockIdx.x; row < (N); row += gridDim.x)
#define VIS_LANE_CH(t, c, C)                                                  \
    _Pragma("unroll") for (int t = 0; t < MAXV; ++t)                          \
        if (const int c = threadIdx.x + LANES * t; c < (C))

__global__ void __launch_bounds__(LANES)
k_vis_nbr_fwd(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ cut,
              const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, int64_t N, int C,
              float* __restrict__ y) {
    VIS_ROWS(i, N) {
        float acc[MAXV] = {};
        const int n = cnt[i];
        for (int s = 0; s < n; ++s) {
            const int64_t e = i * K + s;
            const int64_t j = slot[e];
            if (j == i) continue;
            const float ce = cut[e];
            VIS_LANE_CH(t, c, C) acc[t] += x[j * C + c] * (W[e * C + c] * ce);
        }
        VIS_LANE_CH(t, c, C) y[i * C + c] = acc[t];
    }
}

__global__ void __launch_bounds__(LANES)
k_vis_nbr_bwd_edge(const float* __restrict__ x, const float* __restrict__ cut, const int32_t* __restrict__ slot,
                   const int32_t* __restrict__ cnt, const float* __restrict__ dy, int64_t N, int C,
                   float* __restrict__ dW) {
    VIS_ROWS(i, N) {
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            const int64_t j = s < n ? slot[e] : -1;
            const bool live = j >= 0 && j != i;
            const float ce = live ? cut[e] : 0.f;
            VIS_LANE_CH(t, c, C) dW[e * C + c] = live ? (dy[i * C + c] * x[j * C + c]) * ce : 0.f;
        }
    }
}

__global__ void __launch_bounds__(LANES)
k_vis_nbr_bwd_node(const float* __restrict__ W, const float* __restrict__ cut, const int32_t* __restrict__ src_start,
                   const int32_t* __restrict__ src_cnt, const int32_t* __restrict__ src_eid,
                   const float* __restrict__ dy, int64_t N, int C, float* __restrict__ dx) {
    VIS_ROWS(j, N) {
        float acc[MAXV] = {};
        const int q0 = src_start[j], q1 = q0 + src_cnt[j];
        for (int q = q0; q < q1; ++q) {
            const int64_t e = src_eid[q], i = e / K;
            if (i == j) continue;
            const float ce = cut[e];
            VIS_LANE_CH(t, c, C) acc[t] += dy[i * C + c] * (W[e * C + c] * ce);
        }
        VIS_LANE_CH(t, c, C) dx[j * C + c] = acc[t];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// edge embedding: f_e = (x_i + x_j) W_e;  W = edge_proj(rbf)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LANES)
k_vis_eemb_fwd(const float* __restrict__ x, const float* __restrict__ W, const int32_t* __restrict__ slot,
               const int32_t* __restrict__ cnt, int64_t N, int C, float* __restrict__ f) {
    VIS_ROWS(i, N) {
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            const int64_t j = s < n ? slot[e] : -1;
            VIS_LANE_CH(t, c, C) f[e * C + c] = j >= 0 ? (x[i * C + c] + x[j * C + c]) * W[e * C + c] : 0.f;
        }
    }
}

__global__ void __launch_bounds__(LANES)
k_vis_eemb_bwd_edge(const float* __restrict__ x, const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt,
                    const float* __restrict__ df, int64_t N, int C, float* __restrict__ dW) {
    VIS_ROWS(i, N) {
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            const int64_t j = s < n ? slot[e] : -1;
            VIS_LANE_CH(t, c, C) dW[e * C + c] = j >= 0 ? df[e * C + c] * (x[i * C + c] + x[j * C + c]) : 0.f;
        }
    }
}

// dx_n = sum over n's own slots (n as target) + sum over n's by-source edges (n as source)
__global__ void __launch_bounds__(LANES)
k_vis_eemb_bwd_node(const float* __restrict__ W, const int32_t* __restrict__ cnt, const int32_t* __restrict__ src_start,
                    const int32_t* __restrict__ src_cnt, const int32_t* __restrict__ src_eid,
                    const float* __restrict__ df, int64_t N, int C, float* __restrict__ dx) {
    VIS_ROWS(n, N) {
        float acc[MAXV] = {};
        const int m = cnt[n];
        for (int s = 0; s < m; ++s) {
            const int64_t e = n * K + s;
            VIS_LANE_CH(t, c, C) acc[t] += df[e * C + c] * W[e * C + c];
        }
        const int q0 = src_start[n], q1 = q0 + src_cnt[n];
        for (int q = q0; q < q1; ++q) {
            const int64_t e = src_eid[q];
            VIS_LANE_CH(t, c, C) acc[t] += df[e * C + c] * W[e * C + c];
        }
        VIS_LANE_CH(t, c, C) dx[n * C + c] = acc[t];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ViS_MP attention message: pre_{e,h} = sum_{c in h} q_i k_j silu(dkr_e);  a_{e,h} = silu(pre) C(r_e)
//   u_e = v_j silu(dvr_e) a_{e,h};  xagg_i = sum_e u_e
// ---------------------------------------------------------------------------------------------------------------------
// per-head sums of the lane products p[t] (LDS: s_p[C] + s_h[HEADS]); returns with s_h filled and visible
__device__ __forceinline__ void head_sums(const float (&p)[MAXV], int C, float* s_p, float* s_h) {
    VIS_LANE_CH(t, c, C) s_p[c] = p[t];
    __syncthreads();
    if (threadIdx.x < HEADS) {
        const int D = C / HEADS;
        float a = 0.f;
        for (int d = 0; d < D; ++d) a += s_p[threadIdx.x * D + d];
        s_h[threadIdx.x] = a;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(LANES)
k_vis_attn_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
               const float* __restrict__ dkr, const float* __restrict__ dvr, const float* __restrict__ cut,
               const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, int64_t N, int C,
               float* __restrict__ u, float* __restrict__ xagg, float* __restrict__ pre) {
    extern __shared__ float s_lds[];
    float* s_p = s_lds;
    float* s_h = s_lds + C;
    const int D = C / HEADS;
    VIS_ROWS(i, N) {
        float acc[MAXV] = {};
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            if (s >= n) {
                VIS_LANE_CH(t, c, C) u[e * C + c] = 0.f;
                if (threadIdx.x < HEADS) pre[e * HEADS + threadIdx.x] = 0.f;
                continue;
            }
            const int64_t j = slot[e];
            float p[MAXV] = {};
            VIS_LANE_CH(t, c, C) p[t] = (q[i * C + c] * k[j * C + c]) * silu_exact(dkr[e * C + c]);
            head_sums(p, C, s_p, s_h);
            const float ce = cut[e];
            if (threadIdx.x < HEADS) pre[e * HEADS + threadIdx.x] = s_h[threadIdx.x];
            VIS_LANE_CH(t, c, C) {
                const float a = silu_exact(s_h[c / D]) * ce;
                const float m = (v[j * C + c] * silu_exact(dvr[e * C + c])) * a;
                u[e * C + c] = m;
                acc[t] += m;
            }
            __syncthreads();
        }
        VIS_LANE_CH(t, c, C) xagg[i * C + c] = acc[t];
    }
}

// by target: g = du_e + dxagg_i; ddvr, dpre (-> LDS, stored), ddkr, dq_i
__global__ void __launch_bounds__(LANES)
k_vis_attn_bwd_edge(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                    const float* __restrict__ dkr, const float* __restrict__ dvr, const float* __restrict__ cut,
                    const float* __restrict__ pre, const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt,
                    const float* __restrict__ du, const float* __restrict__ dxagg, int64_t N, int C,
                    float* __restrict__ dq, float* __restrict__ ddkr, float* __restrict__ ddvr,
                    float* __restrict__ dpre) {
    extern __shared__ float s_lds[];
    float* s_p = s_lds;
    float* s_h = s_lds + C;
    const int D = C / HEADS;
    VIS_ROWS(i, N) {
        float acc[MAXV] = {};
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            if (s >= n) {
                VIS_LANE_CH(t, c, C) { ddkr[e * C + c] = 0.f; ddvr[e * C + c] = 0.f; }
                if (threadIdx.x < HEADS) dpre[e * HEADS + threadIdx.x] = 0.f;
                continue;
            }
            const int64_t j = slot[e];
            const float ce = cut[e];
            float p[MAXV] = {};
            VIS_LANE_CH(t, c, C) {
                const float g = du[e * C + c] + dxagg[i * C + c];
                const float dvv = dvr[e * C + c];
                const float ph = pre[e * HEADS + c / D];
                const float a = silu_exact(ph) * ce;
                ddvr[e * C + c] = ((g * a) * v[j * C + c]) * dsilu(dvv);
                p[t] = g * (v[j * C + c] * silu_exact(dvv));
            }
            head_sums(p, C, s_p, s_h);
            if (threadIdx.x < HEADS) {
                const float dp = (s_h[threadIdx.x] * ce) * dsilu(pre[e * HEADS + threadIdx.x]);
                dpre[e * HEADS + threadIdx.x] = dp;
                s_h[threadIdx.x] = dp;
            }
            __syncthreads();
            VIS_LANE_CH(t, c, C) {
                const float dp = s_h[c / D];
                const float dkk = dkr[e * C + c];
                ddkr[e * C + c] = ((dp * q[i * C + c]) * k[j * C + c]) * dsilu(dkk);
                acc[t] += (dp * k[j * C + c]) * silu_exact(dkk);
            }
            __syncthreads();
        }
        VIS_LANE_CH(t, c, C) dq[i * C + c] = acc[t];
    }
}

// by source: dk_j = sum dpre q_i silu(dkr_e);  dv_j = sum (du_e + dxagg_i) silu(dvr_e) a_{e,h}
__global__ void __launch_bounds__(LANES)
k_vis_attn_bwd_node(const float* __restrict__ q, const float* __restrict__ dkr, const float* __restrict__ dvr,
                    const float* __restrict__ cut, const float* __restrict__ pre, const float* __restrict__ dpre,
                    const int32_t* __restrict__ src_start, const int32_t* __restrict__ src_cnt,
                    const int32_t* __restrict__ src_eid, const float* __restrict__ du, const float* __restrict__ dxagg,
                    int64_t N, int C, float* __restrict__ dk, float* __restrict__ dv) {
    const int D = C / HEADS;
    VIS_ROWS(j, N) {
        float ak[MAXV] = {}, av[MAXV] = {};
        const int q0 = src_start[j], q1 = q0 + src_cnt[j];
        for (int qq = q0; qq < q1; ++qq) {
            const int64_t e = src_eid[qq], i = e / K;
            const float ce = cut[e];
            VIS_LANE_CH(t, c, C) {
                const int h = c / D;
                ak[t] += (dpre[e * HEADS + h] * q[i * C + c]) * silu_exact(dkr[e * C + c]);
                const float g = du[e * C + c] + dxagg[i * C + c];
                av[t] += (g * (silu_exact(pre[e * HEADS + h]) * ce)) * silu_exact(dvr[e * C + c]);
            }
        }
        VIS_LANE_CH(t, c, C) { dk[j * C + c] = ak[t]; dv[j * C + c] = av[t]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ViS_MP vector message: vo_i[m] = sum_e vec_j[m] s1_e + s2_e d_e[m];  (s1, s2) = silu(sr_e) split at C
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LANES)
k_vis_vec_fwd(const float* __restrict__ vec, const float* __restrict__ sr, const float* __restrict__ sh,
              const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, int64_t N, int C,
              float* __restrict__ vo) {
    VIS_ROWS(i, N) {
        float acc[NSH][MAXV] = {};
        const int n = cnt[i];
        for (int s = 0; s < n; ++s) {
            const int64_t e = i * K + s;
            const int64_t j = slot[e];
            float d[NSH];
            for (int m = 0; m < NSH; ++m) d[m] = sh[e * NSH + m];
            VIS_LANE_CH(t, c, C) {
                const float s1 = silu_exact(sr[e * 2 * C + c]), s2 = silu_exact(sr[e * 2 * C + C + c]);
#pragma unroll
                for (int m = 0; m < NSH; ++m) acc[m][t] += vec[(j * NSH + m) * C + c] * s1 + s2 * d[m];
            }
        }
        VIS_LANE_CH(t, c, C) {
#pragma unroll
            for (int m = 0; m < NSH; ++m) vo[(i * NSH + m) * C + c] = acc[m][t];
        }
    }
}

__global__ void __launch_bounds__(LANES)
k_vis_vec_bwd_edge(const float* __restrict__ vec, const float* __restrict__ sr, const float* __restrict__ sh,
                   const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt, const float* __restrict__ dvo,
                   int64_t N, int C, float* __restrict__ dsr) {
    VIS_ROWS(i, N) {
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            if (s >= n) {
                VIS_LANE_CH(t, c, C) { dsr[e * 2 * C + c] = 0.f; dsr[e * 2 * C + C + c] = 0.f; }
                continue;
            }
            const int64_t j = slot[e];
            float d[NSH];
            for (int m = 0; m < NSH; ++m) d[m] = sh[e * NSH + m];
            VIS_LANE_CH(t, c, C) {
                float a1 = 0.f, a2 = 0.f;
#pragma unroll
                for (int m = 0; m < NSH; ++m) {
                    const float g = dvo[(i * NSH + m) * C + c];
                    a1 += g * vec[(j * NSH + m) * C + c];
                    a2 += g * d[m];
                }
                dsr[e * 2 * C + c] = a1 * dsilu(sr[e * 2 * C + c]);
                dsr[e * 2 * C + C + c] = a2 * dsilu(sr[e * 2 * C + C + c]);
            }
        }
    }
}

__global__ void __launch_bounds__(LANES)
k_vis_vec_bwd_node(const float* __restrict__ sr, const int32_t* __restrict__ src_start,
                   const int32_t* __restrict__ src_cnt, const int32_t* __restrict__ src_eid,
                   const float* __restrict__ dvo, int64_t N, int C, float* __restrict__ dvec) {
    VIS_ROWS(j, N) {
        float acc[NSH][MAXV] = {};
        const int q0 = src_start[j], q1 = q0 + src_cnt[j];
        for (int qq = q0; qq < q1; ++qq) {
            const int64_t e = src_eid[qq], i = e / K;
            VIS_LANE_CH(t, c, C) {
                const float s1 = silu_exact(sr[e * 2 * C + c]);
#pragma unroll
                for (int m = 0; m < NSH; ++m) acc[m][t] += dvo[(i * NSH + m) * C + c] * s1;
            }
        }
        VIS_LANE_CH(t, c, C) {
#pragma unroll
            for (int m = 0; m < NSH; ++m) dvec[(j * NSH + m) * C + c] = acc[m][t];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ViS_MP edge update: df_e = silu(fr_e) sum_m a_m b_m,  a = rej(wt_i, d_e), b = rej(ws_j, -d_e),
//   rej(w, d) = w - (sum_m w_m d_m) d  (the 8 components as one 8-vector, vector_rejection)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rejection(const float (&w)[NSH], const float (&d)[NSH], float (&out)[NSH]) {
    float p = 0.f;
#pragma unroll
    for (int m = 0; m < NSH; ++m) p += w[m] * d[m];
#pragma unroll
    for (int m = 0; m < NSH; ++m) out[m] = w[m] - p * d[m];
}

__device__ __forceinline__ float edge_pair(const float* __restrict__ wt, const float* __restrict__ ws, int64_t i,
                                           int64_t j, int c, int C, const float (&d)[NSH], const float (&nd)[NSH],
                                           float (&a)[NSH], float (&b)[NSH]) {
    float w1[NSH], w2[NSH];
#pragma unroll
    for (int m = 0; m < NSH; ++m) {
        w1[m] = wt[(i * NSH + m) * C + c];
        w2[m] = ws[(j * NSH + m) * C + c];
    }
    rejection(w1, d, a);
    rejection(w2, nd, b);
    float dot = 0.f;
#pragma unroll
    for (int m = 0; m < NSH; ++m) dot += a[m] * b[m];
    return dot;
}

__global__ void __launch_bounds__(LANES)
k_vis_eupd_fwd(const float* __restrict__ wt, const float* __restrict__ ws, const float* __restrict__ fr,
               const float* __restrict__ sh, const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt,
               int64_t N, int C, float* __restrict__ df) {
    VIS_ROWS(i, N) {
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            if (s >= n) {
                VIS_LANE_CH(t, c, C) df[e * C + c] = 0.f;
                continue;
            }
            const int64_t j = slot[e];
            float d[NSH], nd[NSH];
            for (int m = 0; m < NSH; ++m) { d[m] = sh[e * NSH + m]; nd[m] = -d[m]; }
            VIS_LANE_CH(t, c, C) {
                float a[NSH], b[NSH];
                const float dot = edge_pair(wt, ws, i, j, c, C, d, nd, a, b);
                df[e * C + c] = silu_exact(fr[e * C + c]) * dot;
            }
        }
    }
}

// by target: dfr_e, dwt_i = sum_e J(d) (dwdot b)   (J(d) = I - d d^T)
__global__ void __launch_bounds__(LANES)
k_vis_eupd_bwd_edge(const float* __restrict__ wt, const float* __restrict__ ws, const float* __restrict__ fr,
                    const float* __restrict__ sh, const int32_t* __restrict__ slot, const int32_t* __restrict__ cnt,
                    const float* __restrict__ ddf, int64_t N, int C, float* __restrict__ dfr,
                    float* __restrict__ dwt) {
    VIS_ROWS(i, N) {
        float acc[NSH][MAXV] = {};
        const int n = cnt[i];
        for (int s = 0; s < K; ++s) {
            const int64_t e = i * K + s;
            if (s >= n) {
                VIS_LANE_CH(t, c, C) dfr[e * C + c] = 0.f;
                continue;
            }
            const int64_t j = slot[e];
            float d[NSH], nd[NSH];
            for (int m = 0; m < NSH; ++m) { d[m] = sh[e * NSH + m]; nd[m] = -d[m]; }
            VIS_LANE_CH(t, c, C) {
                float a[NSH], b[NSH], da[NSH], ja[NSH];
                const float dot = edge_pair(wt, ws, i, j, c, C, d, nd, a, b);
                const float g = ddf[e * C + c], f = fr[e * C + c];
                dfr[e * C + c] = (g * dot) * dsilu(f);
                const float gd = g * silu_exact(f);
#pragma unroll
                for (int m = 0; m < NSH; ++m) da[m] = gd * b[m];
                rejection(da, d, ja);
#pragma unroll
                for (int m = 0; m < NSH; ++m) acc[m][t] += ja[m];
            }
        }
        VIS_LANE_CH(t, c, C) {
#pragma unroll
            for (int m = 0; m < NSH; ++m) dwt[(i * NSH + m) * C + c] = acc[m][t];
        }
    }
}

// by source: dws_j = sum_e J(-d) (dwdot a)
__global__ void __launch_bounds__(LANES)
k_vis_eupd_bwd_node(const float* __restrict__ wt, const float* __restrict__ ws, const float* __restrict__ fr,
                    const float* __restrict__ sh, const int32_t* __restrict__ src_start,
                    const int32_t* __restrict__ src_cnt, const int32_t* __restrict__ src_eid,
                    const float* __restrict__ ddf, int64_t N, int C, float* __restrict__ dws) {
    VIS_ROWS(j, N) {
        float acc[NSH][MAXV] = {};
        const int q0 = src_start[j], q1 = q0 + src_cnt[j];
        for (int qq = q0; qq < q1; ++qq) {
            const int64_t e = src_eid[qq], i = e / K;
            float d[NSH], nd[NSH];
            for (int m = 0; m < NSH; ++m) { d[m] = sh[e * NSH + m]; nd[m] = -d[m]; }
            VIS_LANE_CH(t, c, C) {
                float a[NSH], b[NSH], db[NSH], jb[NSH];
                edge_pair(wt, ws, i, j, c, C, d, nd, a, b);
                const float gd = ddf[e * C + c] * silu_exact(fr[e * C + c]);
#pragma unroll
                for (int m = 0; m < NSH; ++m) db[m] = gd * a[m];
                rejection(db, nd, jb);
#pragma unroll
                for (int m = 0; m < NSH; ++m) acc[m][t] += jb[m];
            }
        }
        VIS_LANE_CH(t, c, C) {
#pragma unroll
            for (int m = 0; m < NSH; ++m) dws[(j * NSH + m) * C + c] = acc[m][t];
        }
    }
}

int check_c(int64_t N, int32_t C) {
    if (N < 0 || C <= 0 || C % HEADS || C > LANES * MAXV) return EQH_ERR_ARG;
    if (N * K >= INT32_MAX) return EQH_ERR_RANGE;
    return EQH_OK;
}

int row_grid(int64_t N) { return eqh_grid_for(N, 1, GRID_CAP); }

}  // namespace

extern "C" int vis_radius_graph(const float* pos, const int32_t* batch, const int32_t* pool_rowptr,
                                const int32_t* n_real, const float* means, const float* betas, int64_t N, float cutoff,
                                int32_t* slot, int32_t* cnt, float* r, float* cut, float* rbf, float* sh,
                                int32_t* src_start, int32_t* src_cnt, int32_t* src_eid, void* stream_) {
    if (N < 0 || !(cutoff > 0.f)) return EQH_ERR_ARG;
    if (N * K >= INT32_MAX) return EQH_ERR_RANGE;
    if (N == 0) return EQH_OK;
    if (!pos || !batch || !pool_rowptr || !means || !betas || !slot || !cnt || !r || !cut || !rbf || !sh ||
        !src_start || !src_cnt || !src_eid)
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int g = (int)((N + 255) / 256);
    const int64_t E = N * K;
    hipLaunchKernelGGL(k_vis_radius, dim3(g), dim3(256), 0, stream, pos, batch, pool_rowptr, n_real, N,
                       cutoff * cutoff, slot, cnt);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_geom, dim3((int)((E + 255) / 256)), dim3(256), 0, stream, pos, slot, means, betas, E, cutoff,
                       r, cut, rbf, sh);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_src_count, dim3(g), dim3(256), 0, stream, slot, cnt, batch, pool_rowptr, n_real, N, src_cnt);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_src_fill, dim3(g), dim3(256), 0, stream, slot, cnt, batch, pool_rowptr, n_real, N, src_cnt,
                       src_start, src_eid);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}




extern "C" int vis_nbr_fwd(const float* x, const float* W, const float* cut, const int32_t* slot, const int32_t* cnt, int64_t N, int32_t C,
                           float* y, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!x || !W || !cut || !slot || !cnt || !y) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_vis_nbr_fwd, dim3(row_grid(N)), dim3(LANES), 0, static_cast<hipStream_t>(stream_), x, W, cut,
                       slot, cnt, N, C, y);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_nbr_bwd(const float* x, const float* W, const float* cut, const int32_t* slot, const int32_t* cnt, const int32_t* src_start, const int32_t* src_cnt, const int32_t* src_eid,
                           const float* dy, int64_t N, int32_t C, float* dx, float* dW, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!x || !W || !cut || !slot || !cnt || !src_start || !src_cnt || !src_eid || !dy || !dx || !dW) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_vis_nbr_bwd_edge, dim3(row_grid(N)), dim3(LANES), 0, stream, x, cut, slot, cnt, dy, N, C, dW);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_nbr_bwd_node, dim3(row_grid(N)), dim3(LANES), 0, stream, W, cut, src_start, src_cnt,
                       src_eid, dy, N, C, dx);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_edge_embed_fwd(const float* x, const float* W, const int32_t* slot, const int32_t* cnt, int64_t N, int32_t C, float* f,
                                  void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!x || !W || !slot || !cnt || !f) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_vis_eemb_fwd, dim3(row_grid(N)), dim3(LANES), 0, static_cast<hipStream_t>(stream_), x, W,
                       slot, cnt, N, C, f);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_edge_embed_bwd(const float* x, const float* W, const int32_t* slot, const int32_t* cnt, const int32_t* src_start, const int32_t* src_cnt, const int32_t* src_eid, const float* df,
                                  int64_t N, int32_t C, float* dx, float* dW, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!x || !W || !slot || !cnt || !src_start || !src_cnt || !src_eid || !df || !dx || !dW) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_vis_eemb_bwd_edge, dim3(row_grid(N)), dim3(LANES), 0, stream, x, slot, cnt, df, N, C, dW);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_eemb_bwd_node, dim3(row_grid(N)), dim3(LANES), 0, stream, W, cnt, src_start, src_cnt,
                       src_eid, df, N, C, dx);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_attn_fwd(const float* q, const float* k, const float* v, const float* dkr, const float* dvr,
                            const float* cut, const int32_t* slot, const int32_t* cnt, int64_t N, int32_t C, float* u, float* xagg, float* pre,
                            void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!q || !k || !v || !dkr || !dvr || !cut || !slot || !cnt || !u || !xagg || !pre) return EQH_ERR_ARG;
    const size_t lds = (size_t)(C + HEADS) * sizeof(float);
    hipLaunchKernelGGL(k_vis_attn_fwd, dim3(row_grid(N)), dim3(LANES), lds, static_cast<hipStream_t>(stream_), q, k, v,
                       dkr, dvr, cut, slot, cnt, N, C, u, xagg, pre);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_attn_bwd(const float* q, const float* k, const float* v, const float* dkr, const float* dvr,
                            const float* cut, const float* pre, const int32_t* slot, const int32_t* cnt, const int32_t* src_start, const int32_t* src_cnt, const int32_t* src_eid, const float* du,
                            const float* dxagg, int64_t N, int32_t C, float* dq, float* dk, float* dv, float* ddkr,
                            float* ddvr, float* dpre, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!q || !k || !v || !dkr || !dvr || !cut || !pre || !slot || !cnt || !src_start || !src_cnt || !src_eid || !du ||
        !dxagg || !dq || !dk || !dv || !ddkr || !ddvr || !dpre)
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t lds = (size_t)(C + HEADS) * sizeof(float);
    hipLaunchKernelGGL(k_vis_attn_bwd_edge, dim3(row_grid(N)), dim3(LANES), lds, stream, q, k, v, dkr, dvr, cut, pre,
                       slot, cnt, du, dxagg, N, C, dq, ddkr, ddvr, dpre);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_attn_bwd_node, dim3(row_grid(N)), dim3(LANES), 0, stream, q, dkr, dvr, cut, pre, dpre,
                       src_start, src_cnt, src_eid, du, dxagg, N, C, dk, dv);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_vec_fwd(const float* vec, const float* sr, const float* sh, const int32_t* slot, const int32_t* cnt, int64_t N, int32_t C,
                           float* vo, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!vec || !sr || !sh || !slot || !cnt || !vo) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_vis_vec_fwd, dim3(row_grid(N)), dim3(LANES), 0, static_cast<hipStream_t>(stream_), vec, sr, sh,
                       slot, cnt, N, C, vo);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_vec_bwd(const float* vec, const float* sr, const float* sh, const int32_t* slot, const int32_t* cnt, const int32_t* src_start, const int32_t* src_cnt, const int32_t* src_eid,
                           const float* dvo, int64_t N, int32_t C, float* dvec, float* dsr, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!vec || !sr || !sh || !slot || !cnt || !src_start || !src_cnt || !src_eid || !dvo || !dvec || !dsr)
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_vis_vec_bwd_edge, dim3(row_grid(N)), dim3(LANES), 0, stream, vec, sr, sh, slot, cnt, dvo, N, C,
                       dsr);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_vec_bwd_node, dim3(row_grid(N)), dim3(LANES), 0, stream, sr, src_start, src_cnt, src_eid,
                       dvo, N, C, dvec);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_edge_update_fwd(const float* wt, const float* ws, const float* fr, const float* sh, const int32_t* slot, const int32_t* cnt,
                                   int64_t N, int32_t C, float* df, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!wt || !ws || !fr || !sh || !slot || !cnt || !df) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_vis_eupd_fwd, dim3(row_grid(N)), dim3(LANES), 0, static_cast<hipStream_t>(stream_), wt, ws, fr,
                       sh, slot, cnt, N, C, df);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int vis_edge_update_bwd(const float* wt, const float* ws, const float* fr, const float* sh, const int32_t* slot, const int32_t* cnt,
                                   const int32_t* src_start, const int32_t* src_cnt, const int32_t* src_eid, const float* ddf, int64_t N, int32_t C, float* dwt, float* dws,
                                   float* dfr, void* stream_) {
    int rc = check_c(N, C);
    if (rc || N == 0) return rc;
    if (!wt || !ws || !fr || !sh || !slot || !cnt || !src_start || !src_cnt || !src_eid || !ddf || !dwt || !dws || !dfr)
        return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_vis_eupd_bwd_edge, dim3(row_grid(N)), dim3(LANES), 0, stream, wt, ws, fr, sh, slot, cnt, ddf, N,
                       C, dfr, dwt);
    EQH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vis_eupd_bwd_node, dim3(row_grid(N)), dim3(LANES), 0, stream, wt, ws, fr, sh, src_start,
                       src_cnt, src_eid, ddf, N, C, dws);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}
