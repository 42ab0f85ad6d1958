// Optimiser-side helpers of the graphed training step (main.py:137-140: torch.optim.Adam(lr, weight_decay)).
//
// eqh_adam_step: Adam over ONE flat fp32 tensor (the trainer keeps all parameters in one buffer, their
//   gradients in another).  torch's fused multi-tensor Adam covers a single tensor with one 512-thread
//   block per 64 Ki elements -- 40 blocks for the 2.6 M parameters of egnn_equihnns, 46 us; an ordinary
//   grid-stride elementwise kernel needs 12.  Same arithmetic as torch.optim.Adam (amsgrad = False,
//   L2 weight decay folded into the gradient, bias corrections from a step counter), fp32 throughout.
//   The learning rate and the step counter live in device memory, so a captured hipGraph keeps working
//   when a scheduler changes the rate; the counter is advanced by the last workgroup to finish (a ticket
//   in the state block), after every workgroup has read it.
// eqh_grad_sumsq + eqh_adam_step_clip: the same update behind torch.nn.utils.clip_grad_norm_ (norm_type 2,
//   error_if_nonfinite False) of grad * grad_scale.  A first launch leaves one double partial of sum g^2 per workgroup;
//   the update (k_adam<true>) sums them in a fixed order in front of its bias corrections -- the kernel boundary is the
//   ordering between the two stages, no ticket, no fence, no atomics -- and folds min(1, max_norm / (norm + 1e-6)) into
//   the gradient scale.  Workgroup 0 keeps a 4-float readout {norm, coef, running max of norm, steps with coef < 1}.
// eqh_adam_step_ema / eqh_adam_step_clip_ema: the same launch keeping an exponential moving average of the parameters
//   (k_adam<CLIP, true>): the average is a fifth stream of the pass, requested with p, g, m, v, updated in registers from the
//   new p and stored with them -- e += (1 - d_t) (p - e), a copy at the first update; d_t from the step counter the kernel
//   reads anyway.  eqh_swap_f32 exchanges two flat buffers in place (live parameters <-> their average around an evaluation).
// eqh_copy_many: up to 64 small device-to-device copies in one launch (gradients that autograd allocated,
//   packed into the flat gradient buffer).
// eqh_add_many: the adding form, dst[i] += src[i] on k_copy_many's grid, for a step that accumulates the gradients of several
//   micro-batches; one more column of workgroups clears a second buffer, as k_adam does (the merged weights' scratch, which
//   no update clears between two micro-batches).
// eqh_mse_fwd_bwd / eqh_smooth_l1_fwd_bwd: a batch's loss and its gradient in one launch of one workgroup (k_mse; k_smooth_l1
//   for the l1 / smooth-l1 / Huber family of loss_family.h).
#include "common.h"
#include "loss_family.h"

namespace {

struct AdamState {       // device memory, 16 bytes, zero-initialised by the caller
    int64_t step;
    unsigned int ticket;
    unsigned int pad;
};

// The sum-of-squares pass: SQ_U quads per thread and trip, as k_adam's load (all loads of a trip requested before the
// first is used), at most SQ_GRID workgroups, g * g accumulated in double.  Every workgroup of the grid writes its slot,
// also one that found no element: the workspace is never cleared.
constexpr int SQ_U = 4;
constexpr int SQ_GRID = 256;
static inline int sumsq_grid(int64_t n) { return eqh_grid_for(n >> 2, 256 * SQ_U, SQ_GRID); }

__global__ void __launch_bounds__(256)
k_sumsq(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * SQ_U;
    double acc[SQ_U];
#pragma unroll
    for (int u = 0; u < SQ_U; ++u) acc[u] = 0.0;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x * SQ_U + threadIdx.x; i0 < n4; i0 += stride) {
        float4 gg[SQ_U];
#pragma unroll
        for (int u = 0; u < SQ_U; ++u) {
            const int64_t i = i0 + (int64_t)u * blockDim.x;
            gg[u] = i < n4 ? reinterpret_cast<const float4*>(g)[i] : f4_zero();
        }
#pragma unroll
        for (int u = 0; u < SQ_U; ++u) {
            const double x = gg[u].x, y = gg[u].y, z = gg[u].z, w = gg[u].w;
            acc[u] = fma(w, w, fma(z, z, fma(y, y, fma(x, x, acc[u]))));
        }
    }
    if (blockIdx.x == 0 && 4 * n4 + threadIdx.x < n) {  // ragged tail (n not a multiple of 4; all of it when n < 4)
        const double x = g[4 * n4 + threadIdx.x];
        acc[0] = fma(x, x, acc[0]);
    }
    // fixed order: the thread's accumulators as a tree, the wavefront by halving distances, the four wavefronts in turn
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int off = EQH_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
    __shared__ double s_wave[256 / EQH_WAVE];
    if ((threadIdx.x & (EQH_WAVE - 1)) == 0) s_wave[threadIdx.x / EQH_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// What stands where k_adam's `float gscale` stood: for CLIP = false that float alone (same size, same offset: the
// unclipped kernel keeps its argument block), for CLIP = true the clip's arguments behind it.
template <bool CLIP> struct ClipArgs { float gscale; };
template <> struct ClipArgs<true> {
    float gscale;
    float max_norm;
    const double* partials;   // n_partials doubles of k_sumsq
    float* readout;           // {norm before clipping, coef, running max of norm, steps with coef < 1}
    int n_partials;
};

// What stands where k_adam's `int64_t zero_also_n` stood, at the end of the argument block: for EMA = false that count alone
// (the kernels without an average keep their argument blocks), for EMA = true the average's arguments behind it.
template <bool EMA> struct EmaArgs { int64_t zero_also_n; };
template <> struct EmaArgs<true> {
    int64_t zero_also_n;
    float* ema;               // n floats beside p: the moving average, updated in place
    float decay;              // d in [0, 1)
    int warmup;               // != 0: d_t = min(d, (1 + t) / (10 + t))
};

template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256)
k_adam(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
       const float* __restrict__ lr_ptr, float beta1, float beta2, float eps, float wd, ClipArgs<CLIP> ca,
       AdamState* __restrict__ st, int zero_grad, float* __restrict__ zero_also, EmaArgs<EMA> ea) {
    const int64_t zero_also_n = ea.zero_also_n;
    // AD_U quads per thread and pass, all sixteen 16-byte loads of a pass requested before anything else -- before the bias
    // corrections are worked out, too (the step counter's load, two powf and a barrier otherwise sit in front of every memory
    // request).  Round 6: one quad per thread on 1340 workgroups moved 44 MB in 23 us (1.9 TB/s, four loads in flight per
    // thread and 1340 tickets on one address); a quarter of the workgroups with four times the bytes in flight each.
    constexpr int AD_U = 4;
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * AD_U;
    int64_t i0 = (int64_t)blockIdx.x * blockDim.x * AD_U + threadIdx.x;
    float4 pp[AD_U], gg[AD_U], mm[AD_U], vv[AD_U];
    float4 ee[EMA ? AD_U : 1];   // EMA: a fifth stream, the average (twenty loads of a pass in flight)
    float* __restrict__ e = nullptr;
    if constexpr (EMA) e = ea.ema;
    auto load = [&](int64_t base) {
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const int64_t i = base + (int64_t)u * blockDim.x;
            if (i < n4) {
                pp[u] = reinterpret_cast<float4*>(p)[i];
                gg[u] = reinterpret_cast<const float4*>(g)[i];
                mm[u] = reinterpret_cast<float4*>(m)[i];
                vv[u] = reinterpret_cast<float4*>(v)[i];
                if constexpr (EMA) ee[u] = reinterpret_cast<float4*>(e)[i];
            }
        }
    };
    load(i0);
    // the bias corrections once per workgroup (two powf per THREAD were most of the kernel's instructions)
    constexpr int EMA_AT = CLIP ? 3 : 2;
    __shared__ float s_corr[EMA_AT + (EMA ? 2 : 0)];
    if (threadIdx.x == 0) {
        const float t = (float)(st->step + 1);
        s_corr[0] = *lr_ptr / (1.0f - powf(beta1, t));
        s_corr[1] = sqrtf(1.0f - powf(beta2, t));
        if constexpr (EMA) {
            // the average's weight 1 - d_t of update t = step + 1, formed in double and rounded once; t == 1 copies
            const int64_t ti = st->step + 1;
            double d = (double)ea.decay;
            if (ea.warmup) {
                const double dw = (double)(1 + ti) / (double)(10 + ti);
                d = dw < d ? dw : d;
            }
            s_corr[EMA_AT] = (float)(1.0 - d);
            s_corr[EMA_AT + 1] = ti == 1 ? 1.0f : 0.0f;
        }
    }
    if constexpr (CLIP) {
        // the second stage of the norm, by the first wavefront of EVERY workgroup in one fixed order (so all of them scale
        // by the same bits): lane l sums partials l, l + 64, ..., then the lanes by halving distances
        if (threadIdx.x < EQH_WAVE) {
            double s = 0.0;
            for (int k = threadIdx.x; k < ca.n_partials; k += EQH_WAVE) s += ca.partials[k];
#pragma unroll
            for (int off = EQH_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (threadIdx.x == 0) {
                // clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1); a NaN coef stays NaN, as torch.clamp keeps it
                const float total_norm = (float)(sqrt(s) * (double)ca.gscale);
                float coef = ca.max_norm / (total_norm + 1e-6f);
                coef = coef > 1.0f ? 1.0f : coef;
                s_corr[2] = ca.gscale * coef;
                if (blockIdx.x == 0) {
                    float* r = ca.readout;
                    const float seen = r[2], clipped = r[3];
                    r[0] = total_norm;
                    r[1] = coef;
                    r[2] = total_norm > seen ? total_norm : seen;
                    r[3] = coef < 1.0f ? clipped + 1.0f : clipped;
                }
            }
        }
    }
    __syncthreads();
    const float step_size = s_corr[0];
    const float bc2_sqrt = s_corr[1];
    float gscale = ca.gscale;
    if constexpr (CLIP) gscale = s_corr[2];
    float ema_w = 0.f;
    bool ema_first = false;
    if constexpr (EMA) {
        ema_w = s_corr[EMA_AT];
        ema_first = s_corr[EMA_AT + 1] != 0.f;
    }
    for (; i0 < n4; i0 += stride) {
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const int64_t i = i0 + (int64_t)u * blockDim.x;
            if (i >= n4) continue;
            float* pe = &pp[u].x; float* ge = &gg[u].x; float* me = &mm[u].x; float* ve = &vv[u].x;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float gr = ge[c] * gscale;
                if (wd != 0.f) gr = fmaf(wd, pe[c], gr);
                me[c] = beta1 * me[c] + (1.0f - beta1) * gr;
                ve[c] = beta2 * ve[c] + (1.0f - beta2) * gr * gr;
                const float denom = sqrtf(ve[c]) / bc2_sqrt + eps;
                pe[c] -= step_size * (me[c] / denom);
                if constexpr (EMA) {    // from the NEW p: subtract, scale, add (three roundings); the first update is a copy
                    float* ae = &ee[u].x;
                    ae[c] = ema_first ? pe[c] : ae[c] + ema_w * (pe[c] - ae[c]);
                }
            }
            reinterpret_cast<float4*>(p)[i] = pp[u];
            reinterpret_cast<float4*>(m)[i] = mm[u];
            reinterpret_cast<float4*>(v)[i] = vv[u];
            if constexpr (EMA) reinterpret_cast<float4*>(e)[i] = ee[u];
            if (zero_grad) reinterpret_cast<float4*>(g)[i] = f4_zero();   // the next step's kernels accumulate into zeros
        }
        if (i0 + stride < n4) load(i0 + stride);
    }
    // a second buffer cleared on the way (accumulators that are not parameter gradients: the merged weights' scratch)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (zero_also_n >> 2); i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(zero_also)[i] = f4_zero();
    if (blockIdx.x == 0) {  // ragged tail (n not a multiple of 4)
        for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
            float gr = g[i] * gscale;
            if (wd != 0.f) gr = fmaf(wd, p[i], gr);
            const float mi = beta1 * m[i] + (1.0f - beta1) * gr;
            const float vi = beta2 * v[i] + (1.0f - beta2) * gr * gr;
            m[i] = mi;
            v[i] = vi;
            const float pi = p[i] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
            p[i] = pi;
            if constexpr (EMA) e[i] = ema_first ? pi : e[i] + ema_w * (pi - e[i]);
            if (zero_grad) g[i] = 0.f;
        }
    }
    // the last workgroup to finish advances the step counter: every workgroup read it before finishing
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int ticket = atomicAdd(&st->ticket, 1u);
        if (ticket == gridDim.x - 1) {
            st->step += 1;
            st->ticket = 0;
        }
    }
}

// eqh_swap_f32: SW_U quads of each buffer per thread and trip, all loads of a trip requested before the first store; at most
// SWAP_GRID workgroups, workgroup 0 takes the ragged tail.  The two buffers do not overlap (checked on the host).
constexpr int SW_U = 4;
constexpr int SWAP_GRID = 2048;

__global__ void __launch_bounds__(256) k_swap(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * SW_U;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x * SW_U + threadIdx.x; i0 < n4; i0 += stride) {
        float4 aa[SW_U], bb[SW_U];
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const int64_t i = i0 + (int64_t)u * blockDim.x;
            aa[u] = i < n4 ? reinterpret_cast<const float4*>(a)[i] : f4_zero();
            bb[u] = i < n4 ? reinterpret_cast<const float4*>(b)[i] : f4_zero();
        }
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const int64_t i = i0 + (int64_t)u * blockDim.x;
            if (i < n4) {
                reinterpret_cast<float4*>(a)[i] = bb[u];
                reinterpret_cast<float4*>(b)[i] = aa[u];
            }
        }
    }
    if (blockIdx.x == 0) {  // ragged tail (n not a multiple of 4)
        for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
            const float x = a[i];
            a[i] = b[i];
            b[i] = x;
        }
    }
}

constexpr int COPY_MAX = 64;
struct CopyBatch {
    const float* src[COPY_MAX];
    float* dst[COPY_MAX];
    int n[COPY_MAX];
};

__global__ void __launch_bounds__(256) k_copy_many(CopyBatch b) {
    const float* __restrict__ s = b.src[blockIdx.x];
    float* __restrict__ d = b.dst[blockIdx.x];
    const int n = b.n[blockIdx.x];
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {  // float4 body, scalar tail
        const int n4 = n >> 2;
        for (int i = blockIdx.y * 256 + threadIdx.x; i < n4; i += gridDim.y * 256)
            reinterpret_cast<float4*>(d)[i] = reinterpret_cast<const float4*>(s)[i];
        if (blockIdx.y == 0)
            for (int i = 4 * n4 + threadIdx.x; i < n; i += 256) d[i] = s[i];
    } else {
        for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) d[i] = s[i];
    }
}

__global__ void __launch_bounds__(1024)
k_mse(const float* __restrict__ pred, const float* __restrict__ target, int n, float* __restrict__ loss,
      float* __restrict__ grad) {
    __shared__ float s_sum[1024];
    const float inv_n = 1.0f / (float)n;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) {   // fixed assignment and tree: reproducible
        const float d = pred[i] - target[i];
        acc = fmaf(d, d, acc);
        grad[i] = 2.0f * d * inv_n;
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = s_sum[0] * inv_n;
}

// k_mse for the family of loss_family.h: the same element-to-thread assignment and the same tree.  The gradient is
// slope / n by a division, so the linear branch gives the correctly rounded +-scale / n.
__global__ void __launch_bounds__(1024)
k_smooth_l1(const float* __restrict__ pred, const float* __restrict__ target, int n, float beta, float scale,
            float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ float s_sum[1024];
    const float fn = (float)n;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) {   // fixed assignment and tree: reproducible
        float term, slope;
        sl1_term_slope(pred[i] - target[i], beta, scale, term, slope);
        acc += term;
        grad[i] = slope / fn;
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = s_sum[0] / fn;
}

}  // namespace

extern "C" int eqh_mse_fwd_bwd(const float* pred, const float* target, int32_t n, float* loss, float* grad,
                               void* stream_) {
    if (n <= 0 || n > 65536 || !pred || !target || !loss || !grad) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_mse, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_), pred, target, (int)n, loss, grad);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_smooth_l1_fwd_bwd(const float* pred, const float* target, int32_t n, float beta, float scale, float* loss,
                                     float* grad, void* stream_) {
    if (n <= 0 || n > 65536 || !pred || !target || !loss || !grad || !sl1_args_ok(beta, scale)) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_smooth_l1, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_), pred, target, (int)n, beta, scale,
                       loss, grad);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

// eqh_adam_step (CLIP = false) and eqh_adam_step_clip (CLIP = true), each with its _ema twin (EMA = true): one set of
// argument checks, one launch
template <bool CLIP, bool EMA>
static int adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr, float beta1,
                     float beta2, float eps, float weight_decay, ClipArgs<CLIP> ca, void* state, int32_t zero_grad,
                     float* zero_also, EmaArgs<EMA> ea, void* stream_) {
    const int64_t zero_also_n = ea.zero_also_n;
    if (n < 0 || !lr || !state) return EQH_ERR_ARG;
    if constexpr (CLIP) {
        if (!ca.partials || !ca.readout || !(ca.max_norm > 0.f)) return EQH_ERR_ARG;
    }
    if constexpr (EMA) {
        if (!(ea.decay >= 0.f && ea.decay < 1.f)) return EQH_ERR_ARG;     // (a NaN decay fails both comparisons)
    }
    if (n == 0) return EQH_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return EQH_ERR_ARG;
    if constexpr (EMA) {
        if (!ea.ema) return EQH_ERR_ARG;
    }
    if (zero_also_n < 0 || (zero_also_n > 0 && !zero_also) || (zero_also_n & 3) || !eqh_aligned16(zero_also)) return EQH_ERR_ARG;
    if (!eqh_aligned16(param) || !eqh_aligned16(grad) || !eqh_aligned16(exp_avg) || !eqh_aligned16(exp_avg_sq) ||
        ((uintptr_t)state & 7))
        return EQH_ERR_ALIGN;
    if constexpr (CLIP) {
        if (((uintptr_t)ca.partials & 7) || !eqh_aligned16(ca.readout)) return EQH_ERR_ALIGN;
    }
    if constexpr (EMA) {
        if (!eqh_aligned16(ea.ema)) return EQH_ERR_ALIGN;
    }
    hipLaunchKernelGGL((k_adam<CLIP, EMA>), dim3(eqh_grid_for(n / 16 + 1, 256, 2048)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                       ca, static_cast<AdamState*>(state), (int)zero_grad, zero_also, ea);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             const float* lr, float beta1, float beta2, float eps, float weight_decay,
                             float grad_scale, void* state, int32_t zero_grad, float* zero_also, int64_t zero_also_n,
                             void* stream_) {
    return adam_step<false, false>(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                                   ClipArgs<false>{grad_scale}, state, zero_grad, zero_also, EmaArgs<false>{zero_also_n}, stream_);
}

extern "C" int eqh_adam_step_ema(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 const float* lr, float beta1, float beta2, float eps, float weight_decay,
                                 float grad_scale, void* state, int32_t zero_grad, float* zero_also, int64_t zero_also_n,
                                 float* ema, float decay, int32_t warmup, void* stream_) {
    return adam_step<false, true>(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                                  ClipArgs<false>{grad_scale}, state, zero_grad, zero_also,
                                  EmaArgs<true>{zero_also_n, ema, decay, (int)warmup}, stream_);
}

extern "C" size_t eqh_grad_sumsq_workspace_bytes(int64_t n) {
    return n < 0 ? 0 : (size_t)sumsq_grid(n) * sizeof(double);
}

extern "C" int eqh_grad_sumsq(const float* grad, int64_t n, void* partials, void* stream_) {
    if (n < 0 || !partials || (n > 0 && !grad)) return EQH_ERR_ARG;
    if (!eqh_aligned16(grad) || ((uintptr_t)partials & 7)) return EQH_ERR_ALIGN;
    hipLaunchKernelGGL(k_sumsq, dim3(sumsq_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream_), grad, n,
                       static_cast<double*>(partials));
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_adam_step_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  const float* lr, float beta1, float beta2, float eps, float weight_decay,
                                  float grad_scale, void* state, int32_t zero_grad, float* zero_also,
                                  int64_t zero_also_n, const void* partials, float max_norm, float* readout,
                                  void* stream_) {
    return adam_step<true, false>(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                                  ClipArgs<true>{grad_scale, max_norm, static_cast<const double*>(partials), readout, sumsq_grid(n)},
                                  state, zero_grad, zero_also, EmaArgs<false>{zero_also_n}, stream_);
}

extern "C" int eqh_adam_step_clip_ema(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                      const float* lr, float beta1, float beta2, float eps, float weight_decay,
                                      float grad_scale, void* state, int32_t zero_grad, float* zero_also,
                                      int64_t zero_also_n, const void* partials, float max_norm, float* readout,
                                      float* ema, float decay, int32_t warmup, void* stream_) {
    return adam_step<true, true>(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                                 ClipArgs<true>{grad_scale, max_norm, static_cast<const double*>(partials), readout, sumsq_grid(n)},
                                 state, zero_grad, zero_also, EmaArgs<true>{zero_also_n, ema, decay, (int)warmup}, stream_);
}

// The in-place exchange of two buffers that do not overlap (the live parameters and their average, around an evaluation)
extern "C" int eqh_swap_f32(float* a, float* b, int64_t n, void* stream_) {
    if (n < 0) return EQH_ERR_ARG;
    if (n == 0) return EQH_OK;
    if (!a || !b) return EQH_ERR_ARG;
    const uintptr_t lo = (uintptr_t)(a < b ? a : b), hi = (uintptr_t)(a < b ? b : a);
    if ((hi - lo) / sizeof(float) < (uint64_t)n) return EQH_ERR_ARG;      // the same buffer, or two that overlap
    if (!eqh_aligned16(a) || !eqh_aligned16(b)) return EQH_ERR_ALIGN;
    hipLaunchKernelGGL(k_swap, dim3(eqh_grid_for(n / 16 + 1, 256, SWAP_GRID)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       a, b, n);
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_copy_many(int32_t count, const float* const* src, float* const* dst, const int64_t* n,
                             void* stream_) {
    if (count < 0 || (count > 0 && (!src || !dst || !n))) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int i0 = 0; i0 < count; i0 += COPY_MAX) {
        CopyBatch b;
        const int m = (count - i0 < COPY_MAX) ? count - i0 : COPY_MAX;
        int64_t most = 0;
        for (int i = 0; i < m; ++i) {
            if (n[i0 + i] < 0 || n[i0 + i] >= ((int64_t)1 << 31) || (n[i0 + i] > 0 && (!src[i0 + i] || !dst[i0 + i])))
                return EQH_ERR_ARG;
            b.src[i] = src[i0 + i];
            b.dst[i] = dst[i0 + i];
            b.n[i] = (int)n[i0 + i];
            if (n[i0 + i] > most) most = n[i0 + i];
        }
        if (most == 0) continue;
        const int by = (int)((most + 4095) / 4096 < 256 ? (most + 4095) / 4096 : 256);  // 16 floats per thread and pass
        hipLaunchKernelGGL(k_copy_many, dim3(m, by), dim3(256), 0, stream, b);
        EQH_CHECK_LAUNCH();
    }
    return EQH_OK;
}

namespace {

// k_copy_many's adding twin: workgroup column e < b.count adds entry e, column b.count clears zero_also (zero_n floats, a
// multiple of 4, 16-byte aligned: checked on the host).  64-bit trip variables: an entry may hold up to 2^31 - 1 floats.
struct AddBatch {
    const float* src[COPY_MAX];
    float* dst[COPY_MAX];
    int n[COPY_MAX];
    int count;
    float* zero_also;
    int64_t zero_n;
};

__global__ void __launch_bounds__(256) k_add_many(AddBatch b) {
    const int64_t first = (int64_t)blockIdx.y * 256 + threadIdx.x, stride = (int64_t)gridDim.y * 256;
    if ((int)blockIdx.x >= b.count) {
        for (int64_t i = first; i < (b.zero_n >> 2); i += stride) reinterpret_cast<float4*>(b.zero_also)[i] = f4_zero();
        return;
    }
    const float* __restrict__ s = b.src[blockIdx.x];
    float* __restrict__ d = b.dst[blockIdx.x];
    const int64_t n = b.n[blockIdx.x];
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {  // float4 body, scalar tail
        const int64_t n4 = n >> 2;
        for (int64_t i = first; i < n4; i += stride) {
            const float4 x = reinterpret_cast<const float4*>(s)[i];
            float4 y = reinterpret_cast<float4*>(d)[i];
            y.x += x.x; y.y += x.y; y.z += x.z; y.w += x.w;
            reinterpret_cast<float4*>(d)[i] = y;
        }
        if (blockIdx.y == 0)
            for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += 256) d[i] += s[i];
    } else {
        for (int64_t i = first; i < n; i += stride) d[i] += s[i];
    }
}

}  // namespace

// The adding form of eqh_copy_many, with k_adam's second job: the first launch also clears zero_also.  Every argument is
// checked before the first launch.
extern "C" int eqh_add_many(int32_t count, const float* const* src, float* const* dst, const int64_t* n,
                            float* zero_also, int64_t zero_also_n, void* stream_) {
    if (count < 0 || (count > 0 && (!src || !dst || !n))) return EQH_ERR_ARG;
    if (zero_also_n < 0 || (zero_also_n & 3) || (zero_also_n > 0 && !zero_also) || !eqh_aligned16(zero_also)) return EQH_ERR_ARG;
    for (int i = 0; i < count; ++i)
        if (n[i] < 0 || n[i] >= ((int64_t)1 << 31) || (n[i] > 0 && (!src[i] || !dst[i]))) return EQH_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int64_t zero_n = zero_also_n;
    for (int i0 = 0; i0 < count || zero_n > 0; i0 += COPY_MAX) {
        AddBatch b;
        const int m = (count - i0 < COPY_MAX) ? (count - i0 > 0 ? count - i0 : 0) : COPY_MAX;
        int64_t most = zero_n;
        for (int i = 0; i < m; ++i) {
            b.src[i] = src[i0 + i];
            b.dst[i] = dst[i0 + i];
            b.n[i] = (int)n[i0 + i];
            if (n[i0 + i] > most) most = n[i0 + i];
        }
        b.count = m;
        b.zero_also = zero_also;
        b.zero_n = zero_n;
        const bool clear = zero_n > 0;
        zero_n = 0;
        if (most == 0) continue;
        const int by = (int)((most + 4095) / 4096 < 256 ? (most + 4095) / 4096 : 256);  // 16 floats per thread and pass
        hipLaunchKernelGGL(k_add_many, dim3(m + (clear ? 1 : 0), by), dim3(256), 0, stream, b);
        EQH_CHECK_LAUNCH();
    }
    return EQH_OK;
}
