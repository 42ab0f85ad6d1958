// An epoch's loss and bootstrap metrics kept on the device (main.py:37-42,65-76,90-110: torchmetrics BootStrapper(
// MeanAbsoluteError / MeanSquaredError, num_bootstraps = 50) and the per-epoch mean of the training loss).
//
// eqh_bootstrap_update: one validation / test batch into the running sums of every bootstrap copy.  One workgroup per
//   copy; the copy's Poisson(1) weight of element i is poisson1(seed, position0 + i, copy) (poisson_hash.h), recomputed
//   here instead of read from a [copies, n] matrix drawn on the host.  Sums in double, reduced in a fixed order -- the
//   thread's accumulators, the wavefront by halving distances, the four wavefronts in turn (k_sumsq's scheme, optim.hip)
//   -- and added to the copy's three slots by thread 0: one writer per slot, no atomics, bitwise reproducible.
// eqh_loss_accumulate: {sum, count} of the training step's loss scalars, one thread.
// eqh_bootstrap_weights_host: the weights themselves, on the host (tests, and whoever wants to redo a resample).
#include "common.h"
#include "poisson_hash.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_SLOTS = 64;     // row length of acc: [3, 64] doubles

__global__ void __launch_bounds__(BS_THREADS)
k_bootstrap_update(const float* __restrict__ pred, const float* __restrict__ target, int64_t n, float scale, uint64_t seed,
                   uint64_t position0, double* __restrict__ acc) {
    const uint32_t copy = blockIdx.x;
    double s_abs = 0.0, s_sq = 0.0, s_w = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += BS_THREADS) {
        const uint32_t w = poisson1(seed, position0 + (uint64_t)i, copy);
        if (w == 0u) continue;          // an element this copy did not draw contributes nothing, whatever its value (NaN)
        // the fp32 products first: the arithmetic of metrics.update(out * scale, y * scale)
        const double e = (double)(pred[i] * scale) - (double)(target[i] * scale);
        const double wd = (double)w;
        s_abs += wd * fabs(e);
        s_sq += wd * (e * e);
        s_w += wd;
    }
#pragma unroll
    for (int off = EQH_WAVE / 2; off > 0; off >>= 1) {
        s_abs += __shfl_down(s_abs, off);
        s_sq += __shfl_down(s_sq, off);
        s_w += __shfl_down(s_w, off);
    }
    __shared__ double s_wave[3][BS_THREADS / EQH_WAVE];
    if ((threadIdx.x & (EQH_WAVE - 1)) == 0) {
        const int wv = threadIdx.x / EQH_WAVE;
        s_wave[0][wv] = s_abs;
        s_wave[1][wv] = s_sq;
        s_wave[2][wv] = s_w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            acc[r * BS_SLOTS + copy] += (s_wave[r][0] + s_wave[r][1]) + (s_wave[r][2] + s_wave[r][3]);
    }
}

__global__ void k_loss_accumulate(const float* __restrict__ loss, double* __restrict__ acc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        acc[0] += (double)loss[0];
        acc[1] += 1.0;
    }
}

}  // namespace

extern "C" int eqh_bootstrap_update(const float* pred, const float* target, int64_t n, float scale, int32_t copies,
                                    int64_t seed, int64_t position0, void* acc, void* stream_) {
    if (!acc || n < 0 || copies < 1 || copies > BS_SLOTS || position0 < 0) return EQH_ERR_ARG;
    if ((uintptr_t)acc & 7) return EQH_ERR_ALIGN;
    if (n == 0) return EQH_OK;
    if (!pred || !target) return EQH_ERR_ARG;
    hipLaunchKernelGGL(k_bootstrap_update, dim3(copies), dim3(BS_THREADS), 0, static_cast<hipStream_t>(stream_), pred, target,
                       n, scale, (uint64_t)seed, (uint64_t)position0, static_cast<double*>(acc));
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_loss_accumulate(const float* loss, void* acc, void* stream_) {
    if (!loss || !acc) return EQH_ERR_ARG;
    if ((uintptr_t)acc & 7) return EQH_ERR_ALIGN;
    hipLaunchKernelGGL(k_loss_accumulate, dim3(1), dim3(EQH_WAVE), 0, static_cast<hipStream_t>(stream_), loss,
                       static_cast<double*>(acc));
    EQH_CHECK_LAUNCH();
    return EQH_OK;
}

extern "C" int eqh_bootstrap_weights_host(int64_t seed, int64_t position0, int64_t n, int32_t copies, int32_t* out) {
    if (n < 0 || copies < 1 || copies > BS_SLOTS || position0 < 0 || (n > 0 && !out)) return EQH_ERR_ARG;
    for (int32_t c = 0; c < copies; ++c)
        for (int64_t i = 0; i < n; ++i)
            out[(int64_t)c * n + i] = (int32_t)poisson1((uint64_t)seed, (uint64_t)position0 + (uint64_t)i, (uint32_t)c);
    return EQH_OK;
}
