// The regression losses beside the MSE ("l1", "smooth_l1", "huber" of ops.loss_spec) as ONE parametrised form.  With
// d = pred - target and a = |d|:
//
//   term(d)  = scale * (a < beta ? 0.5 d^2 / beta : a - 0.5 beta)
//   slope(d) = scale * (a < beta ? d / beta       : sign(d)),   sign(0) = 0
//
//   l1          beta = 0, scale = 1: a < 0 never holds, so the quadratic branch (and its division) is never taken
//   smooth_l1   scale = 1: F.smooth_l1_loss(beta = beta); beta = 0 is l1, as in torch
//   huber       beta = scale = delta: F.huber_loss(delta = delta) = delta * smooth_l1(beta = delta)
//
// In the linear branch the slope is +-scale exactly, so a kernel's gradient there is the correctly rounded +-scale / n.
// Used by k_smooth_l1 (optim.hip) and by the SL1 forms of the two read-out heads (readout_head.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

__device__ __forceinline__ void sl1_term_slope(float d, float beta, float scale, float& term, float& slope) {
    const float a = fabsf(d);
    if (a < beta) {
        const float q = d / beta;
        term = scale * (0.5f * d * q);
        slope = scale * q;
    } else {
        term = scale * (a - 0.5f * beta);
        slope = d > 0.f ? scale : (d < 0.f ? -scale : d);     // (d: 0 at d == 0, and a NaN stays one)
    }
}

// what the five entries ask of the two floats: finite, beta >= 0, scale > 0 (a NaN fails the comparisons)
inline bool sl1_args_ok(float beta, float scale) { return beta >= 0.f && scale > 0.f && std::isfinite(beta) && std::isfinite(scale); }
