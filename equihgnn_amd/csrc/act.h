// Sigmoid and SiLU, defined ONCE per rounding.  The variants differ in their last bits and are not interchangeable: a
// kernel pair (forward / backward, fused / stand-alone) must use the same one.
#pragma once
#include "common.h"

namespace {

// 1 / (1 + e^-x) with libm's expf and an IEEE division
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// the same through v_exp_f32 / v_rcp_f32 (each ~1 ulp)
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float silu_fast(float x) { return x * sigmoid_fast(x); }

// GELU in its erf form (nn.GELU's default) and its derivative, with libm's erff / expf
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.7071067811865476f)) + x * (0.3989422804014327f * expf(-0.5f * x * x));
}

}  // namespace
