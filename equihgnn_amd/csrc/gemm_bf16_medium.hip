// The k_gemm_x6 kernels of matmul precision "medium" (1 bf16 plane per operand, one product per fp32 product) and their launch
// function gx_launch_planes1: gemm_x6.hip compiled with GX_PLANES = 1, a translation unit of its own so that the three modes'
// instantiations build side by side.
#define GX_PLANES 1
#include "gemm_x6.hip"
