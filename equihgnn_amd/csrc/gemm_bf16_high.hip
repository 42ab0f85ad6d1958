// The k_gemm_x6 kernels of matmul precision "high" (2 bf16 planes per operand, three products per fp32 product) and their launch
// function gx_launch_planes2: gemm_x6.hip compiled with GX_PLANES = 2, a translation unit of its own so that the three modes'
// instantiations build side by side.
#define GX_PLANES 2
#include "gemm_x6.hip"
