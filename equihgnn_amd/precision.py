"""The matmul precision mode: torch.set_float32_matmul_precision's three words for this package's dense products.

"highest" (the default): six bf16 products per fp32 product, fp32-grade results -- what every parity test pins.  "high": three
products (two bf16 planes per operand, TF32 grade: every dropped term below 2^-14 |a||b|).  "medium": one product (one plane, bf16
grade: operands truncated to 8 significand bits).  A permission, not an obligation: products that do not go to the x6 GEMM kernel
(the fp32 library below its threshold, the panel kernels, the EGNN edge kernel, the batched weight gradients) stay at fp32 grade.
ops.products reads the mode at call time; a captured step replays the mode it was captured under (trainer keys its graphs by it).
"""
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}     # mode -> `products` of hg_gemm_bf16_batch
_mode = "highest"


def set_float32_matmul_precision(mode: str) -> None:
    global _mode
    if mode not in PRODUCTS:
        raise ValueError(f"matmul precision must be one of {tuple(PRODUCTS)}, not {mode!r}")
    _mode = mode


def get_float32_matmul_precision() -> str:
    return _mode


def products() -> int:
    """Partial products per fp32 product under the current mode (6, 3 or 1)."""
    return PRODUCTS[_mode]
