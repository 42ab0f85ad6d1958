"""The matmul precision mode: torch.set_float32_matmul_precision's three words for this package's dense products.

"highest" (the default): six bf16 products per fp32 product, fp32-grade results -- what every parity test pins.  "high": three
products (two bf16 planes per operand, TF32 grade: every dropped term below 2^-14 |a||b|).  "medium": one product (one plane, bf16
grade: operands truncated to 8 significand bits).  A permission, not an obligation: the word alone governs the x6 GEMM kernel
only.  ``set_float32_matmul_precision(mode, panels=True)`` extends it to the row-panel kernels (csrc/panel.hip: the plain,
streamed, multi- and summed products, the conv stages, the EGNN node stages): their weights are then packed with two / one plane,
their row images in LDS hold two / one plane, and they sum the same three / one terms.  The flag is off by default and a call
without the keyword switches it off again, so the word keeps its earlier meaning at every earlier call site.  Products that go
to neither (the fp32 library below its threshold, the EGNN edge kernel, the batched weight gradients) and all row-wise work stay
at fp32 grade in every mode.  ops.products and the panel operators read the mode at call time (an autograd node of the panel
operators multiplies its backward pass as it multiplied its forward pass); a captured step replays the mode it was captured
under (trainer keys its graphs by the word and the flag).  profiles/panel_precision_bench.json has what the flag gains.
"""
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}     # mode -> `products` of hg_gemm_bf16_batch and of the panel entry points
PLANES = {6: 3, 3: 2, 1: 1}                           # products -> bf16 planes per operand
_mode = "highest"
_panels = False


def set_float32_matmul_precision(mode: str, panels: bool = False) -> None:
    global _mode, _panels
    if mode not in PRODUCTS:
        raise ValueError(f"matmul precision must be one of {tuple(PRODUCTS)}, not {mode!r}")
    _mode = mode
    _panels = bool(panels)


def get_float32_matmul_precision() -> str:
    return _mode


def get_float32_matmul_precision_panels() -> bool:
    """Whether the mode also governs the row-panel kernels (the ``panels`` keyword of the last set call)."""
    return _panels


def products() -> int:
    """Partial products per fp32 product under the current mode (6, 3 or 1)."""
    return PRODUCTS[_mode]


def panel_products() -> int:
    """Partial products per fp32 product of the row-panel kernels: the mode's with ``panels=True``, else 6."""
    return PRODUCTS[_mode] if _panels else 6
