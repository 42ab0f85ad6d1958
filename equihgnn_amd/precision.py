"""The matmul precision mode: torch.set_float32_matmul_precision's three words for this package's dense products.

"highest" (the default): six bf16 products per fp32 product, fp32-grade results -- what every parity test pins.  "high": three
products (two bf16 planes per operand, TF32 grade: every dropped term below 2^-14 |a||b|).  "medium": one product (one plane, bf16
grade: operands truncated to 8 significand bits).  A permission, not an obligation: the word alone governs the x6 GEMM kernel
only.  ``set_float32_matmul_precision(mode, panels=True)`` extends it to the row-panel kernels (csrc/panel.hip: the plain,
streamed, multi- and summed products, the conv stages, the EGNN node stages): their weights are then packed with two / one plane,
their row images in LDS hold two / one plane, and they sum the same three / one terms.  The flag is off by default and a call
without the keyword switches it off again, so the word keeps its earlier meaning at every earlier call site.
``set_float32_matmul_precision(mode, wgrads=True)`` extends it, in the same way, to the batched weight gradients of a training
step (csrc/wgrad.hip, hg_wgrad_batch_bf16: the dY^T X products that defer_flush runs in one launch per shape): both operands are
then split into two / one plane in registers and the same three / one terms are summed.  Products that go to none of these (the
fp32 library below its threshold, the EGNN edge kernel, the single-product and skinny weight gradients hg_wgrad_f32 and
hg_wgrad_skinny_f32) and all row-wise work stay at fp32 grade in every mode.  ops.products and the panel operators read the mode at call time (an autograd node of the panel
operators multiplies its backward pass as it multiplied its forward pass); a captured step replays the mode it was captured
under (trainer keys its graphs by the word and both flags; ops.wgrad_batch reads the mode when it runs, at defer_flush).
profiles/panel_precision_bench.json has what the `panels` flag gains; tools/bench_matmul_precision.py --wgrads measures the
`wgrads` flag (into profiles/wgrad_precision_bench.json).
"""
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}     # mode -> `products` of hg_gemm_bf16_batch and of the panel entry points
PLANES = {6: 3, 3: 2, 1: 1}                           # products -> bf16 planes per operand
_mode = "highest"
_panels = False
_wgrads = False


def set_float32_matmul_precision(mode: str, panels: bool = False, wgrads: bool = False) -> None:
    global _mode, _panels, _wgrads
    if mode not in PRODUCTS:
        raise ValueError(f"matmul precision must be one of {tuple(PRODUCTS)}, not {mode!r}")
    _mode = mode
    _panels = bool(panels)
    _wgrads = bool(wgrads)


def get_float32_matmul_precision() -> str:
    return _mode


def get_float32_matmul_precision_panels() -> bool:
    """Whether the mode also governs the row-panel kernels (the ``panels`` keyword of the last set call)."""
    return _panels


def get_float32_matmul_precision_wgrads() -> bool:
    """Whether the mode also governs the batched weight gradients (the ``wgrads`` keyword of the last set call)."""
    return _wgrads


def products() -> int:
    """Partial products per fp32 product under the current mode (6, 3 or 1)."""
    return PRODUCTS[_mode]


def panel_products() -> int:
    """Partial products per fp32 product of the row-panel kernels: the mode's with ``panels=True``, else 6."""
    return PRODUCTS[_mode] if _panels else 6


def wgrad_products() -> int:
    """Partial products per fp32 product of the batched weight gradients: the mode's with ``wgrads=True``, else 6."""
    return PRODUCTS[_mode] if _wgrads else 6
