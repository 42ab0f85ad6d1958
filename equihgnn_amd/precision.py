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
then split into two / one plane in registers and the same three / one terms are summed.
``set_float32_matmul_precision(mode, edges=True)`` extends it to the fused EGNN edge update (csrc/egnn_edge.hip, egnn_edge_fwd_p /
egnn_edge_bwd_p): the forward's silu(h) W2^T product, and the backward's dpre2 W2 products of the receiver and the sender pass
and its dW2 = dpre2^T silu(h) product (which lives in that kernel, so `edges` governs it, not `wgrads`), split their operands
into two / one plane in registers and sum three / one bf16 terms into fp32.  Where the forward runs its fp32-MFMA kernel (Hp above
1152, or EQH_EDGE_F32=1) it stays at fp32 grade in every mode; the backward is reduced at every width.  The three flags are
independent.  Products that go to none of these (the fp32 library below its threshold, the EGNN edge kernel without the `edges`
flag, the single-product and skinny weight gradients hg_wgrad_f32 and hg_wgrad_skinny_f32) and all row-wise work (the
recomputation of h, SiLU and its derivative, dwd, the row sums of dA / dB, every reduction) stay at fp32 grade in every mode.
So do the two one-launch read-out heads (csrc/readout.hip, csrc/readout_pair.hip): every product in them, the paired head's
[16, 2C] x [2C, H] first layer included, is the fp32 16 x 16 x 4 MFMA whatever the word and the flags say.
ops.products and the panel operators read the mode at call time (an autograd node of the panel
operators, and of the edge update, multiplies its backward pass as it multiplied its forward pass); a captured step replays the
mode it was captured under (trainer keys its graphs by the word and the three flags; ops.wgrad_batch reads the mode when it runs, at defer_flush).
profiles/panel_precision_bench.json has what the `panels` flag gains; tools/bench_matmul_precision.py --wgrads measures the
`wgrads` flag (into profiles/wgrad_precision_bench.json) and, with --edges, the `edges` flag (into
profiles/edge_precision_bench.json; no run of it is recorded yet).
"""
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}     # mode -> `products` of hg_gemm_bf16_batch and of the panel entry points
PLANES = {6: 3, 3: 2, 1: 1}                           # products -> bf16 planes per operand
_mode = "highest"
_panels = False
_wgrads = False
_edges = False


def set_float32_matmul_precision(mode: str, panels: bool = False, wgrads: bool = False, edges: bool = False) -> None:
    global _mode, _panels, _wgrads, _edges
    if mode not in PRODUCTS:
        raise ValueError(f"matmul precision must be one of {tuple(PRODUCTS)}, not {mode!r}")
    _mode = mode
    _panels = bool(panels)
    _wgrads = bool(wgrads)
    _edges = bool(edges)


def get_float32_matmul_precision() -> str:
    return _mode


def get_float32_matmul_precision_panels() -> bool:
    """Whether the mode also governs the row-panel kernels (the ``panels`` keyword of the last set call)."""
    return _panels


def get_float32_matmul_precision_wgrads() -> bool:
    """Whether the mode also governs the batched weight gradients (the ``wgrads`` keyword of the last set call)."""
    return _wgrads


def get_float32_matmul_precision_edges() -> bool:
    """Whether the mode also governs the fused EGNN edge kernels (the ``edges`` keyword of the last set call)."""
    return _edges


def products() -> int:
    """Partial products per fp32 product under the current mode (6, 3 or 1)."""
    return PRODUCTS[_mode]


def panel_products() -> int:
    """Partial products per fp32 product of the row-panel kernels: the mode's with ``panels=True``, else 6."""
    return PRODUCTS[_mode] if _panels else 6


def wgrad_products() -> int:
    """Partial products per fp32 product of the batched weight gradients: the mode's with ``wgrads=True``, else 6."""
    return PRODUCTS[_mode] if _wgrads else 6


def edge_products() -> int:
    """Partial products per fp32 product of the fused EGNN edge kernels: the mode's with ``edges=True``, else 6."""
    return PRODUCTS[_mode] if _edges else 6
