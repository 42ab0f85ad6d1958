"""Matmul precision modes: ``equihgnn_amd.set_float32_matmul_precision`` ("highest" / "high" / "medium") and the entry point
behind it, ``hg_gemm_bf16_batch`` (csrc/gemm_x6.hip with 3 / 2 / 1 bf16 planes per operand: 6 / 3 / 1 products).

Kernel level.  The planes are rebuilt on the host by the same truncation (top 16 bits, then the top 16 bits of the remainder),
``C_P = sum_{i + j < P} A_i . B_j`` is formed in float64, and a mode must compute EXACTLY its products: ``|C - C_P| <= K 2^-23
(|A|.|B|)``, the fp32 accumulation error alone -- a bound that the reduced modes' results must at the same time VIOLATE against the
full product ``A.B`` (so a kernel that quietly kept all six products fails).  The distance from ``A.B`` stays within the bound that
follows from the truncation: |a - a0| < 2^-7 |a|, |a - a0 - a1| < 2^-14 |a|, so per term "medium" errs by at most
(2 2^-7 + 2^-14) |a||b| and "high" by at most 3 2^-14 |a||b|.

Split-K.  The K = 512 case runs with the workspace query and a workspace pointer as every product of ops.gemm does; the plan of
gemm_x6.hip (gx_plan) splits only from 64 K steps of 32 on, so at K = 512 it takes one pass.  A K = 2560 case is added whose plan does
split (its workspace query is asserted non-zero), so that the slab path is covered in every mode.

Model level.  Tolerances are measured on the CPU from the reference side, not chosen: the oracle restatement run in eval mode with both
operands of every F.linear reduced by the same truncation (``truncated_linears`` below), its largest deviation from the fixture
(|out - ref| / max(1, |ref|)), times 4 for the different accumulation order.  Measured (``test_model_tolerances_are_the_measured_ones``
repeats the measurement):
    equiformer_equihnns_c64   high 5.16e-5 -> 2.1e-4     medium 1.21e-2 -> 4.9e-2
    faformer_equihnns_c64     high 7.53e-5 -> 3.0e-4     medium 1.27e-2 -> 5.1e-2
"""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import assert_close, batch_from_case, load_case
from test_oracle_golden import build as build_case_model

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "equihgnn_hip.h")
PLANES = {6: 3, 3: 2, 1: 1}                       # products -> planes
MODES = {"highest": 6, "high": 3, "medium": 1}
TRUNC = {3: 0.0, 2: 3 * 2.0 ** -14, 1: 2 * 2.0 ** -7 + 2.0 ** -14}      # planes -> per-term truncation error, in |a||b|
# largest deviation of the oracle with truncated Linear operands from the fixture (measured on the CPU: see the header)
MODEL_DEV = {("equiformer_equihnns_c64", "high"): 5.16e-5, ("equiformer_equihnns_c64", "medium"): 1.21e-2,
             ("faformer_equihnns_c64", "high"): 7.53e-5, ("faformer_equihnns_c64", "medium"): 1.27e-2}
MODEL_TOL = {k: 4 * v for k, v in MODEL_DEV.items()}


@pytest.fixture(autouse=True)
def _restore_mode():
    import equihgnn_amd
    yield
    equihgnn_amd.set_float32_matmul_precision("highest")


# ---------------------------------------------------------------------------------------------------------------------------
# host-side construction
# ---------------------------------------------------------------------------------------------------------------------------
def planes(x: torch.Tensor, n: int):
    """The first n bf16 planes of an fp32 tensor, as fp32 tensors: the top 16 bits, then the top 16 bits of the remainder, ..."""
    out, r = [], x.float().contiguous()
    for _ in range(n):
        p = (r.view(torch.int32) & -65536).view(torch.float32)
        out.append(p)
        r = r - p                                   # (exact: p is a truncation of r)
    return out


def product_ref(a, b, ta, tb, n_planes):
    """(C_P, A.B, |A|.|B|) in float64 for op(a) [M, K], op(b) [K, N]"""
    A, B = (a.t() if ta else a), (b.t() if tb else b)
    pa, pb = [p.double() for p in planes(A, n_planes)], [p.double() for p in planes(B, n_planes)]
    c_p = sum(pa[i] @ pb[j] for i in range(n_planes) for j in range(n_planes - i))
    return c_p, A.double() @ B.double(), A.double().abs() @ B.double().abs()


def operands(M, N, K, ta, tb, seed):
    """mixed sign, rows of a and b scaled over a few orders of magnitude (the low planes matter in every dot product)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((K, M) if ta else (M, K), generator=g)
    b = torch.randn((N, K) if tb else (K, N), generator=g)
    a *= torch.exp(2.0 * torch.randn(a.shape[0], 1, generator=g))
    b *= torch.exp(2.0 * torch.randn(b.shape[0], 1, generator=g))
    a *= torch.exp(1.0 * torch.randn(a.shape, generator=g))
    return a, b


def run(entries, tile, products, new_entry=True, with_ws=True):
    """One launch of hg_gemm_bf16_batch (or hg_gemm_x6_batch) over `entries`: dicts with a, b, ta, tb and optionally bias, d,
    alpha, beta, relu (tensors on the device).  Returns (outputs, workspace bytes)."""
    from equihgnn_amd import hip
    L = hip.lib()
    n = len(entries)
    arr = (hip.HgGemmProblem * n)()
    outs = []
    for q, e in zip(arr, entries):
        a, b, ta, tb = e["a"], e["b"], e.get("ta", False), e.get("tb", True)
        M, K = (a.shape[1], a.shape[0]) if ta else a.shape
        N = b.shape[0] if tb else b.shape[1]
        out = torch.empty(M, N, device=a.device)
        q.a, q.lda, q.b, q.ldb, q.c, q.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), N
        q.m, q.n, q.k, q.trans_a, q.trans_b = M, N, K, int(ta), int(tb)
        q.alpha, q.beta, q.relu = float(e.get("alpha", 1.0)), float(e.get("beta", 1.0)), int(e.get("relu", False))
        if e.get("bias") is not None:
            q.bias = e["bias"].data_ptr()
        if e.get("d") is not None:
            q.d, q.ldd = e["d"].data_ptr(), e["d"].stride(0)
        outs.append(out)
    ws_bytes = L.hg_gemm_x6_workspace_bytes(n, arr, tile) if with_ws else 0
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wp = ctypes.c_void_p(ws.data_ptr()) if with_ws else None
    if new_entry:
        rc = L.hg_gemm_bf16_batch(n, arr, tile, products, wp, ws_bytes, stream)
    else:
        rc = L.hg_gemm_x6_batch(n, arr, tile, wp, ws_bytes, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return outs, ws_bytes


def check_product(out, a, b, ta, tb, products, what):
    """the two assertions of the header for one result"""
    K = a.shape[0] if ta else a.shape[1]
    P = PLANES[products]
    c_p, full, scale = product_ref(a, b, ta, tb, P)
    acc = K * 2.0 ** -23 * scale
    got = out.cpu().double()
    e_own = ((got - c_p).abs() / scale).max().item()
    e_full = ((got - full).abs() / scale).max().item()
    print(f"{what} products={products}: |C - C_P| {e_own:.3e} (bound {K * 2.0 ** -23:.3e}), |C - A.B| {e_full:.3e} "
          f"(bound {TRUNC[P] + K * 2.0 ** -23:.3e}) of |A|.|B|")
    assert bool(((got - c_p).abs() <= acc).all()), (what, products, e_own)
    if P < 3:
        # The reference values themselves are told apart from the full product by this bound: checked on the CPU for every case
        # of this file -- at K = 36 and 100 some entry of C_P lies 2.5 x (high) to 2600 x (medium) the bound away from A.B.  (At
        # K >= 512 the bound, which grows with K, has overtaken the truncation error of "high": only "medium" is told apart there.)
        far = (c_p - full).abs() > 2 * acc
        if K <= 100 or P == 1:
            assert bool(far.any()), "the operands do not separate this mode from the full product"
        # ... and so is the result, wherever C_P is two bounds away (the result is within one of C_P): the mode dropped its planes
        assert bool(((got - full).abs() > acc)[far].all()), (what, products, "computed more than its products")
        assert bool(((got - full).abs() <= TRUNC[P] * scale + acc).all()), (what, products, e_full)


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_default_mode_is_highest_and_the_three_words_round_trip():
    import equihgnn_amd
    from equihgnn_amd import precision
    assert equihgnn_amd.get_float32_matmul_precision() == "highest"
    for mode, products in MODES.items():
        equihgnn_amd.set_float32_matmul_precision(mode)
        assert equihgnn_amd.get_float32_matmul_precision() == mode
        assert precision.products() == products
    equihgnn_amd.set_float32_matmul_precision("highest")
    assert equihgnn_amd.get_float32_matmul_precision() == "highest"


@pytest.mark.parametrize("word", ["low", "HIGH", "", "bf16", None, 3])
def test_a_bad_word_raises_value_error_and_leaves_the_mode(word):
    import equihgnn_amd
    equihgnn_amd.set_float32_matmul_precision("high")
    with pytest.raises(ValueError):
        equihgnn_amd.set_float32_matmul_precision(word)
    assert equihgnn_amd.get_float32_matmul_precision() == "high"


def test_entry_point_is_declared_exported_and_bound_from_the_header():
    from equihgnn_amd import build, hip
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+hg_gemm_bf16_batch\s*\(([^;{]*)\)\s*;", text)
    assert m, "hg_gemm_bf16_batch is not declared in the header"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["int32_t n_problems", "const HgGemmProblem* problems", "int32_t tile", "int32_t products", "void* workspace",
                      "size_t workspace_bytes", "void* stream"]
    build.build(verbose=False)
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "hg_gemm_bf16_batch")
    res, args = hip.SIGNATURES["hg_gemm_bf16_batch"]                # derived from the header: no hand-kept mirror
    assert res is ctypes.c_int32 and len(args) == 7
    assert args[0] is ctypes.c_int32 and args[2] is ctypes.c_int32 and args[3] is ctypes.c_int32 and args[5] is ctypes.c_size_t
    fn = hip.lib().hg_gemm_bf16_batch
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert "hg_gemm_bf16_batch" not in open(os.path.join(ROOT, "equihgnn_amd", "hip.py")).read()


@pytest.mark.parametrize("products", [0, 2, 4, 5, 7, -1, 12])
def test_products_outside_1_3_6_is_an_argument_error_before_anything_else(products):
    """the library loads without a device; the value is refused before the problems are looked at (a null problem array with a
    valid count would otherwise be the argument error of its own, so a VALID host-side array is passed too)"""
    from equihgnn_amd import hip
    L = hip.lib()
    arr = (hip.HgGemmProblem * 1)()
    arr[0].a = arr[0].b = arr[0].c = 4096                          # never dereferenced: the call must return first
    arr[0].m, arr[0].n, arr[0].k, arr[0].lda, arr[0].ldb, arr[0].ldc, arr[0].trans_b = 64, 64, 64, 64, 64, 64, 1
    assert L.hg_gemm_bf16_batch(1, arr, 0, products, None, 0, None) == hip.EQH_ERR_ARG


def test_trainer_keys_its_graphs_by_the_mode():
    import equihgnn_amd
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    b = synth_batch(2, 1)
    keys = {}
    for mode in MODES:
        equihgnn_amd.set_float32_matmul_precision(mode)
        keys[mode] = GraphedTrainStep._key(b)
        assert mode in keys[mode]
    assert len(set(keys.values())) == 3


@contextlib.contextmanager
def truncated_linears(n_planes):
    """every F.linear of the oracle with both operands reduced to their first n_planes bf16 planes and the products with
    i + j < n_planes summed in fp32: the reference side of a reduced mode"""
    import torch.nn.functional as F
    real = F.linear

    def linear(x, w, bias=None):
        xs, ws = planes(x, n_planes), planes(w, n_planes)
        y = sum(real(xs[i], ws[j]) for i in range(n_planes) for j in range(n_planes - i))
        return y if bias is None else y + bias

    F.linear = linear
    try:
        yield
    finally:
        F.linear = real


@pytest.mark.parametrize("name", ["equiformer_equihnns_c64", "faformer_equihnns_c64"])
def test_model_tolerances_are_the_measured_ones(name):
    """repeats the measurement behind MODEL_DEV on the oracle (CPU): the constants are what the reference side gives"""
    case = load_case(name)
    model = build_case_model(case).eval()
    data = batch_from_case(case)
    ref = case["out"].astype(np.float64)
    with torch.no_grad():
        assert_close(model(data).numpy(), ref, 1e-5, "the oracle in eval mode gives the fixture")
        for mode in ("high", "medium"):
            with truncated_linears(PLANES[MODES[mode]]):
                out = model(data).numpy().astype(np.float64)
            dev = float((np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max())
            print(f"{name} {mode}: oracle with truncated Linear operands deviates {dev:.3e} (recorded {MODEL_DEV[name, mode]:.3e})")
            assert MODEL_DEV[name, mode] / 1.5 <= dev <= MODEL_DEV[name, mode] * 1.5


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel
# ---------------------------------------------------------------------------------------------------------------------------
# M in {70, 200} x N in {36, 132} (no multiple of a tile) x K in {36, 100} (no multiple of 32), the four transpositions, every
# tile code (trans_a needs M % 4 == 0: 200)
SHAPES = [(70, 36, 36, False, True, 64), (200, 132, 100, False, True, 128), (70, 132, 100, False, False, 256),
          (200, 36, 36, False, False, 512), (200, 132, 36, True, False, 513), (200, 36, 100, True, True, 64),
          (200, 132, 100, True, True, 256), (70, 132, 36, False, True, 512), (70, 36, 100, False, False, 513),
          (200, 132, 100, True, False, 128), (200, 36, 100, True, True, 512), (70, 132, 100, False, True, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,ta,tb,tile", SHAPES)
def test_each_mode_computes_exactly_its_products(M, N, K, ta, tb, tile):
    a, b = operands(M, N, K, ta, tb, M + 3 * N + 7 * K + tile)
    e = dict(a=a.to(DEV), b=b.to(DEV), ta=ta, tb=tb)
    for products in (6, 3, 1):
        (out,), _ = run([e], tile, products)
        check_product(out, a, b, ta, tb, products, f"[{M}x{N}x{K} ta={ta} tb={tb} tile={tile}]")
        (again,), _ = run([e], tile, products)
        assert torch.equal(out, again), "two runs of a mode differ"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,ta,tb,tile,splits", [(200, 132, 512, False, True, 64, False), (200, 36, 512, True, False, 0, False),
                                                     (200, 36, 2560, True, False, 64, True), (70, 132, 2560, False, True, 256, True)])
def test_each_mode_through_the_workspace_and_split_k(M, N, K, ta, tb, tile, splits):
    """K = 512 with the workspace query and pointer (one pass: the plan splits from 64 K steps on), K = 2560 really split"""
    import equihgnn_amd
    from equihgnn_amd import ops
    a, b = operands(M, N, K, ta, tb, M + N + K)
    e = dict(a=a.to(DEV), b=b.to(DEV), ta=ta, tb=tb)
    for products in (6, 3, 1):
        (out,), ws_bytes = run([e], tile, products)
        assert (ws_bytes > 0) == splits
        check_product(out, a, b, ta, tb, products, f"[{M}x{N}x{K} ta={ta} tb={tb} tile={tile} ws={ws_bytes}]")
        (again,), _ = run([e], tile, products)
        assert torch.equal(out, again)
        if splits:                                   # the accumulating form of the weight gradients: c += a b through the slabs
            c_p, _, scale = product_ref(a, b, ta, tb, PLANES[products])
            d = torch.randn(M, N, generator=torch.Generator().manual_seed(1)) * scale.float()
            acc = d.to(DEV)
            equihgnn_amd.set_float32_matmul_precision({6: "highest", 3: "high", 1: "medium"}[products])
            ops.gemm(e["a"], e["b"], trans_a=ta, trans_b=tb, d=acc, out=acc)
            equihgnn_amd.set_float32_matmul_precision("highest")
            bound = K * 2.0 ** -23 * scale + 2.0 ** -23 * (d.double().abs() + scale)
            assert bool(((acc.cpu().double() - (d.double() + c_p)).abs() <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [64, 128, 256, 512, 513, 0])
def test_six_products_through_the_new_entry_are_the_bits_of_hg_gemm_x6_batch(tile):
    entries = []
    for i, (M, N, K, ta, tb) in enumerate([(70, 132, 100, False, True), (200, 36, 36, False, True)]):
        a, b = operands(M, N, K, ta, tb, 11 + i)
        entries.append(dict(a=a.to(DEV), b=b.to(DEV), ta=ta, tb=tb))
    g = torch.Generator().manual_seed(3)
    entries[1].update(bias=torch.randn(36, generator=g).to(DEV), d=torch.randn(200, 36, generator=g).to(DEV), beta=0.5, relu=True)
    old, _ = run(entries, tile, 6, new_entry=False)
    new, _ = run(entries, tile, 6)
    for o, n_ in zip(old, new):
        assert torch.equal(o, n_)
    a, b = operands(200, 132, 2560, True, False, 5)               # and through split-K
    e = [dict(a=a.to(DEV), b=b.to(DEV), ta=True, tb=False)]
    assert torch.equal(run(e, tile, 6, new_entry=False)[0][0], run(e, tile, 6)[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("products", [6, 3, 1])
def test_a_batch_of_two_different_problems(products):
    entries, host = [], []
    for i, (M, N, K) in enumerate([(70, 132, 100), (200, 36, 36)]):
        a, b = operands(M, N, K, False, True, 21 + i)
        host.append((a, b))
        entries.append(dict(a=a.to(DEV), b=b.to(DEV)))
    outs, _ = run(entries, 0, products)
    outs2, _ = run(entries, 0, products)
    for (a, b), o, o2 in zip(host, outs, outs2):
        check_product(o, a, b, False, True, products, f"batch {tuple(a.shape)}")
        assert torch.equal(o, o2)


@pytest.mark.gpu
@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("tile", [64, 512])
def test_epilogue_bias_relu_and_addend_in_a_reduced_mode(products, tile):
    """relu(alpha C_P + beta D + bias): the same construction, the accumulation bound scaled by |alpha| plus the epilogue's own
    three fp32 roundings"""
    M, N, K, alpha, beta = 200, 132, 100, 0.5, 2.0
    a, b = operands(M, N, K, False, True, 31)
    g = torch.Generator().manual_seed(32)
    c_p, full, scale = product_ref(a, b, False, True, PLANES[products])
    bias = torch.randn(N, generator=g) * scale.mean().float()
    d = torch.randn(M, N, generator=g) * scale.float()
    e = dict(a=a.to(DEV), b=b.to(DEV), bias=bias.to(DEV), d=d.to(DEV), alpha=alpha, beta=beta, relu=True)
    (out,), _ = run([e], tile, products)
    pre = alpha * c_p + beta * d.double() + bias.double()
    mag = alpha * scale + beta * d.double().abs() + bias.double().abs()
    bound = alpha * K * 2.0 ** -23 * scale + 3 * 2.0 ** -24 * mag
    got = out.cpu().double()
    assert bool(((got - torch.relu(pre)).abs() <= bound).all()), float(((got - torch.relu(pre)).abs() / bound).max())
    assert bool((got == 0).any()) and bool((got > 0).any())         # the ReLU cut something and kept something
    assert bool(((got - torch.relu(alpha * full + beta * d.double() + bias.double())).abs() > bound).any())    # reduced indeed
    (again,), _ = run([e], tile, products)
    assert torch.equal(out, again)


@pytest.mark.gpu
def test_a_presplit_image_goes_with_six_products_only():
    from equihgnn_amd import hip, ops
    import equihgnn_amd
    a, b = operands(200, 64, 64, False, True, 41)
    ad, bd = a.to(DEV), b.to(DEV)
    ref = ops.gemm(ad, bd, presplit=False)
    equihgnn_amd.set_float32_matmul_precision("medium")
    assert torch.equal(ops.gemm(ad, bd, presplit=True), ref)        # ops keeps six products for a packed weight
    from equihgnn_amd.ops.panel import panel_pack
    (img,) = panel_pack([(bd, True, 64)], k_major=True)
    arr = (hip.HgGemmProblem * 1)()
    out = torch.empty(200, 64, device=DEV)
    q = arr[0]
    q.a, q.lda, q.b_packed, q.c, q.ldc, q.m, q.n, q.k, q.trans_b, q.alpha = ad.data_ptr(), 64, img.data_ptr(), out.data_ptr(), 64, 200, 64, 64, 1, 1.0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for products in (3, 1):
        assert hip.lib().hg_gemm_bf16_batch(1, arr, 0, products, None, 0, stream) == hip.EQH_ERR_ARG
    assert hip.lib().hg_gemm_bf16_batch(1, arr, 0, 6, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["highest", "high", "medium"])
def test_ops_gemm_reads_the_mode_at_call_time(mode):
    """ops.gemm (forward x W^T, input gradient dY W, weight gradient dY^T X) under a mode is the launch with that mode's
    products, bit for bit -- and the mode is read at the call, not at import"""
    import equihgnn_amd
    from equihgnn_amd import ops
    for M, N, K, ta, tb in [(200, 132, 100, False, True), (200, 132, 100, False, False), (200, 36, 100, True, False)]:
        a, b = operands(M, N, K, ta, tb, 51)
        ad, bd = a.to(DEV), b.to(DEV)
        equihgnn_amd.set_float32_matmul_precision(mode)
        got = ops.gemm(ad, bd, trans_a=ta, trans_b=tb)
        equihgnn_amd.set_float32_matmul_precision("highest")
        (want,), _ = run([dict(a=ad, b=bd, ta=ta, tb=tb)], 0, MODES[mode])
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the models
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equiformer_equihnns_c64", "faformer_equihnns_c64"])
def test_model_forward_under_the_reduced_modes(name, monkeypatch):
    """eval-mode forward of a hidden-64 golden case with every eligible dense product on the kernel (X6_MIN_OUTPUTS = 0: at
    fixture size nothing reaches it otherwise): "highest" keeps the 1e-5 parity, "high" and "medium" move the output (the mode is
    engaged) and stay within 4 x the deviation the reference side shows under the same truncation"""
    import equihgnn_amd
    from equihgnn_amd import models
    from equihgnn_amd.ops import products as P
    monkeypatch.setattr(P, "X6_MIN_OUTPUTS", 0)
    case = load_case(name)
    model = build_case_model(case, models.MODELS).eval().to(DEV)
    data = batch_from_case(case).to(DEV)
    ref = case["out"].astype(np.float64)
    outs = {}
    with torch.no_grad():
        for mode in MODES:
            equihgnn_amd.set_float32_matmul_precision(mode)
            if hasattr(data, "_hyper_index"):
                data._hyper_index = None
            outs[mode] = model(data).cpu().numpy().astype(np.float64)
    assert_close(outs["highest"], ref, 1e-5, "highest")
    for mode in ("high", "medium"):
        moved = float(np.abs(outs[mode] - outs["highest"]).max())
        dev = float((np.abs(outs[mode] - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(f"{name} {mode}: differs from highest by {moved:.3e}, from the fixture by {dev:.3e} (tolerance {MODEL_TOL[name, mode]:.3e})")
        assert moved > 0.0, f"{mode}: the output is the one of highest -- the mode is not engaged"
        assert dev <= MODEL_TOL[name, mode], (mode, dev)
    assert np.abs(outs["medium"] - outs["highest"]).max() > np.abs(outs["high"] - outs["highest"]).max()


@pytest.mark.gpu
def test_training_under_medium_and_recapture_on_a_change_of_mode(monkeypatch):
    """training steps under "medium" leave finite gradients for every parameter that has one; GraphedTrainStep captures ANEW
    when the mode changes (capture count and slot keys), and goes back to the old graph when the mode does"""
    import equihgnn_amd
    from common import fill_state_dict, zero_dropouts
    from equihgnn_amd import models
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.ops import products as P
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    monkeypatch.setattr(P, "X6_MIN_OUTPUTS", 0)
    method = "faformer_equihnns"
    model = models.MODELS[method](1, default_args(method=method, MLP_hidden=64, output_hidden=32))
    fill_state_dict(model, 3)
    zero_dropouts(model)
    model.to(DEV).train()
    raw = synth_batch(8, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 8

    tr = GraphedTrainStep(model, lr=1e-3, keep_grads=True)     # (p.grad of the last step stays readable)
    tr.index_prefetch = False                     # one form of the step: no calibration captures in the count
    captures = []
    real = tr._capture
    monkeypatch.setattr(tr, "_capture", lambda static: (captures.append(equihgnn_amd.get_float32_matmul_precision()), real(static))[1])
    equihgnn_amd.set_float32_matmul_precision("highest")
    losses = [float(tr.step(batch)) for _ in range(3)]           # bootstrap, capture, replay
    assert captures == ["highest"] and len(tr.slots) == 1
    equihgnn_amd.set_float32_matmul_precision("medium")
    losses += [float(tr.step(batch)) for _ in range(2)]           # capture under the new mode, replay
    assert captures == ["highest", "medium"] and len(tr.slots) == 2
    assert sorted(k[-1] for k in tr.slots) == ["highest", "medium"]
    grads = [p.grad for p in model.parameters() if p.grad is not None]              # of the replayed step under "medium"
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    equihgnn_amd.set_float32_matmul_precision("highest")
    losses.append(float(tr.step(batch)))                          # the first graph again: nothing new
    assert captures == ["highest", "medium"] and len(tr.slots) == 2
    assert all(np.isfinite(losses)), losses
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
