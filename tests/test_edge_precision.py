"""Matmul precision modes for the fused EGNN edge update: ``set_float32_matmul_precision(mode, edges=True)`` and the entry points
behind it, ``egnn_edge_fwd_p`` / ``egnn_edge_bwd_p`` (csrc/egnn_edge.hip with 3 / 2 / 1 bf16 planes per operand of its matrix
products: the forward's silu(h) W2^T, the backward's dpre2 W2 of the receiver and the sender pass and dW2 = dpre2^T silu(h)).

Kernel level.  Everything is compared with the explicit per-edge formulation in float64.  A result of a mode with P planes may miss
the float64 value by the truncation of its operands, ``TRUNC[P]`` (test_matmul_precision.py) times the same contraction evaluated on
absolute values, on top of what the fp32-grade kernel is held to; that the reduced modes are really taken is asserted beside it: the
one- and two-plane results lie (rms) at less than a quarter of their distance to the float64 product from the float64 plane model
``sum_{i + j < P} a_i . b_j`` of host-truncated operands, and differ in bits from the six-product result.

Inputs are those of test_hip_kernels.py::test_egnn_edge_fused_matches_float64_reference, except that neighbours are drawn from
[0, N - 5) (the last five senders have no in-edge: their dB rows must be exactly zero), that for N > 20 one column points at node 3
(one sender's entries span several 16-entry tiles of the sender pass) and that no self column is forced.

Model level.  The tolerance is measured on the CPU from the reference side, not chosen: the oracle of egnn_equihnns_c64 in eval mode
with both operands of ONLY the second edge Linear (``edge_mlp[3]`` of its EGNN: the product the flag governs in a forward pass)
reduced by the same truncation, its largest deviation from the fixture (|out - ref| / max(1, |ref|)), times 4 for the different
accumulation order.  Measured (``test_model_tolerances_are_the_measured_ones`` repeats the measurement):
    egnn_equihnns_c64   high 8.98e-5 -> 3.6e-4     medium 1.99e-2 -> 8.0e-2
"""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from common import assert_close, batch_from_case, load_case
from test_matmul_precision import MODES, PLANES, TRUNC, planes
from test_oracle_golden import build as build_case_model

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "equihgnn_hip.h")
CASE = "egnn_equihnns_c64"
MODEL_DEV = {"high": 8.98e-5, "medium": 1.99e-2}     # the oracle with edge_mlp[3] truncated against the fixture (see the header)
MODEL_TOL = {k: 4 * v for k, v in MODEL_DEV.items()}
# (N, Hp): fewer nodes than one tile; two k-steps over four wavefronts; N no multiple of the nodes per workgroup and a ragged last
# sender tile; the BASELINE width (the nine-step template, the largest W2 image); the forward on the fp32 kernel
SHAPES = [(7, 128), (16, 64), (37, 192), (50, 1088), (50, 2112)]
TAKEN = [(37, 192), (50, 1088)]
COUNTS = (6, 3, 1)


@pytest.fixture(autouse=True)
def _restore_mode():
    import equihgnn_amd
    yield
    equihgnn_amd.set_float32_matmul_precision("highest")


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def flags():
    import equihgnn_amd as E
    return (E.get_float32_matmul_precision(), E.get_float32_matmul_precision_panels(), E.get_float32_matmul_precision_wgrads(),
            E.get_float32_matmul_precision_edges())


def test_the_edges_keyword_sets_and_a_plain_call_resets_the_flag():
    import equihgnn_amd
    assert flags() == ("highest", False, False, False)
    for mode in MODES:
        equihgnn_amd.set_float32_matmul_precision(mode, edges=True)
        assert flags() == (mode, False, False, True)                                 # the three flags are separate
        equihgnn_amd.set_float32_matmul_precision(mode)                              # a plain call resets it
        assert flags() == (mode, False, False, False)
    equihgnn_amd.set_float32_matmul_precision("medium", edges=True)
    equihgnn_amd.set_float32_matmul_precision("medium", panels=True)                 # ... and so does a call with another keyword
    assert flags() == ("medium", True, False, False)
    equihgnn_amd.set_float32_matmul_precision("medium", edges=True)
    equihgnn_amd.set_float32_matmul_precision("medium", wgrads=True)
    assert flags() == ("medium", False, True, False)
    equihgnn_amd.set_float32_matmul_precision("high", panels=True, wgrads=True)
    equihgnn_amd.set_float32_matmul_precision("high", edges=True)                    # ... and the other way round
    assert flags() == ("high", False, False, True)
    equihgnn_amd.set_float32_matmul_precision("high", panels=True, wgrads=True, edges=True)
    assert flags() == ("high", True, True, True)


@pytest.mark.parametrize("word", ["low", "HIGH", "", None, 3])
def test_a_bad_word_raises_value_error_and_leaves_the_mode_and_all_three_flags(word):
    import equihgnn_amd
    from equihgnn_amd import precision
    for before in (dict(edges=True), dict(panels=True, wgrads=True), dict(panels=True, edges=True)):
        equihgnn_amd.set_float32_matmul_precision("high", **before)
        was = flags()
        for kw in ({}, {"edges": True}, {"edges": False}, {"panels": True, "wgrads": True, "edges": True}):
            with pytest.raises(ValueError):
                equihgnn_amd.set_float32_matmul_precision(word, **kw)
            assert flags() == was
            assert precision.edge_products() == (3 if before.get("edges") else 6)


def test_edge_products_is_the_modes_count_with_the_flag_and_six_without():
    import equihgnn_amd
    from equihgnn_amd import precision
    assert precision.edge_products() == 6
    for mode, products in MODES.items():
        equihgnn_amd.set_float32_matmul_precision(mode, edges=True)
        assert precision.edge_products() == products == precision.products()
        assert precision.panel_products() == 6 and precision.wgrad_products() == 6   # ... which it leaves alone
        equihgnn_amd.set_float32_matmul_precision(mode)
        assert precision.edge_products() == 6 and precision.products() == products
        equihgnn_amd.set_float32_matmul_precision(mode, panels=True, wgrads=True)
        assert precision.edge_products() == 6 and precision.panel_products() == products == precision.wgrad_products()
        equihgnn_amd.set_float32_matmul_precision(mode, panels=True, wgrads=True, edges=True)
        assert precision.edge_products() == precision.panel_products() == precision.wgrad_products() == products


def test_entry_points_are_declared_exported_and_bound_from_the_header():
    from equihgnn_amd import build, hip
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in the header"
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    build.build(verbose=False)
    dll = ctypes.CDLL(hip.LIB_PATH)
    source = open(os.path.join(ROOT, "equihgnn_amd", "hip.py")).read()
    for old_name, n_old in (("egnn_edge_fwd", 11), ("egnn_edge_bwd", 22)):
        name = old_name + "_p"
        old, new = params(old_name), params(name)
        assert len(old) == n_old and new == old + ["int32_t products"]       # the old parameters plus the count
        assert hasattr(dll, name) and hasattr(dll, old_name)
        res, args = hip.SIGNATURES[name]                                      # derived from the header: no hand-kept mirror
        res_old, args_old = hip.SIGNATURES[old_name]
        assert res is ctypes.c_int32 and res_old is ctypes.c_int32
        assert list(args) == list(args_old) + [ctypes.c_int32] and len(args) == n_old + 1
        fn = getattr(hip.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
        assert name not in source


JUNK = ctypes.c_void_p(4096)     # never dereferenced


def fwd_junk(N, products):
    from equihgnn_amd import hip
    return hip.lib().egnn_edge_fwd_p(JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, N, 64, JUNK, JUNK, None, products)


def bwd_junk(N, products):
    """(N = 0 with accumulating dwd / dw2 and no db2: nothing is written, so no device is needed)"""
    from equihgnn_amd import hip
    return hip.lib().egnn_edge_bwd_p(JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, JUNK, 16, JUNK, JUNK, N, 64, JUNK, JUNK, JUNK, JUNK, None, 0, 1,
                                     JUNK, 1 << 30, None, products)


@pytest.mark.parametrize("products", [0, 2, 4, 5, 7, -1, 12])
def test_products_outside_1_3_6_is_an_argument_error_before_anything_else(products):
    """the library loads without a device; the count is refused before any pointer is looked at (they are never dereferenced)"""
    from equihgnn_amd import hip
    assert fwd_junk(1000, products) == hip.EQH_ERR_ARG and bwd_junk(1000, products) == hip.EQH_ERR_ARG
    assert fwd_junk(0, products) == hip.EQH_ERR_ARG and bwd_junk(0, products) == hip.EQH_ERR_ARG
    assert hip.lib().egnn_edge_fwd_p(None, None, None, None, None, None, 0, 64, None, None, None, products) == hip.EQH_ERR_ARG


def test_six_products_with_no_node_is_ok():
    from equihgnn_amd import hip
    for products in (6, 3, 1):                                                      # (the control of the test above)
        assert fwd_junk(0, products) == 0 and bwd_junk(0, products) == 0
    assert hip.lib().egnn_edge_fwd_p(None, None, None, None, None, None, 0, 64, None, None, None, 6) == 0
    assert hip.lib().egnn_edge_fwd(None, None, None, None, None, None, 0, 64, None, None, None) == 0


def test_trainer_keys_its_graphs_by_the_edges_flag():
    import equihgnn_amd
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    b = synth_batch(2, 1)
    keys = set()
    for mode in MODES:
        pair = []
        for edges in (False, True):
            equihgnn_amd.set_float32_matmul_precision(mode, edges=edges)
            pair.append(GraphedTrainStep._key(b))
            assert pair[-1][-1] == mode and pair[-1][-2] is False                   # (where the earlier tests read the word and `panels`)
            assert pair[-1][-3] is False                                            # (... and `wgrads`)
        assert pair[0] != pair[1], f"{mode}: the key does not carry the flag"
        keys.update(pair)
    equihgnn_amd.set_float32_matmul_precision("medium", panels=True, edges=True)
    k = GraphedTrainStep._key(b)
    assert k[-1] == "medium" and k[-2] is True and k[-3] is False
    keys.add(k)
    assert len(keys) == 7


def test_trainer_keys_a_2d_batch_by_the_edges_flag_too():
    import equihgnn_amd
    from equihgnn_amd.trainer import GraphedTrainStep
    b = types.SimpleNamespace(x=torch.zeros(5, 3), edge_index=torch.zeros(2, 7, dtype=torch.long), y=torch.zeros(2, 1))
    equihgnn_amd.set_float32_matmul_precision("high", panels=True)
    off = GraphedTrainStep._key(b)
    equihgnn_amd.set_float32_matmul_precision("high", panels=True, edges=True)
    on = GraphedTrainStep._key(b)
    assert on != off and on[-1] == off[-1] == "high" and on[-2] is True and off[-2] is True


def test_model_tolerances_are_the_measured_ones():
    """repeats the measurement behind MODEL_DEV on the oracle (CPU): the constants are what the reference side gives"""
    import torch.nn.functional as F
    case = load_case(CASE)
    model = build_case_model(case).eval()
    data = batch_from_case(case)
    ref = case["out"].astype(np.float64)
    lin = model.egnn_layer.edge_mlp[3]                       # the second edge Linear: [2 (2 C + 1)] -> 16
    assert isinstance(lin, torch.nn.Linear) and lin.out_features == 16
    with torch.no_grad():
        assert_close(model(data).numpy(), ref, 1e-5, "the oracle in eval mode gives the fixture")
        for mode in ("high", "medium"):
            P = PLANES[MODES[mode]]

            def forward(x, P=P):
                xs, ws = planes(x, P), planes(lin.weight, P)
                return sum(F.linear(xs[i], ws[j]) for i in range(P) for j in range(P - i)) + lin.bias
            lin.forward = forward
            try:
                out = model(data).numpy().astype(np.float64)
            finally:
                del lin.forward
            dev = float((np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max())
            print(f"{CASE} {mode}: oracle with the second edge Linear truncated deviates {dev:.3e} (recorded {MODEL_DEV[mode]:.3e})")
            assert MODEL_DEV[mode] / 1.5 <= dev <= MODEL_DEV[mode] * 1.5


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------------
def silu_grad64(x):
    sig = torch.sigmoid(x)
    return sig + x * sig * (1 - sig)


@functools.lru_cache(maxsize=None)
def problem(N, Hp):
    """inputs (host, fp32) and everything the tests compare with, in float64; computed once per shape and only read afterwards"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(1000 * N + Hp)
    ab = torch.randn(N, 2 * Hp, generator=g)
    wd = torch.randn(Hp, generator=g) * 0.3
    w2 = torch.randn(16, Hp, generator=g) / Hp ** 0.5
    b2 = torch.randn(16, generator=g) * 0.1
    nbr = torch.randint(0, N - 5, (N, 16), generator=g)     # the last five senders have no in-edge
    if N > 20:
        nbr[:, 5] = 3                                       # one sender's entries span several 16-entry tiles
    d2 = torch.rand(N, 16, generator=g) * 3
    dm = torch.randn(N, 16, generator=g)
    p = types.SimpleNamespace(N=N, Hp=Hp, ab=ab, wd=wd, w2=w2, b2=b2, nbr=nbr, d2=d2, dm=dm)
    A, B, W2, D2 = ab[:, :Hp].double(), ab[:, Hp:].double(), w2.double(), d2.double()
    p.h = A[:, None, :] + B[nbr] + D2[..., None] * wd.double()             # [N, 16, Hp]
    p.s = F.silu(p.h)
    p.sabs = p.s.abs() @ W2.abs().T                                         # sum_k |s_k| |W2_ok|
    p.pre2 = p.s @ W2.T + b2.double()
    p.m = F.silu(p.pre2).sum(1)
    # the backward starts from pre2 rounded to fp32 (what the kernel is given), so the forward's error does not enter
    p.pre2_f32 = p.pre2.float()
    p.dpre2 = dm.double()[:, None, :] * silu_grad64(p.pre2_f32.double())    # [N, 16, 16]
    p.dsilu = silu_grad64(p.h)
    gk = p.dpre2 @ W2
    gk_abs = p.dpre2.abs() @ W2.abs()
    dh, dh_abs = gk * p.dsilu, gk_abs * p.dsilu.abs()
    flat = nbr.reshape(-1)
    p.grads = {"dA": dh.sum(1), "dB": torch.zeros(N, Hp, dtype=torch.float64).index_add_(0, flat, dh.reshape(-1, Hp)),
               "dw2": torch.einsum("ijo,ijk->ok", p.dpre2, p.s), "dwd": (dh * D2[..., None]).sum((0, 1)),
               "db2": p.dpre2.sum((0, 1))}
    p.bound = {"dA": dh_abs.sum(1), "dB": torch.zeros(N, Hp, dtype=torch.float64).index_add_(0, flat, dh_abs.reshape(-1, Hp)),
               "dw2": torch.einsum("ijo,ijk->ok", p.dpre2.abs(), p.s.abs()), "dwd": (dh_abs * D2[..., None]).sum((0, 1)),
               "db2": torch.zeros(16, dtype=torch.float64)}
    return p


def on_device(p):
    if not hasattr(p, "dev"):
        from equihgnn_amd import ops
        d = types.SimpleNamespace(**{k: getattr(p, k).to(DEV) for k in ("ab", "wd", "w2", "b2", "d2", "dm")})
        d.nbr = p.nbr.to(DEV).int()
        d.csr_t = ops.csr_build(p.nbr.reshape(-1).to(DEV), None, p.N)
        d.pre2 = p.pre2_f32.to(DEV)
        p.dev = d
    return p.dev


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fwd(p, products):
    """egnn_edge_fwd_p (products = None: egnn_edge_fwd) -> (m, pre2) on the host"""
    from equihgnn_amd import hip
    d, L = on_device(p), hip.lib()
    m = torch.full((p.N, 16), float("nan"), device=DEV)
    pre2 = torch.full((p.N, 16, 16), float("nan"), device=DEV)
    args = [ptr(d.ab), ptr(d.wd), ptr(d.w2), ptr(d.b2), ptr(d.nbr), ptr(d.d2), p.N, p.Hp, ptr(m), ptr(pre2), stream()]
    rc = L.egnn_edge_fwd(*args) if products is None else L.egnn_edge_fwd_p(*args, products)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return m.cpu(), pre2.cpu()


def bwd(p, products, pre2=None):
    """egnn_edge_bwd_p (products = None: egnn_edge_bwd) from the float64 pre2 rounded to fp32 (or from `pre2`, on the device) -> the
    gradients on the host"""
    from equihgnn_amd import hip
    d, L = on_device(p), hip.lib()
    N, Hp = p.N, p.Hp
    nan = float("nan")
    dab, dwd, dw2 = torch.full((N, 2 * Hp), nan, device=DEV), torch.full((Hp,), nan, device=DEV), torch.full((16, Hp), nan, device=DEV)
    dpre2, db2 = torch.full((N, 16, 16), nan, device=DEV), torch.full((16,), nan, device=DEV)
    ws_bytes = L.egnn_edge_bwd_workspace_bytes(N, Hp)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    args = [ptr(d.ab), ptr(d.wd), ptr(d.w2), ptr(d.nbr), ptr(d.d2), ptr(d.pre2 if pre2 is None else pre2), ptr(d.dm), 16, ptr(d.csr_t.rowptr), ptr(d.csr_t.perm),
            N, Hp, ptr(dab), ptr(dwd), ptr(dw2), ptr(dpre2), ptr(db2), 0, 0, ptr(ws), ws_bytes, stream()]
    rc = L.egnn_edge_bwd(*args) if products is None else L.egnn_edge_bwd_p(*args, products)
    torch.cuda.synchronize()
    assert rc == 0, rc
    dab = dab.cpu()
    return {"dA": dab[:, :Hp], "dB": dab[:, Hp:], "dw2": dw2.cpu(), "dwd": dwd.cpu(), "db2": db2.cpu(), "dpre2": dpre2.cpu()}


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


def plane_matmul(a, b, P):
    """sum_{i + j < P} a_i @ b_j in float64, the planes cut from the operands rounded to fp32"""
    pa, pb = [x.double() for x in planes(a.float(), P)], [x.double() for x in planes(b.float(), P)]
    return sum(pa[i] @ pb[j] for i in range(P) for j in range(P - i))


@pytest.mark.gpu
@pytest.mark.parametrize("N,Hp", SHAPES)
def test_forward_of_every_count_against_float64(N, Hp):
    p = problem(N, Hp)
    six = fwd(p, 6)
    for products in COUNTS:
        P = PLANES[products]
        m, pre2 = six if products == 6 else fwd(p, products)
        bound = TRUNC[P] * p.sabs + Hp * 2.0 ** -23 * p.sabs + 2e-6
        err = (pre2.double() - p.pre2).abs()
        print(f"[{N} x {Hp}] {products} products: max |pre2 - pre2_64| {float(err.max()):.3e}, largest share of its bound "
              f"{float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), (products, float((err / bound).max()))
        # m sums silu over the 16 slots (|silu'| < 1.1); on top, what the fp32-grade kernel is held to
        scale = float(p.m.abs().max())
        bound_m = 1.1 * bound.sum(1) + 2e-6 * max(scale, 1) + 1e-5 * p.m.abs()
        err_m = (m.double() - p.m).abs()
        print(f"[{N} x {Hp}] {products} products: max |m - m_64| {float(err_m.max()):.3e}, largest share of its bound "
              f"{float((err_m / bound_m).max()):.3e}")
        assert bool((err_m <= bound_m).all()), (products, float((err_m / bound_m).max()))
        if Hp > 1152:       # the forward runs its fp32-MFMA kernel there: fp32 grade in every mode
            assert torch.equal(m, six[0]) and torch.equal(pre2, six[1]), products


@pytest.mark.gpu
@pytest.mark.parametrize("N,Hp", SHAPES)
def test_backward_of_every_count_against_float64(N, Hp):
    p = problem(N, Hp)
    for products in COUNTS:
        P = PLANES[products]
        got = bwd(p, products)
        for name in ("dA", "dB", "dw2", "dwd", "db2"):       # db2 is no matrix product: the fp32 tolerance alone (its bound is zero)
            want = p.grads[name]
            bound = TRUNC[P] * p.bound[name] + 2e-5 * float(want.abs().max())
            err = (got[name].double() - want).abs()
            print(f"[{N} x {Hp}] {products} products {name}: max error {float(err.max()):.3e} (largest magnitude "
                  f"{float(want.abs().max()):.3e}), largest share of its bound {float((err / bound).max()):.3e}")
            assert bool((err <= bound).all()), (products, name, float((err / bound).max()))
        assert float(got["dB"][N - 5:].abs().max()) == 0.0, "senders without an in-edge have a zero row"
        assert float((got["dpre2"].double() - p.dpre2).abs().max()) <= 2e-5 * float(p.dpre2.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("N,Hp", TAKEN)
def test_the_reduced_modes_are_really_taken(N, Hp):
    """pre2, dA and dw2 of the one- and two-plane kernels are their own plane model, not the full product (rms, not max: an operand
    that the kernel computes one fp32 ulp off the float64 one can land on the other side of a bf16 boundary)"""
    p = problem(N, Hp)
    W2 = p.w2.double()
    full = {"pre2": p.pre2, "dA": p.grads["dA"], "dw2": p.grads["dw2"]}
    got = {}
    for products in COUNTS:
        b = bwd(p, products)
        got[products] = {"pre2": fwd(p, products)[1], "dA": b["dA"], "dw2": b["dw2"]}
    to_full = {}
    for products in (3, 1):
        P = PLANES[products]
        model = {"pre2": plane_matmul(p.s.reshape(-1, Hp), W2.T, P).reshape(N, 16, 16) + p.b2.double(),
                 "dA": (plane_matmul(p.dpre2.reshape(-1, 16), W2, P).reshape(N, 16, Hp) * p.dsilu).sum(1),
                 "dw2": plane_matmul(p.dpre2.reshape(-1, 16).T, p.s.reshape(-1, Hp), P)}
        for name in ("pre2", "dA", "dw2"):
            g = got[products][name].double()
            near, far = rms(g - model[name]), rms(g - full[name])
            to_full[products, name] = far
            print(f"[{N} x {Hp}] {products} products {name}: rms distance to its plane model {near:.3e}, to the float64 product "
                  f"{far:.3e} (ratio {near / far:.3e})")
            assert near < 0.25 * far, (products, name, near, far)
            assert not torch.equal(got[products][name], got[6][name]), (products, name)
    for name in ("pre2", "dA", "dw2"):
        assert to_full[3, name] < to_full[1, name], name


@pytest.mark.gpu
@pytest.mark.parametrize("N,Hp", SHAPES)
def test_six_products_are_the_old_entry_points_and_every_count_repeats_its_bits(N, Hp):
    import equihgnn_amd
    from equihgnn_amd import ops
    p = problem(N, Hp)
    d = on_device(p)
    old_f, old_b = fwd(p, None), bwd(p, None)
    for products in COUNTS:
        f, b = fwd(p, products), bwd(p, products)
        f2, b2 = fwd(p, products), bwd(p, products)
        assert all(torch.equal(x, y) for x, y in zip(f, f2)) and all(torch.equal(b[k], b2[k]) for k in b), products
        if products == 6:
            assert all(torch.equal(x, y) for x, y in zip(f, old_f)), "six products: not the forward of egnn_edge_fwd"
            assert all(torch.equal(b[k], old_b[k]) for k in b), "six products: not the gradients of egnn_edge_bwd"
    # the flag is off by default and the word alone does not reach this kernel: the operator under "medium" gives the bits of
    # the old entry points (its backward starts from its own pre2, so the old backward is run from that too)
    equihgnn_amd.set_float32_matmul_precision("medium")
    leaves = [x.clone().requires_grad_(True) for x in (d.ab, d.wd, d.w2, d.b2)]
    m = ops.egnn_edge(*leaves, d.nbr, d.d2, d.csr_t)
    (m * d.dm).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(m.detach().cpu(), old_f[0])
    want = bwd(p, None, pre2=old_f[1].to(DEV))
    dab = leaves[0].grad.cpu()
    assert torch.equal(dab[:, :Hp], want["dA"]) and torch.equal(dab[:, Hp:], want["dB"])
    assert torch.equal(leaves[1].grad.cpu(), want["dwd"]) and torch.equal(leaves[2].grad.cpu(), want["dw2"])
    assert torch.equal(leaves[3].grad.cpu(), want["db2"])


def operator_run(p, at_forward, at_backward):
    """ops.egnn_edge with the mode set to `at_forward` before the forward and to `at_backward` before .backward()"""
    import equihgnn_amd
    from equihgnn_amd import ops
    d = on_device(p)
    leaves = [x.clone().requires_grad_(True) for x in (d.ab, d.wd, d.w2, d.b2)]
    equihgnn_amd.set_float32_matmul_precision(*at_forward[:1], **at_forward[1])
    m = ops.egnn_edge(*leaves, d.nbr, d.d2, d.csr_t)
    equihgnn_amd.set_float32_matmul_precision(*at_backward[:1], **at_backward[1])
    (m * d.dm).sum().backward()
    torch.cuda.synchronize()
    equihgnn_amd.set_float32_matmul_precision("highest")
    return [m.detach().cpu()] + [x.grad.cpu() for x in leaves]


@pytest.mark.gpu
def test_the_backward_multiplies_with_the_count_of_its_forward_pass():
    p = problem(37, 192)
    medium, highest = ("medium", dict(edges=True)), ("highest", {})
    stay_m, stay_h = operator_run(p, medium, medium), operator_run(p, highest, highest)
    assert all(torch.equal(a, b) for a, b in zip(operator_run(p, medium, highest), stay_m))
    assert all(torch.equal(a, b) for a, b in zip(operator_run(p, highest, medium), stay_h))
    assert all(not torch.equal(a, b) for a, b in zip(stay_m[:4], stay_h[:4])), "the flag does not reach the operator"
    # ... and the operator's one-product pass is the entry points' (forward, then the backward from that pre2)
    assert torch.equal(stay_m[0], fwd(p, 1)[0]) and torch.equal(stay_h[0], fwd(p, 6)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_forward_with_the_edges_under_the_reduced_modes():
    import equihgnn_amd
    from equihgnn_amd import models
    case = load_case(CASE)
    model = build_case_model(case, models.MODELS).eval().to(DEV)
    data = batch_from_case(case).to(DEV)
    ref = case["out"].astype(np.float64)

    def forward(mode, edges):
        equihgnn_amd.set_float32_matmul_precision(mode, edges=edges)
        if hasattr(data, "_hyper_index"):
            data._hyper_index = None
        with torch.no_grad():
            return model(data).cpu().numpy().astype(np.float64)
    highest = forward("highest", True)
    assert_close(highest, ref, 1e-5, "highest + edges")
    assert np.array_equal(highest, forward("highest", False))
    for mode in ("high", "medium"):
        out = forward(mode, True)
        dev = float((np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(f"{CASE} {mode} + edges: differs from highest by {float(np.abs(out - highest).max()):.3e}, from the fixture by "
              f"{dev:.3e} (tolerance {MODEL_TOL[mode]:.3e})")
        assert dev <= MODEL_TOL[mode], (mode, dev)
        assert not np.array_equal(out, highest), f"{mode}: the output is the one of highest -- the mode is not engaged"
        assert not np.array_equal(out, forward(mode, False)), f"{mode}: the flag does not reach the edge kernel"


@pytest.mark.gpu
def test_training_under_medium_with_the_edges_and_recapture_when_the_flag_changes(monkeypatch):
    """GraphedTrainStep on egnn_equihnns hidden 64, synth_batch(32): three steps on a repeated batch under ("medium", edges=True)
    (the eager first step, the capture, a replay) with a finite, decreasing loss; switching the flag off captures a second graph
    for the bucket, switching it on again replays the first"""
    import equihgnn_amd
    from common import fill_state_dict, zero_dropouts
    from equihgnn_amd import models
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    method = "egnn_equihnns"
    model = models.MODELS[method](1, default_args(method=method, MLP_hidden=64, output_hidden=32))
    fill_state_dict(model, 3)
    zero_dropouts(model)
    model.to(DEV).train()
    raw = synth_batch(32, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 32
    tr = GraphedTrainStep(model, keep_grads=True)
    tr.index_prefetch = False
    captures = []
    real = tr._capture
    monkeypatch.setattr(tr, "_capture", lambda static: (captures.append(
        (equihgnn_amd.get_float32_matmul_precision(), equihgnn_amd.get_float32_matmul_precision_edges())), real(static))[1])

    def grads_now():
        torch.cuda.synchronize()
        return [q.grad.clone() for q in model.parameters() if q.grad is not None]
    equihgnn_amd.set_float32_matmul_precision("medium", edges=True)
    losses = [float(tr.step(batch)) for _ in range(3)]
    print("losses under medium + edges:", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
    assert captures == [("medium", True)] and len(tr.slots) == 1
    g = grads_now()
    assert len(g) > 10 and all(bool(torch.isfinite(x).all()) for x in g) and any(float(x.abs().max()) > 0 for x in g)
    equihgnn_amd.set_float32_matmul_precision("medium")
    losses.append(float(tr.step(batch)))                           # a second graph for the same bucket
    assert captures == [("medium", True), ("medium", False)] and len(tr.slots) == 2
    assert sorted((k[-1], k[-4]) for k in tr.slots) == [("medium", False), ("medium", True)]
    equihgnn_amd.set_float32_matmul_precision("medium", edges=True)
    losses.append(float(tr.step(batch)))                           # the first graph again: nothing new
    assert captures == [("medium", True), ("medium", False)] and len(tr.slots) == 2
    assert all(np.isfinite(losses)), losses
