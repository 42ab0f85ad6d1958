"""Matmul precision modes for the batched weight gradients: ``set_float32_matmul_precision(mode, wgrads=True)`` and the entry
point behind it, ``hg_wgrad_batch_bf16`` (csrc/wgrad.hip: both batched bf16 kernels with 3 / 2 / 1 planes per operand).

The model is the one of test_matmul_precision.py and test_panel_precision.py: the planes are rebuilt on the host by the same
truncation, ``sum_{i + j < P} dy_i^T x_j`` is formed in float64, and ``alpha``, the earlier contents of the destination and the
products that share a destination (in list order) are added.  Against that model only the fp32 accumulation differs, so the
tolerance is the one test_hip_kernels.py::test_wgrad_matches_float64 holds the fp32-grade kernel to against float64 for
unit-normal operands, ``3e-6 sqrt(K) 4`` (K summed over the products of a shared destination).  What makes that mean something
is asserted beside it: the "medium" model misses the "highest" model by more than the tolerance, and the kernel under
("highest", wgrads=True) gives the bits of ``hg_wgrad_batch_f32``.

Shapes: O x I of 64 x 64 (a quarter of a 128 x 128 workgroup tile), 128 x 128 and 192 x 64 (a ragged second tile row); K of 7 (no
whole 16-row step: the masked tail alone), 100 (ragged halves of a chunk) and 1000; one product and three.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_matmul_precision import MODES, PLANES, TRUNC, planes

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "equihgnn_hip.h")
WORD = {v: k for k, v in MODES.items()}                 # products -> mode


@pytest.fixture(autouse=True)
def _restore_mode():
    import equihgnn_amd
    yield
    equihgnn_amd.set_float32_matmul_precision("highest")


def tol(K):
    """test_wgrad_matches_float64's: fp32 accumulation of K unit-normal terms"""
    return 3e-6 * K ** 0.5 * 4


def plane_product(dy, x, P):
    """sum_{i + j < P} dy_i^T x_j in float64 (host tensors)"""
    pa, pb = [p.double() for p in planes(dy, P)], [p.double() for p in planes(x, P)]
    return sum(pa[i].t() @ pb[j] for i in range(P) for j in range(P - i))


def model(entries, before, P):
    """entries: [(dy, x, alpha, key)], before: {key: earlier contents of the destination}, all on the host ->
    ({key: destination after the launch, float64}, {key: summed K})"""
    out = {k: v.double().clone() for k, v in before.items()}
    ks = {k: 0 for k in before}
    for dy, x, alpha, key in entries:
        out[key] += alpha * plane_product(dy, x, P)
        ks[key] += dy.shape[0]
    return out, ks


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def flush(entries, mode, wgrads=True):
    """ops.wgrad_batch(entries) inside a deferral window under (mode, wgrads=...)"""
    import equihgnn_amd
    from equihgnn_amd import ops
    equihgnn_amd.set_float32_matmul_precision(mode, wgrads=wgrads)
    try:
        ops.defer_begin(DEV)
        ops.wgrad_batch(entries)
        ops.defer_flush(DEV)
        torch.cuda.synchronize()
    finally:
        equihgnn_amd.set_float32_matmul_precision("highest")


def entry_call(entries, products):
    """One direct call of hg_wgrad_batch_bf16 (products = None: of hg_wgrad_batch_f32) outside any deferral window; entries as
    for ops.wgrad_batch, whole contiguous operands.  Returns the status."""
    from equihgnn_amd import hip
    L = hip.lib()
    n = len(entries)
    O, I = entries[0][3].shape
    vp, i64, f32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_float * n
    ws_bytes = L.hg_wgrad_batch_workspace_bytes(n, O, I)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    args = [n, vp(*[e[0].data_ptr() for e in entries]), vp(*[e[1].data_ptr() for e in entries]), i64(*[e[0].shape[0] for e in entries]),
            O, I, f32(*[float(e[2]) for e in entries]), vp(*[e[3].data_ptr() for e in entries]), i64(*[e[3].stride(0) for e in entries]),
            1, ctypes.c_void_p(ws.data_ptr()), ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
            i64(*[e[0].stride(0) for e in entries]), i64(*[e[1].stride(0) for e in entries])]
    rc = L.hg_wgrad_batch_f32(*args) if products is None else L.hg_wgrad_batch_bf16(*args, products)
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_wgrads_keyword_sets_and_a_plain_call_resets_the_flag():
    import equihgnn_amd
    assert equihgnn_amd.get_float32_matmul_precision_wgrads() is False
    for mode in MODES:
        equihgnn_amd.set_float32_matmul_precision(mode, wgrads=True)
        assert equihgnn_amd.get_float32_matmul_precision() == mode and equihgnn_amd.get_float32_matmul_precision_wgrads() is True
        assert equihgnn_amd.get_float32_matmul_precision_panels() is False          # the two flags are separate
        equihgnn_amd.set_float32_matmul_precision(mode)                              # a plain call resets it
        assert equihgnn_amd.get_float32_matmul_precision() == mode and equihgnn_amd.get_float32_matmul_precision_wgrads() is False
    equihgnn_amd.set_float32_matmul_precision("medium", panels=True)                 # ... and so does a call with the other keyword
    assert equihgnn_amd.get_float32_matmul_precision_wgrads() is False and equihgnn_amd.get_float32_matmul_precision_panels() is True
    equihgnn_amd.set_float32_matmul_precision("high", panels=True, wgrads=True)
    assert equihgnn_amd.get_float32_matmul_precision_wgrads() is True and equihgnn_amd.get_float32_matmul_precision_panels() is True


@pytest.mark.parametrize("word", ["low", "HIGH", "", None, 3])
def test_a_bad_word_raises_value_error_and_leaves_the_mode_and_the_flag(word):
    import equihgnn_amd
    from equihgnn_amd import precision
    equihgnn_amd.set_float32_matmul_precision("high", wgrads=True)
    for kw in ({}, {"wgrads": True}, {"wgrads": False}):
        with pytest.raises(ValueError):
            equihgnn_amd.set_float32_matmul_precision(word, **kw)
        assert equihgnn_amd.get_float32_matmul_precision() == "high"
        assert equihgnn_amd.get_float32_matmul_precision_wgrads() is True and precision.wgrad_products() == 3


def test_wgrad_products_is_the_modes_count_with_the_flag_and_six_without():
    import equihgnn_amd
    from equihgnn_amd import precision
    assert precision.wgrad_products() == 6
    for mode, products in MODES.items():
        equihgnn_amd.set_float32_matmul_precision(mode, wgrads=True)
        assert precision.wgrad_products() == products == precision.products()
        assert precision.panel_products() == 6
        equihgnn_amd.set_float32_matmul_precision(mode)
        assert precision.wgrad_products() == 6 and precision.products() == products
        equihgnn_amd.set_float32_matmul_precision(mode, panels=True)
        assert precision.wgrad_products() == 6 and precision.panel_products() == products


def test_entry_point_is_declared_exported_and_bound_from_the_header():
    from equihgnn_amd import build, hip
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in the header"
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    old, new = params("hg_wgrad_batch_f32"), params("hg_wgrad_batch_bf16")
    assert len(old) == 15 and new == old + ["int32_t products"]          # the arguments of hg_wgrad_batch_f32 plus the count
    build.build(verbose=False)
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "hg_wgrad_batch_bf16")
    res, args = hip.SIGNATURES["hg_wgrad_batch_bf16"]                     # derived from the header: no hand-kept mirror
    res_old, args_old = hip.SIGNATURES["hg_wgrad_batch_f32"]
    assert res is ctypes.c_int32 and res_old is ctypes.c_int32
    assert list(args) == list(args_old) + [ctypes.c_int32] and len(args) == 16
    fn = hip.lib().hg_wgrad_batch_bf16
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert "hg_wgrad_batch_bf16" not in open(os.path.join(ROOT, "equihgnn_amd", "hip.py")).read()


@pytest.mark.parametrize("products", [0, 2, 4, 5, 7, -1, 12])
def test_products_outside_1_3_6_is_an_argument_error_before_anything_else(products):
    """the library loads without a device; the count is refused before any pointer is looked at (they are never dereferenced)"""
    from equihgnn_amd import hip
    L = hip.lib()
    vp, i64, f32 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_float * 1
    p = vp(4096)
    assert L.hg_wgrad_batch_bf16(1, p, p, i64(64), 64, 64, f32(1.0), p, i64(64), 1, ctypes.c_void_p(4096), 1 << 30, None,
                                 i64(64), i64(64), products) == hip.EQH_ERR_ARG
    assert L.hg_wgrad_batch_bf16(0, None, None, None, 64, 64, None, None, None, 1, None, 0, None, None, None, products) == hip.EQH_ERR_ARG
    assert L.hg_wgrad_batch_bf16(0, None, None, None, 64, 64, None, None, None, 1, None, 0, None, None, None, 6) == 0   # (the control)


def test_trainer_keys_its_graphs_by_the_wgrads_flag():
    import equihgnn_amd
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    b = synth_batch(2, 1)
    keys = set()
    for mode in MODES:
        pair = []
        for wgrads in (False, True):
            equihgnn_amd.set_float32_matmul_precision(mode, wgrads=wgrads)
            pair.append(GraphedTrainStep._key(b))
            assert pair[-1][-1] == mode and pair[-1][-2] is False         # (where the earlier tests read the word and `panels`)
        assert pair[0] != pair[1], f"{mode}: the key does not carry the flag"
        keys.update(pair)
    equihgnn_amd.set_float32_matmul_precision("medium", panels=True, wgrads=True)
    keys.add(GraphedTrainStep._key(b))
    assert len(keys) == 7


def test_trainer_keys_a_2d_batch_by_the_wgrads_flag_too():
    import types
    import equihgnn_amd
    from equihgnn_amd.trainer import GraphedTrainStep
    b = types.SimpleNamespace(x=torch.zeros(5, 3), edge_index=torch.zeros(2, 7, dtype=torch.long), y=torch.zeros(2, 1))
    equihgnn_amd.set_float32_matmul_precision("high")
    off = GraphedTrainStep._key(b)
    equihgnn_amd.set_float32_matmul_precision("high", wgrads=True)
    assert GraphedTrainStep._key(b) != off


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the operator
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [7, 100, 1000])
@pytest.mark.parametrize("O,I", [(64, 64), (128, 128), (192, 64)])
def test_each_mode_computes_exactly_its_products(O, I, K):
    """a batch of one product and a batch of three, fresh (zero) destinations, every mode: the plane model to the accumulation
    tolerance; a single product also within the truncation bound of the plain float64 product; "highest" with the flag the bits
    of hg_wgrad_batch_f32; the word without the flag the bits of "highest"."""
    g = torch.Generator().manual_seed(1000 * O + 10 * I + K)
    host = [(randn(g, K, O), randn(g, K, I)) for _ in range(3)]
    dev = [(dy.to(DEV), x.to(DEV)) for dy, x in host]
    for n in (1, 3):
        got = {}
        for mode, products in MODES.items():
            outs = [torch.zeros(O, I, device=DEV) for _ in range(n)]
            flush([(dy, x, 1.0, o) for (dy, x), o in zip(dev[:n], outs)], mode)
            got[mode] = [o.cpu() for o in outs]
            P = PLANES[products]
            for q, ((dy, x), o) in enumerate(zip(host[:n], got[mode])):
                want = plane_product(dy, x, P)
                err = float((o.double() - want).abs().max())
                full, mag = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()
                print(f"[{O}x{I} K={K} n={n} #{q}] {mode}: |dW - model| {err:.3e} (tolerance {tol(K):.3e}), |dW - dy^T x| "
                      f"{float((o.double() - full).abs().max()):.3e}")
                assert err <= tol(K), (mode, n, q, err)
                assert bool(((o.double() - full).abs() <= TRUNC[P] * mag + tol(K)).all()), (mode, n, q)
        for (dy, x) in host[:n]:                     # the test means something: the models are further apart than the tolerance
            assert float((plane_product(dy, x, 1) - plane_product(dy, x, 3)).abs().max()) > tol(K)
        assert all(not torch.equal(a, b) for a, b in zip(got["high"], got["highest"])), "high: the mode is not engaged"
        # six products through the new entry point / the flag: the bits of hg_wgrad_batch_f32
        old = [torch.zeros(O, I, device=DEV) for _ in range(n)]
        assert entry_call([(dy, x, 1.0, o) for (dy, x), o in zip(dev[:n], old)], None) == 0
        assert all(torch.equal(a.cpu(), b) for a, b in zip(old, got["highest"]))
        for products in (6, 3, 1):                   # ... and the direct call with a count is what the mode gives
            new = [torch.zeros(O, I, device=DEV) for _ in range(n)]
            assert entry_call([(dy, x, 1.0, o) for (dy, x), o in zip(dev[:n], new)], products) == 0
            assert all(torch.equal(a.cpu(), b) for a, b in zip(new, got[WORD[products]])), products
        for mode in ("high", "medium"):              # the word alone leaves the weight gradients at six products
            outs = [torch.zeros(O, I, device=DEV) for _ in range(n)]
            flush([(dy, x, 1.0, o) for (dy, x), o in zip(dev[:n], outs)], mode, wgrads=False)
            assert all(torch.equal(a.cpu(), b) for a, b in zip(outs, got["highest"])), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_shared_and_column_block_destinations_strided_operands_alpha_and_earlier_contents(mode):
    """one launch of four 64 x 128 products: two share a whole-matrix destination (K = 100 and 1000, summed in list order, the
    tolerance of the summed K), one goes with alpha = 0.5 into a column block of a wider matrix whose other columns must stay,
    one reads both operands as column blocks of wider row-major matrices (ld > O, ld > I); every destination is non-zero before"""
    O, I, P = 64, 128, PLANES[MODES[mode]]
    g = torch.Generator().manual_seed(77)
    dy0, x0, dy1, x1, dy2, x2 = randn(g, 100, O), randn(g, 100, I), randn(g, 1000, O), randn(g, 1000, I), randn(g, 100, O), randn(g, 100, I)
    wdy, wx = randn(g, 333, 3 * O), randn(g, 333, 2 * I + 64)
    dy3, x3 = wdy[:, O:2 * O], wx[:, 64:64 + I]
    shared, wide, own = randn(g, O, I), randn(g, O, 64 + I + 64), randn(g, O, I)
    d_shared, d_wide, d_own = shared.to(DEV), wide.to(DEV), own.to(DEV)
    d_wdy, d_wx = wdy.to(DEV), wx.to(DEV)
    entries = [(dy0.to(DEV), x0.to(DEV), 1.0, d_shared), (dy2.to(DEV), x2.to(DEV), 0.5, d_wide[:, 64:64 + I]),
               (dy1.to(DEV), x1.to(DEV), 2.0, d_shared), (d_wdy[:, O:2 * O], d_wx[:, 64:64 + I], 1.0, d_own)]
    assert entries[3][0].stride(0) == 3 * O and entries[3][1].stride(0) == 2 * I + 64
    flush(entries, mode)
    want, ks = model([(dy0, x0, 1.0, "shared"), (dy2, x2, 0.5, "wide"), (dy1, x1, 2.0, "shared"), (dy3, x3, 1.0, "own")],
                     {"shared": shared, "wide": wide[:, 64:64 + I], "own": own}, P)
    assert ks == {"shared": 1100, "wide": 100, "own": 333}
    for key, got in (("shared", d_shared), ("wide", d_wide[:, 64:64 + I]), ("own", d_own)):
        err = float((got.cpu().double() - want[key]).abs().max())
        print(f"{mode} {key}: |dW - model| {err:.3e} (tolerance {tol(ks[key]):.3e})")
        assert err <= tol(ks[key]), (mode, key, err)
    assert torch.equal(d_wide[:, :64].cpu(), wide[:, :64]) and torch.equal(d_wide[:, 64 + I:].cpu(), wide[:, 64 + I:])
    assert torch.equal(d_wdy.cpu(), wdy) and torch.equal(d_wx.cpu(), wx)
    if P < 3:      # the reduced model is another value than the full one here too
        full, _ = model([(dy0, x0, 1.0, "shared"), (dy1, x1, 2.0, "shared")], {"shared": shared}, 3)
        if P == 1:
            assert float((full["shared"] - want["shared"]).abs().max()) > tol(1100)
        assert float((d_shared.cpu().double() - full["shared"]).abs().max()) > 0.0


@pytest.mark.gpu
def test_the_wide_form_in_every_mode():
    """64 products of [100 x 128]^T [100 x 256]: (O / 128) (I / 256) x 64 per launch x 5 >= 256, so the dispatcher takes the
    128 x 256 workgroup tiles by its own rule and cuts K into 256 / 64 = four chunks of 32 rows, the last one a 4-row masked tail
    (the 128 x 128 form would cut this list into three: the workspace query, which follows the same rule, is asserted to answer
    four, and EQH_WGRAD_DEBUG=1 prints "128 x 256 tiles, 4 chunks of K" for the launch.  NOT yet confirmed on a device: no GPU
    could be had while this test was written, see the commit message).  Pairs of products share a destination; every mode
    against its plane model, six products the bits of hg_wgrad_batch_f32."""
    from equihgnn_amd import hip
    n, K, O, I = 64, 100, 128, 256
    assert (O // 128) * (I // 256) * n * 5 >= 256 and n <= 64
    assert hip.lib().hg_wgrad_batch_workspace_bytes(n, O, I) == n * 4 * O * I * 4          # four chunks of K: the wide plan
    g = torch.Generator().manual_seed(5)
    dys, xs = randn(g, n, K, O), randn(g, n, K, I)
    d_dys, d_xs = dys.to(DEV), xs.to(DEV)
    before = randn(g, n // 2, O, I)
    got = {}
    for mode, products in MODES.items():
        P = PLANES[products]
        dst = before.to(DEV)
        flush([(d_dys[q], d_xs[q], 1.0, dst[q // 2]) for q in range(n)], mode)
        got[mode] = dst.cpu()
        worst = 0.0
        for d in range(n // 2):
            want = before[d].double() + plane_product(dys[2 * d], xs[2 * d], P) + plane_product(dys[2 * d + 1], xs[2 * d + 1], P)
            worst = max(worst, float((got[mode][d].double() - want).abs().max()))
        print(f"wide form {mode}: |dW - model| {worst:.3e} (tolerance {tol(2 * K):.3e})")
        assert worst <= tol(2 * K), (mode, worst)
    assert float((plane_product(dys[0], xs[0], 1) - plane_product(dys[0], xs[0], 3)).abs().max()) > tol(2 * K)
    assert not torch.equal(got["high"], got["highest"]) and not torch.equal(got["medium"], got["high"])
    old = before.to(DEV)
    assert entry_call([(d_dys[q], d_xs[q], 1.0, old[q // 2]) for q in range(n)], None) == 0
    assert torch.equal(old.cpu(), got["highest"])


@pytest.mark.gpu
@pytest.mark.parametrize("products", [2, 0, 12])
def test_a_bad_count_through_ctypes_is_refused_and_leaves_the_destination(products):
    from equihgnn_amd import hip
    g = torch.Generator().manual_seed(9)
    dy, x = randn(g, 100, 64).to(DEV), randn(g, 100, 64).to(DEV)
    out = torch.full((64, 64), 7.0, device=DEV)
    assert entry_call([(dy, x, 1.0, out)], products) == hip.EQH_ERR_ARG
    assert float((out - 7.0).abs().max()) == 0.0
    assert entry_call([(dy, x, 1.0, out)], 1) == 0                      # (the control: the same call with a valid count runs)
    assert float((out - 7.0).abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_step_under_medium_with_and_without_the_flag_and_recapture(monkeypatch):
    """mhnnm, hidden 64, synth_batch(32): the trainer's eager step under deferral with ("medium", wgrads=True), every call of
    ops.grads.wgrad_batch recorded (operands and earlier destinations cloned).  Every destination after the flush is the
    one-plane model of its recorded operands; the same step under "medium" alone gives other gradients, equal to the three-plane
    model.  Then three steps of GraphedTrainStep with the flag toggled: the step is captured again, the loss stays finite."""
    import equihgnn_amd
    from common import fill_state_dict, zero_dropouts
    from equihgnn_amd import models
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.ops import grads
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    method = "mhnnm"
    net = models.MODELS[method](1, default_args(method=method, MLP_hidden=64, output_hidden=32))
    fill_state_dict(net, 3)
    zero_dropouts(net)
    net.to(DEV).train()
    raw = synth_batch(32, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 32
    tr = GraphedTrainStep(net, lr=0.0, keep_grads=True)        # lr 0: the weights stay
    tr.index_prefetch = False

    rec = {"on": False, "calls": []}
    real = grads.wgrad_batch

    def recording(entries):
        if rec["on"]:
            seen = {}
            for dy, x, alpha, into in entries:
                key = (into.data_ptr(), into.stride(0))
                if key not in seen:
                    seen[key] = (into, into.clone())
            rec["calls"].append(([(dy.clone(), x.clone(), float(alpha), (into.data_ptr(), into.stride(0))) for dy, x, alpha, into in entries],
                                 seen))
        return real(entries)
    monkeypatch.setattr(grads, "wgrad_batch", recording)

    def check(calls, P, what):
        n, worst = 0, 0.0
        for entries, seen in calls:
            host = [(dy.cpu(), x.cpu(), alpha, key) for dy, x, alpha, key in entries]
            want, ks = model(host, {k: b.cpu() for k, (_, b) in seen.items()}, P)
            for key, (into, _) in seen.items():
                err = float((into.cpu().double() - want[key]).abs().max())
                worst = max(worst, err / tol(ks[key]))
                assert err <= tol(ks[key]), (what, tuple(into.shape), ks[key], err)
            n += len(entries)
        print(f"{what}: {n} recorded products in {len(calls)} launches, worst |dW - model| / tolerance {worst:.3e}")
        return n

    def grads_now():
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters() if p.grad is not None]

    equihgnn_amd.set_float32_matmul_precision("medium", wgrads=True)
    rec["on"] = True
    loss = [float(tr.step(batch))]                               # the eager first step: its last pass runs under deferral
    torch.cuda.synchronize()
    first, rec["calls"] = rec["calls"], []
    assert check(first, 1, "medium + wgrads") >= 3, "no batched weight gradient was recorded: the test shows nothing"
    g_on = grads_now()
    equihgnn_amd.set_float32_matmul_precision("medium")
    tr._fwd_bwd(batch)                                           # the same eager pass under the word alone
    torch.cuda.synchronize()
    second, rec["calls"] = rec["calls"], []
    rec["on"] = False
    assert check(second, 3, "medium alone") == sum(len(e) for e, _ in first)
    g_off = grads_now()
    assert len(g_on) == len(g_off) > 10
    assert any(not torch.equal(a, b) for a, b in zip(g_on, g_off)), "the flag does not reach the weight gradients"
    # the medium model is further from the highest model than the tolerance, for the recorded operands as well
    dy, x, _, _ = max((e for entries, _ in first for e in entries), key=lambda e: float(e[0].abs().max()))
    print(f"largest recorded dy: max |dy| {float(dy.abs().max()):.3e}, medium vs highest model "
          f"{float((plane_product(dy.cpu(), x.cpu(), 1) - plane_product(dy.cpu(), x.cpu(), 3)).abs().max()):.3e}")

    captures = []
    cap = tr._capture
    monkeypatch.setattr(tr, "_capture", lambda static: (captures.append(equihgnn_amd.get_float32_matmul_precision_wgrads()), cap(static))[1])
    for wgrads in (True, False, True):                           # capture, capture anew, replay the first
        equihgnn_amd.set_float32_matmul_precision("medium", wgrads=wgrads)
        loss.append(float(tr.step(batch)))
        if wgrads and len(captures) == 1:
            assert len(tr.slots) == 1
    assert captures == [True, False] and len(tr.slots) == 2
    assert sorted(k[-3] for k in tr.slots) == [False, True] and all(k[-1] == "medium" for k in tr.slots)
    assert all(np.isfinite(loss)), loss
    assert all(bool(torch.isfinite(g).all()) for g in grads_now())
