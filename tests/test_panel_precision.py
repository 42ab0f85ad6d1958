"""Matmul precision modes on the row-panel kernels: ``set_float32_matmul_precision(mode, panels=True)`` and the `products` /
`planes` arguments of the panel entry points behind it (csrc/panel.hip with NP = 6 / 3 / 1 products per fp32 product).

Operator level.  As tests/test_matmul_precision.py does for the x6 kernel, the planes are rebuilt on the host by the same
truncation (top 16 bits, then the top 16 bits of the remainder) and every product of an operator is formed in float64 from the
planes and terms its mode keeps, ``P(a, W) = sum_{i + j < planes} a_i . W_j``.  Against that model only the fp32 accumulation
differs, so a panel operator under its mode is held to the tolerance that the highest-mode test of the same operator
(tests/test_hip_kernels.py) uses against float64 -- a tolerance that a result with more or fewer terms misses (also asserted:
the model of "medium" is not the model of "highest" to that tolerance).  Chained operators are checked link by link from the
kernel's own intermediate rows, as those tests do.  A single product is also held to the bound against the plain float64
product that the truncation implies (3 2^-14 / (2 2^-7 + 2^-14) of sum |a||b|, plus K 2^-23 for the accumulation).

Model level.  Tolerances are measured on the CPU from the reference side as in tests/test_matmul_precision.py: the oracle in eval
mode with both operands of every F.linear cut by the same truncation, its largest deviation from the fixture
(|out - ref| / max(1, |ref|)), times 4 for the different accumulation order.  Measured
(``test_model_tolerances_are_the_measured_ones`` repeats the measurement):
    egnn_equihnns_c64   high 1.74e-4 -> 7.0e-4     medium 3.58e-2 -> 1.4e-1
    mhnnm_c64_eval      high 5.11e-5 -> 2.0e-4     medium 2.08e-2 -> 8.3e-2
"""
import ctypes

import numpy as np
import pytest
import torch

from common import assert_close, batch_from_case, load_case
from test_matmul_precision import MODES, PLANES, TRUNC, planes, truncated_linears
from test_oracle_golden import build as build_case_model

DEV = "cuda:0"
REDUCED = ("high", "medium")
MODEL_DEV = {("egnn_equihnns_c64", "high"): 1.74e-4, ("egnn_equihnns_c64", "medium"): 3.58e-2,
             ("mhnnm_c64_eval", "high"): 5.11e-5, ("mhnnm_c64_eval", "medium"): 2.08e-2}
MODEL_TOL = {k: 4 * v for k, v in MODEL_DEV.items()}
SHAPES = [(70, 64), (33, 64), (70, 128), (33, 128), (70, 256), (33, 256)]      # rows: three panels (the last of 6 rows) / one row in the second


@pytest.fixture(autouse=True)
def _restore_mode():
    import equihgnn_amd
    yield
    equihgnn_amd.set_float32_matmul_precision("highest")


def pack(items):
    """images of the planes that the current mode's panel products read (what the operators of the package pack)"""
    from equihgnn_amd import ops
    return ops.panel_pack(items, planes=ops.panel_planes())


def prod(a, b, n_planes):
    """P(a, b) = sum_{i + j < n_planes} a_i @ b_j in float64 (a [M, K], b [K, N], fp32 tensors on any device)"""
    pa, pb = [p.double() for p in planes(a, n_planes)], [p.double() for p in planes(b.contiguous(), n_planes)]
    return sum(pa[i] @ pb[j] for i in range(n_planes) for j in range(n_planes - i))


def ln64(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def under(mode, panels, fn):
    import equihgnn_amd
    equihgnn_amd.set_float32_matmul_precision(mode, panels=panels)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        equihgnn_amd.set_float32_matmul_precision("highest")


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_panels_keyword_sets_and_a_plain_call_resets_the_flag():
    import equihgnn_amd
    from equihgnn_amd import precision
    assert equihgnn_amd.get_float32_matmul_precision_panels() is False and precision.panel_products() == 6
    equihgnn_amd.set_float32_matmul_precision("medium")
    assert precision.products() == 1 and precision.panel_products() == 6
    for mode, products in MODES.items():
        equihgnn_amd.set_float32_matmul_precision(mode, panels=True)
        assert equihgnn_amd.get_float32_matmul_precision() == mode and equihgnn_amd.get_float32_matmul_precision_panels() is True
        assert precision.panel_products() == products == precision.products()
    equihgnn_amd.set_float32_matmul_precision("medium")                    # a later plain call resets it
    assert equihgnn_amd.get_float32_matmul_precision_panels() is False and precision.panel_products() == 6
    equihgnn_amd.set_float32_matmul_precision("high", panels=True)
    with pytest.raises(ValueError):
        equihgnn_amd.set_float32_matmul_precision("low", panels=True)
    assert equihgnn_amd.get_float32_matmul_precision() == "high" and precision.panel_products() == 3


def test_backward_as_forward_pins_the_count_for_the_call_and_puts_the_earlier_one_back():
    import types
    import equihgnn_amd
    from equihgnn_amd.ops import panel
    seen = []

    @panel.backward_as_forward
    def inner(ctx, fail=False):
        seen.append((panel._products(), panel.panel_planes(), panel._products(6)))
        if fail:
            raise RuntimeError("boom")

    @panel.backward_as_forward
    def outer(ctx):
        seen.append(panel._products())
        inner(types.SimpleNamespace(products=3))
        seen.append(panel._products())

    equihgnn_amd.set_float32_matmul_precision("high", panels=True)
    outer(types.SimpleNamespace(products=1))
    assert seen == [1, (3, 2, 6), 1] and panel._products() == 3
    equihgnn_amd.set_float32_matmul_precision("highest")
    with pytest.raises(RuntimeError):
        inner(types.SimpleNamespace(products=1), True)
    assert seen[-1] == (1, 1, 6) and panel._products() == 6 and getattr(panel._PIN, "products", None) is None


def test_trainer_keys_its_graphs_by_the_flag():
    import equihgnn_amd
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    b = synth_batch(2, 1)
    keys = set()
    for mode in MODES:
        for panels in (False, True):
            equihgnn_amd.set_float32_matmul_precision(mode, panels=panels)
            key = GraphedTrainStep._key(b)
            assert key[-1] == mode and key[-2] is panels
            keys.add(key)
    assert len(keys) == 6


def test_panel_entry_points_refuse_a_bad_product_count_and_too_few_planes():
    """argument validation without a device: `products` outside {6, 3, 1}, `planes` outside 1..3 or below what the products
    read are EQH_ERR_ARG before anything is launched (the pointers are never dereferenced)"""
    from equihgnn_amd import hip
    L = hip.lib()
    p = ctypes.c_void_p(4096)

    # (rows = 0: a call whose arguments are accepted answers EQH_OK without a launch -- the control of every refusal below)
    def plain(products, n_planes):
        return L.hg_panel_gemm_f32_p(p, 64, 0, 64, p, 1.0, None, 0, 0.0, None, 0, p, 64, products, n_planes, None)

    def stream(products, n_planes):
        return L.hg_panel_stream_gemm_f32_p(p, 128, 0, 128, 128, p, 1.0, None, 0, 0.0, None, 0, p, 128, products, n_planes, None)

    def conv(products, n_planes):
        q = hip.HgConvPanel()
        q.rows, q.C, q.products, q.planes = 0, 64, products, n_planes
        return L.hg_conv_panel(hip.HG_CONV_F2, q, None)

    def multi(products, n_planes):
        q = hip.HgPanelMulti()
        q.a, q.lda, q.rows, q.C, q.n, q.products, q.planes = 4096, 64, 0, 64, 1, products, n_planes
        q.w[0], q.out[0], q.ldo[0] = 4096, 4096, 64
        return L.hg_panel_multi(ctypes.byref(q), None)

    def psum(products, n_planes):
        q = hip.HgPanelSum()
        q.rows, q.C, q.n, q.out, q.ldo, q.products, q.planes = 0, 64, 1, 4096, 64, products, n_planes
        q.a[0], q.lda[0], q.w[0] = 4096, 64, 4096
        return L.hg_panel_sum(ctypes.byref(q), None)

    for name, call in (("plain", plain), ("stream", stream), ("conv", conv), ("multi", multi), ("sum", psum)):
        for products, n_planes in ((0, 0), (6, 3), (6, 0), (3, 2), (3, 3), (3, 0), (1, 1), (1, 2), (1, 3), (1, 0)):
            assert call(products, n_planes) == hip.EQH_OK, (name, products, n_planes)
        for products in (2, 4, 5, 7, -1, 12):
            assert call(products, 3) == hip.EQH_ERR_ARG, (name, products)
        for products, n_planes in ((6, 2), (6, 1), (0, 2), (3, 1), (1, 4), (3, -1)):
            assert call(products, n_planes) == hip.EQH_ERR_ARG, (name, products, n_planes)
    # the pack: planes outside 0..3, and a k_major image (the x6 kernel's pre-split operand) of fewer than three
    for n_planes, k_major in ((4, 0), (-1, 0), (2, 1), (1, 1)):
        it = (hip.HgPanelPack * 1)()
        it[0].w, it[0].ld, it[0].dst, it[0].K, it[0].N, it[0].trans = 4096, 64, 4096, 64, 64, 1
        it[0].planes, it[0].k_major = n_planes, k_major
        assert L.hg_panel_pack(1, it, None) == hip.EQH_ERR_ARG, (n_planes, k_major)
    assert L.hg_panel_pack_bytes_p(64, 64, 3) == L.hg_panel_pack_bytes(64, 64) == 64 * 64 * 6
    assert L.hg_panel_pack_bytes_p(64, 64, 2) == 64 * 64 * 4 and L.hg_panel_pack_bytes_p(64, 64, 1) == 64 * 64 * 2
    assert L.hg_panel_pack_bytes_p(64, 64, 0) == 0 and L.hg_panel_pack_bytes_p(64, 64, 4) == 0


@pytest.mark.parametrize("name", ["egnn_equihnns_c64", "mhnnm_c64_eval"])
def test_model_tolerances_are_the_measured_ones(name):
    """repeats the measurement behind MODEL_DEV on the oracle (CPU): the constants are what the reference side gives"""
    case = load_case(name)
    model = build_case_model(case).eval()
    data = batch_from_case(case)
    ref = case["out"].astype(np.float64)
    with torch.no_grad():
        assert_close(model(data).numpy(), ref, 1e-5, "the oracle in eval mode gives the fixture")
        for mode in REDUCED:
            with truncated_linears(PLANES[MODES[mode]]):
                out = model(data).numpy().astype(np.float64)
            dev = float((np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max())
            print(f"{name} {mode}: oracle with truncated Linear operands deviates {dev:.3e} (recorded {MODEL_DEV[name, mode]:.3e})")
            assert MODEL_DEV[name, mode] / 1.5 <= dev <= MODEL_DEV[name, mode] * 1.5


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the operators
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_case(rows, C):
    g = torch.Generator(device=DEV).manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, device=DEV, generator=g)
    w = torch.randn(C, C, device=DEV, generator=g) * C ** -0.5
    bias = torch.randn(C, device=DEV, generator=g)
    return x, w, bias


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_plain_product_computes_exactly_the_terms_of_its_mode(rows, C):
    """hg_panel_gemm_f32_p: x W^T and x W^T + bias -> ReLU under each mode against the float64 model of that mode's planes and
    terms, at the bounds of test_panel_gemm_matches_float64 (4e-7 of sum |a||b|; rtol = atol = 1e-5 with the epilogue); the
    distance from the plain float64 product within the truncation bound; a packed image of exactly the planes and the
    three-plane image give the same bits; a second run gives the same bits"""
    from equihgnn_amd import ops
    x, w, bias = _plain_case(rows, C)
    full = x.double() @ w.double().t()
    scale = x.abs().double() @ w.abs().double().t()
    acc = C * 2.0 ** -23 * scale
    models = {m: prod(x, w.t(), PLANES[MODES[m]]) for m in MODES}
    for mode in MODES:
        def run():
            (img,) = pack([(w, True)])
            return ops.panel_gemm(x, img, C), ops.panel_gemm(x, img, C, bias=bias, relu=True), img
        got, got_act, img = under(mode, True, run)
        P = PLANES[MODES[mode]]
        assert img.numel() == C * C * 2 * P
        err = ((got.double() - models[mode]).abs() / scale).max().item()
        err_full = ((got.double() - full).abs() / scale).max().item()
        print(f"plain rows={rows} C={C} {mode}: |C - C_P| {err:.3e} (bound 4e-7), |C - A.B| {err_full:.3e} "
              f"(bound {TRUNC[P] + C * 2.0 ** -23:.3e}) of |A|.|B|")
        assert err < 4e-7, (mode, err)
        assert torch.allclose(got_act.double(), torch.relu(models[mode] + bias.double()), rtol=1e-5, atol=1e-5), mode
        assert bool(((got.double() - full).abs() <= TRUNC[P] * scale + acc).all()), (mode, err_full)
        if mode != "highest":       # the model of this mode is told apart from the full product by the same bound
            assert ((models[mode] - full).abs() / scale).max().item() > 8e-7, mode
            assert not torch.allclose(torch.relu(models[mode] + bias.double()), torch.relu(full + bias.double()), rtol=1e-5, atol=1e-5)
        # the three-plane image serves every mode, bit for bit; and a second run repeats the first
        (img3,) = ops.panel_pack([(w, True)], planes=3)
        assert torch.equal(under(mode, True, lambda: ops.panel_gemm(x, img3, C)), got), mode
        assert torch.equal(under(mode, True, lambda: ops.panel_gemm(x, img, C, products=MODES[mode])), got), mode
    # an image with fewer planes than the products read is refused
    (img1,) = ops.panel_pack([(w, True)], planes=1)
    with pytest.raises(Exception, match="hg_panel_gemm_f32_p"):
        ops.panel_gemm(x, img1, C, products=3)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", [(70, 64), (33, 256)])
def test_six_products_are_the_present_path_and_the_flag_is_off_by_default(rows, C):
    """("highest", panels=True) and ("medium", panels=False) are bitwise the plain call: plain, multi, summed and conv products"""
    from equihgnn_amd import hip, ops
    x, w, bias = _plain_case(rows, C)

    def run():
        img_t, img_n = pack([(w, True), (w, False)])
        a = ops.panel_gemm(x, img_t, C, bias=bias, relu=True)
        b = torch.empty_like(x)
        ops.panel_sum([(x, img_n), (a, img_t)], C, b)
        c = torch.empty_like(x)
        ops.panel_multi(x, C, [(img_t, bias, None, a, c)])
        h1, h1n, pa = (torch.empty_like(x) for _ in range(3))
        ops.conv_panel(hip.HG_CONV_F1, rows, C, DEV, in0=x, w0=img_t, w1=img_n, b0=bias, g0=bias, be0=bias, out0=h1, out1=h1n, out2=pa)
        return a, b, c, h1, h1n, pa

    base = under("highest", False, run)
    for mode, panels in (("highest", True), ("medium", False), ("high", False)):
        for got, want in zip(under(mode, panels, run), base):
            assert torch.equal(got, want), (mode, panels)
    moved = under("medium", True, run)
    assert not torch.equal(moved[0], base[0]) and not torch.equal(moved[3], base[3])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_multi_and_summed_products_compute_the_terms_of_their_mode(rows, C):
    """hg_panel_multi (three weight streams over one A image) and hg_panel_sum (three A images) under each mode against the
    float64 model, at test_panel_sum_matches_float64's bound of 4e-7 of sum |a||w|"""
    from equihgnn_amd import ops
    g = torch.Generator(device=DEV).manual_seed(rows * 11 + C)
    a = [torch.randn(rows, C, device=DEV, generator=g) for _ in range(3)]
    w = [torch.randn(C, C, device=DEV, generator=g) * C ** -0.5 for _ in range(3)]
    scale_sum = sum(ai.abs().double() @ wi.abs().double() for ai, wi in zip(a, w))
    for mode in MODES:
        P = PLANES[MODES[mode]]

        def run():
            imgs = pack([(wi, False) for wi in w])
            out = torch.empty(rows, C, device=DEV)
            ops.panel_sum(list(zip(a, imgs)), C, out)
            outs = [torch.empty(rows, C, device=DEV) for _ in range(3)]
            ops.panel_multi(a[0], C, [(img, None, None, None, o) for img, o in zip(imgs, outs)])
            return out, outs
        out, outs = under(mode, True, run)
        want = sum(prod(ai, wi, P) for ai, wi in zip(a, w))
        assert ((out.double() - want).abs() / scale_sum).max().item() < 4e-7, mode
        for o, wi in zip(outs, w):
            sc = a[0].abs().double() @ wi.abs().double()
            assert ((o.double() - prod(a[0], wi, P)).abs() / sc).max().item() < 4e-7, mode
        again, _ = under(mode, True, run)
        assert torch.equal(again, out), mode


def _conv_case(C, n_nodes, n_he, seed):
    from equihgnn_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *sh, s=1.0: torch.randn(*sh, device=DEV, generator=g) * s
    nnz = int(2.2 * n_nodes)
    v = torch.randint(0, n_nodes, (nnz,), device=DEV, generator=g)
    e = torch.randint(0, n_he, (nnz,), device=DEV, generator=g)
    by_e, by_v = ops.csr_build(e, v, n_he), ops.csr_build(v, e, n_nodes)
    Pm = dict(W1a=rn(C, C, s=C ** -0.5), W2v=rn(C, C, s=C ** -0.5), w12=rn(C, C, s=C ** -0.5), w23=rn(C, C, s=C ** -0.5),
              W3b=rn(C, C, s=C ** -0.5), b1a=rn(C, s=0.3), g1=1 + rn(C, s=0.2), be1=rn(C, s=0.2), b12=rn(C, s=0.3),
              b3a=rn(C, s=0.3), g3=1 + rn(C, s=0.2), be3=rn(C, s=0.2), b3b=rn(C, s=0.3))
    return Pm, rn(n_nodes, C), rn(n_nodes, C, s=0.5), rn(n_nodes, C), v, e, by_e, by_v


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_conv_forward_stages_compute_the_terms_of_their_mode(rows, C):
    """HG_CONV_F1 (two products of one A image), F2 (a gathered mean in front of the product) and F3 with the chained F1 tail
    (four products, a LayerNorm between the first two) under each mode against the float64 model of the mode, link by link from
    the kernel's own intermediate rows, at the tolerances of test_conv_panel_forward_stages_match_float64"""
    from equihgnn_amd import hip, ops
    n_he = rows + 5
    Pm, X, cw, s, v, e, by_e, by_v = _conv_case(C, rows, n_he, 11 + rows + C)
    d = lambda t: t.double()
    new = lambda r: torch.empty(r, C, device=DEV)
    runs = {}
    for mode in MODES:
        P = PLANES[MODES[mode]]
        pr = lambda a, name: prod(a, Pm[name].t(), P)

        def run():
            iW1a, iW2v, iw12, iw23, iW3b = pack([(Pm[k], True) for k in ("W1a", "W2v", "w12", "w23", "W3b")])
            h1, h1n, pa = new(rows), new(rows), new(rows)
            ops.conv_panel(hip.HG_CONV_F1, rows, C, DEV, in0=X, w0=iW1a, w1=iW2v, b0=Pm["b1a"], g0=Pm["g1"], be0=Pm["be1"],
                           out0=h1, out1=h1n, out2=pa)
            hbar, qb = new(n_he), new(n_he)
            ops.conv_panel(hip.HG_CONV_F2, n_he, C, DEV, in0=h1n, rowptr=by_e.rowptr, col=by_e.col, w0=iw12, bias_out=Pm["b12"],
                           out0=hbar, out1=qb)
            u, x3, xn, h1b, h1nb, pab = (new(rows) for _ in range(6))
            ops.conv_panel(hip.HG_CONV_F3, rows, C, DEV, scale=0.5, relu=True, tail=True, in0=s, in1=cw, w0=iw23, b0=Pm["b3a"],
                           g0=Pm["g3"], be0=Pm["be3"], w1=iW3b, bias_out=Pm["b3b"], out0=u, out1=x3, out2=xn, w2=iW1a, w3=iW2v,
                           b1=Pm["b1a"], g1=Pm["g1"], be1=Pm["be1"], out3=h1b, out4=h1nb, out5=pab)
            return h1, h1n, pa, hbar, qb, u, x3, xn, h1b, h1nb, pab
        out = runs[mode] = under(mode, True, run)
        h1, h1n, pa, hbar, qb, u, x3, xn, h1b, h1nb, pab = out
        t5, t25 = dict(rtol=1e-5, atol=1e-5), dict(rtol=1e-5, atol=2e-5)
        assert torch.allclose(d(h1), pr(X, "W1a"), **t5) and torch.allclose(d(pa), pr(X, "W2v"), **t5), mode
        assert torch.allclose(d(h1n), ln64(torch.relu(d(h1) + d(Pm["b1a"])), d(Pm["g1"]), d(Pm["be1"])), rtol=1e-4, atol=2e-5), mode
        assert torch.allclose(d(qb), pr(hbar, "w12") + d(Pm["b12"]), **t25), mode
        assert torch.allclose(d(u), 0.5 * pr(s, "w23") + d(cw), **t5), mode
        assert torch.allclose(d(x3), ln64(torch.relu(d(u) + d(Pm["b3a"])), d(Pm["g3"]), d(Pm["be3"])), rtol=1e-4, atol=2e-5), mode
        assert torch.allclose(d(xn), torch.relu(pr(x3, "W3b") + d(Pm["b3b"])), **t25), mode
        assert torch.allclose(d(h1b), pr(xn, "W1a"), **t25) and torch.allclose(d(pab), pr(xn, "W2v"), **t25), mode
        if mode != "highest":       # ... which the full product misses: the mode dropped its planes
            assert not torch.allclose(d(h1), d(X) @ d(Pm["W1a"]).t(), **t5), mode
            assert not torch.allclose(d(xn), torch.relu(d(x3) @ d(Pm["W3b"]).t() + d(Pm["b3b"])), **t25), mode
        for a, b in zip(under(mode, True, run), out):
            assert torch.equal(a, b), mode
    for a, b in zip(under("medium", False, run), runs["highest"]):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_conv_backward_stages_compute_the_terms_of_their_mode(rows, C):
    """HG_CONV_B3 (dx3 = g W3b, LayerNorm backward, ds = scale dpre w23) and HG_CONV_B1 with B2 folded in and the chained B3
    tail (five products; the stacked [W1a ; W2v] image of K = 2 C) under each mode: the products against the float64 model of the
    mode from the kernel's own rows (rtol = atol = 2e-4, test_conv_panel_backward_stages_match_autograd_float64's), the chained
    tail bitwise equal to the stage on its own, and every result the same bits on a second run"""
    from equihgnn_amd import hip, ops
    n_he = rows + 5
    Pm, X, cw, s, v, e, by_e, by_v = _conv_case(C, rows, n_he, 12 + rows + C)
    d = lambda t: t.double()
    new = lambda r: torch.empty(r, C, device=DEV)
    g_ = torch.Generator(device=DEV).manual_seed(3)
    rn = lambda r: torch.randn(r, C, device=DEV, generator=g_)
    dxn, xprev, dqb, dpa, h1 = rn(rows), rn(rows), rn(n_he), rn(rows), rn(rows)
    u = (0.5 * (s @ Pm["w23"].t()) + cw).contiguous()
    ew = ops.entry_weights(by_v, by_e)
    tol = dict(rtol=2e-4, atol=2e-4)
    base = None
    for mode in MODES:
        P = PLANES[MODES[mode]]

        def run():
            iW3b_n, iw23_n, iw12_n = pack([(Pm["W3b"], False), (Pm["w23"], False), (Pm["w12"], False)])
            (istack,) = pack([[(Pm["W1a"], False), (Pm["W2v"], False)]])
            gout, dpre, ds, acc, vec = new(rows), new(rows), new(rows), new(rows), torch.zeros(3, C, device=DEV)
            ops.conv_panel(hip.HG_CONV_B3, rows, C, DEV, scale=0.5, acc_first=True, in0=dxn, in1=xprev, w0=iW3b_n, w1=iw23_n, in2=u,
                           b0=Pm["b3a"], g0=Pm["g3"], out0=gout, out1=dpre, out2=ds, acc_out=acc, slab=ops.conv_panel_slab(rows, C, DEV),
                           dbias=vec[0], dgamma=vec[1], dbeta=vec[2])
            dh1, dX, g2, dpre2, ds2, acc2 = (new(rows) for _ in range(6))
            vec1, vec3 = torch.zeros(3, C, device=DEV), torch.zeros(3, C, device=DEV)
            ops.conv_panel(hip.HG_CONV_B1, rows, C, DEV, scale=0.5, tail=True, acc_first=True, in0=dqb, w3=iw12_n, rowptr=by_v.rowptr,
                           col=by_v.col, wq=ew, in1=h1, b0=Pm["b1a"], g0=Pm["g1"], in2=dpa, w0=istack, out0=dh1, out1=dX,
                           slab=ops.conv_panel_slab(rows, C, DEV), dbias=vec1[0], dgamma=vec1[1], dbeta=vec1[2], in3=xprev, w1=iW3b_n,
                           w2=iw23_n, out5=u, b1=Pm["b3a"], g1=Pm["g3"], out2=g2, out3=dpre2, out4=ds2, acc_out=acc2,
                           slab2=ops.conv_panel_slab(rows, C, DEV), dbias2=vec3[0], dgamma2=vec3[1], dbeta2=vec3[2])
            gr, dprer, dsr, vr = new(rows), new(rows), new(rows), torch.zeros(3, C, device=DEV)
            ops.conv_panel(hip.HG_CONV_B3, rows, C, DEV, scale=0.5, acc_first=True, in0=dX, in1=xprev, w0=iW3b_n, w1=iw23_n, in2=u,
                           b0=Pm["b3a"], g0=Pm["g3"], out0=gr, out1=dprer, out2=dsr, acc_out=new(rows),
                           slab=ops.conv_panel_slab(rows, C, DEV), dbias=vr[0], dgamma=vr[1], dbeta=vr[2])
            return gout, dpre, ds, vec, dh1, dX, g2, dpre2, ds2, vec1, vec3, gr, dprer, dsr, vr
        out = under(mode, True, run)
        gout, dpre, ds, vec, dh1, dX, g2, dpre2, ds2, vec1, vec3, gr, dprer, dsr, vr = out
        assert torch.equal(gout, dxn * (xprev > 0))
        # B3's second product from its own dpre; B1's stacked product from its own dh1 and dpa
        assert torch.allclose(d(ds), 0.5 * prod(dpre, Pm["w23"], P), **tol), mode
        assert torch.allclose(d(dX), prod(torch.cat((dh1, dpa), 1), torch.cat((Pm["W1a"], Pm["W2v"]), 0), P), **tol), mode
        assert torch.allclose(d(ds2), 0.5 * prod(dpre2, Pm["w23"], P), **tol), mode
        # B3's first product feeds the LayerNorm backward: dpre against float64 autograd over the model's dx3
        ub = (d(u) + d(Pm["b3a"])).requires_grad_()
        ln64(torch.relu(ub), d(Pm["g3"]), d(Pm["be3"])).backward(prod(gout, Pm["W3b"], P))
        assert torch.allclose(d(dpre), ub.grad, **tol), mode
        assert torch.equal(g2, gr) and torch.equal(dpre2, dprer) and torch.equal(ds2, dsr) and torch.equal(vec3, vr), mode
        assert all(bool(torch.isfinite(t).all()) for t in out)
        for a, b in zip(under(mode, True, run), out):
            assert torch.equal(a, b), mode
        if mode == "highest":
            base = out
        else:
            assert not torch.equal(ds, base[2]) and not torch.equal(dX, base[5]), mode
    for a, b in zip(under("medium", False, run), base):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_egnn_node_stages_compute_the_terms_of_their_mode(rows, C):
    """HG_EGNN_NODE_F / _B (K = C + 16 and K = 2 C images, the C + 16 output columns of the backward stage) under each mode
    against the float64 model of the mode from the kernel's own rows, at test_egnn_node_panel_stages_match_float64's tolerances"""
    from equihgnn_amd import hip, ops
    g = torch.Generator(device=DEV).manual_seed(C + rows)
    rn = lambda *sh, s=1.0: torch.randn(*sh, device=DEV, generator=g) * s
    d = lambda t: t.double()
    normed, m_i, feats, dout = rn(rows, C), rn(rows, 16), rn(rows, C), rn(rows, C)
    w0, b0 = rn(2 * C, C + 16, s=(C + 16) ** -0.5), rn(2 * C, s=0.3)
    w3, b3 = rn(C, 2 * C, s=(2 * C) ** -0.5), rn(C, s=0.3)
    base = None
    for mode in MODES:
        P = PLANES[MODES[mode]]

        def run():
            imgs = pack([(w0[:C], True), (w0[C:], True), (w3, True), (w3[:, :C], False), (w3[:, C:], False), (w0, False, C + 32)])
            node_in, hpre, hid, out = (torch.empty(rows, k, device=DEV) for k in (C + 16, 2 * C, 2 * C, C))
            ops.conv_panel(hip.HG_EGNN_NODE_F, rows, C, DEV, in0=normed, in1=m_i, in2=feats, w0=imgs[0], w1=imgs[1], w2=imgs[2], b0=b0,
                           bias_out=b3, out0=node_in, out1=hpre, out2=hid, out3=out)
            dpre, dnode_in = torch.empty(rows, 2 * C, device=DEV), torch.empty(rows, C + 16, device=DEV)
            ops.conv_panel(hip.HG_EGNN_NODE_B, rows, C, DEV, in0=dout, ld0=C, in1=hpre, w0=imgs[3], w1=imgs[4], w2=imgs[5], out0=dpre,
                           out1=dnode_in)
            return node_in, hpre, hid, out, dpre, dnode_in
        res = under(mode, True, run)
        node_in, hpre, hid, out, dpre, dnode_in = res
        assert torch.equal(node_in, torch.cat((normed, m_i), -1))
        assert torch.allclose(d(hpre), prod(node_in, w0.t(), P) + d(b0), rtol=1e-5, atol=1e-5), mode
        assert torch.allclose(d(hid), torch.nn.functional.silu(d(hpre)), rtol=1e-5, atol=1e-5), mode
        assert torch.allclose(d(out), prod(hid, w3.t(), P) + d(b3) + d(feats), rtol=1e-5, atol=2e-5), mode
        h64 = d(hpre).requires_grad_()
        torch.nn.functional.silu(h64).backward(prod(dout, w3, P))
        assert torch.allclose(d(dpre), h64.grad, rtol=1e-4, atol=1e-5), mode
        assert torch.allclose(d(dnode_in), prod(dpre, w0, P), rtol=1e-4, atol=2e-5), mode
        for a, b in zip(under(mode, True, run), res):
            assert torch.equal(a, b), mode
        if mode == "highest":
            base = res
        else:
            assert not torch.allclose(d(hpre), d(node_in) @ d(w0).t() + d(b0), rtol=1e-5, atol=1e-5), mode
    for a, b in zip(under("medium", False, run), base):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(64, 128), (256, 256)])
def test_streamed_product_computes_the_terms_of_its_mode(K, N):
    """hg_panel_stream_gemm_f32_p (persistent workgroups, two A images) on 70 rows, bias + ReLU: the float64 model of each mode
    at rtol = atol = 1e-5 (test_panel_stream_gemm_matches_float64's), the flag off bitwise the six-product call"""
    from equihgnn_amd import ops
    g = torch.Generator(device=DEV).manual_seed(K + N)
    x = torch.randn(70, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
    bias = torch.randn(N, device=DEV, generator=g)
    run = lambda: ops.panel_stream_gemm(x, w, True, bias=bias, relu=True)
    outs = {}
    for mode in MODES:
        outs[mode] = under(mode, True, run)
        want = torch.relu(prod(x, w.t(), PLANES[MODES[mode]]) + bias.double())
        assert torch.allclose(outs[mode].double(), want, rtol=1e-5, atol=1e-5), mode
        assert torch.equal(under(mode, True, run), outs[mode])
    assert torch.equal(under("medium", False, run), outs["highest"])
    assert not torch.equal(outs["medium"], outs["highest"]) and not torch.equal(outs["high"], outs["highest"])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", SHAPES)
def test_egnn_node_stages_with_the_layer_norm_inside_compute_the_terms_of_their_mode(rows, C):
    """HG_EGNN_NODE_F / _B in the form the model uses (g0 given: normed = LayerNorm(feats) formed inside, the residual is feats;
    backward: d feats = LayerNorm backward of d normed + dout, d m_i, the slab sums of d gamma / d beta) under each mode against
    the float64 model of the mode from the kernel's own rows: the product links at the tolerances of
    test_egnn_node_panel_stages_match_float64, the LayerNorm links at those of the conv stages' (rtol 1e-4 / atol 2e-5 forward,
    rtol = atol = 2e-4 backward, 1e-3 of the largest entry for the vector gradients)"""
    from equihgnn_amd import hip, ops
    g = torch.Generator(device=DEV).manual_seed(3 * C + rows)
    rn = lambda *sh, s=1.0: torch.randn(*sh, device=DEV, generator=g) * s
    d = lambda t: t.double()
    feats, m_i, dout = rn(rows, C), rn(rows, 16), rn(rows, C)
    gam, bet = 1 + rn(C, s=0.2), rn(C, s=0.2)
    w0, b0 = rn(2 * C, C + 16, s=(C + 16) ** -0.5), rn(2 * C, s=0.3)
    w3, b3 = rn(C, 2 * C, s=(2 * C) ** -0.5), rn(C, s=0.3)
    base = None
    for mode in MODES:
        P = PLANES[MODES[mode]]

        def run():
            imgs = pack([(w0[:C], True), (w0[C:], True), (w3, True), (w3[:, :C], False), (w3[:, C:], False), (w0, False, C + 32)])
            node_in, hpre, hid, out = (torch.empty(rows, k, device=DEV) for k in (C + 16, 2 * C, 2 * C, C))
            ops.conv_panel(hip.HG_EGNN_NODE_F, rows, C, DEV, eps=1e-5, in0=feats, in1=m_i, w0=imgs[0], w1=imgs[1], w2=imgs[2], b0=b0,
                           bias_out=b3, g0=gam, be0=bet, out0=node_in, out1=hpre, out2=hid, out3=out)
            dpre, dfeats, dm = torch.empty(rows, 2 * C, device=DEV), torch.empty(rows, C, device=DEV), torch.empty(rows, 16, device=DEV)
            vec = torch.zeros(3, C, device=DEV)
            ops.conv_panel(hip.HG_EGNN_NODE_B, rows, C, DEV, eps=1e-5, in0=dout, ld0=C, in1=hpre, w0=imgs[3], w1=imgs[4], w2=imgs[5],
                           out0=dpre, out1=dfeats, out2=dm, in3=feats, g0=gam, slab=ops.conv_panel_slab(rows, C, DEV), dbias=vec[0],
                           dgamma=vec[1], dbeta=vec[2])
            return node_in, hpre, hid, out, dpre, dfeats, dm, vec[1:].clone()
        res = under(mode, True, run)
        node_in, hpre, hid, out, dpre, dfeats, dm, vec = res
        f64, g64, b64 = d(feats).requires_grad_(), d(gam).requires_grad_(), d(bet).requires_grad_()
        normed64 = ln64(f64, g64, b64)
        assert torch.allclose(d(node_in[:, :C]), normed64.detach(), rtol=1e-4, atol=2e-5) and torch.equal(node_in[:, C:], m_i), mode
        assert torch.allclose(d(hpre), prod(node_in, w0.t(), P) + d(b0), rtol=1e-5, atol=1e-5), mode
        assert torch.allclose(d(out), prod(hid, w3.t(), P) + d(b3) + d(feats), rtol=1e-5, atol=2e-5), mode
        h64 = d(hpre).requires_grad_()
        torch.nn.functional.silu(h64).backward(prod(dout, w3, P))
        assert torch.allclose(d(dpre), h64.grad, rtol=1e-4, atol=1e-5), mode
        dnode = prod(dpre, w0, P)                                     # [d normed | d m_i] of the mode, from the kernel's own dpre
        assert torch.allclose(d(dm), dnode[:, C:], rtol=1e-4, atol=2e-5), mode
        normed64.backward(dnode[:, :C])
        assert torch.allclose(d(dfeats), f64.grad + d(dout), rtol=2e-4, atol=2e-4), mode
        for got, want in ((vec[0], g64.grad), (vec[1], b64.grad)):
            assert torch.allclose(d(got), want, rtol=1e-3, atol=1e-3 * float(want.abs().max())), mode
        for a, b in zip(under(mode, True, run), res):
            assert torch.equal(a, b), mode
        if mode == "highest":
            base = res
        else:
            assert not torch.allclose(d(hpre), d(node_in) @ d(w0).t() + d(b0), rtol=1e-5, atol=1e-5), mode
            assert not torch.equal(dfeats, base[5]) and not torch.equal(dm, base[6]), mode
    for a, b in zip(under("medium", False, run), base):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_the_planes_of_an_image_are_read_from_its_size():
    """a clone of an image is the image (nothing rides beside the tensor); images of different plane counts in one call, and a
    buffer that is no whole image, are refused on the host"""
    from equihgnn_amd import hip, ops
    C = 64
    x, w, bias = _plain_case(33, C)
    (img1,) = ops.panel_pack([(w, True)], planes=1)
    (img3,) = ops.panel_pack([(w, True)])
    assert img3.numel() == C * C * 6 and img1.numel() == C * C * 2 and ops.panel_pack_bytes([(w, True)]) == C * C * 6
    want = ops.panel_gemm(x, img1, C, products=1)
    assert torch.equal(ops.panel_gemm(x, img1.clone(), C, products=1), want)
    assert torch.equal(ops.panel_gemm(x, img3[:].contiguous(), C, products=1), want)
    out = torch.empty_like(x)
    with pytest.raises(ValueError, match="same number of planes"):
        ops.panel_sum([(x, img1), (x, img3)], C, out)
    with pytest.raises(ValueError, match="same number of planes"):
        ops.conv_panel(hip.HG_CONV_F1, 33, C, DEV, in0=x, w0=img1, w1=img3, b0=bias, g0=bias, be0=bias, out0=out, out1=out, out2=out)
    with pytest.raises(ValueError, match="bf16 planes"):
        ops.panel_gemm(x, img3[:-16], C)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the autograd nodes (ops.merged_conv_stack, the EGNN node update, ops.mhnn_conv_panel) through the models that use them
# ---------------------------------------------------------------------------------------------------------------------------
_PANEL_ENTRIES = ("hg_conv_panel", "hg_panel_multi", "hg_panel_sum", "hg_panel_gemm_f32_p", "hg_panel_stream_gemm_f32_p")


class _Spy:
    """records (phase, entry point, stage, products, planes) of every panel launch and the planes of every pack, as the
    library receives them"""

    def __init__(self, monkeypatch):
        from equihgnn_amd import hip
        self.calls, self.packs, self.phase = [], [], "forward"
        L = hip.lib()
        for name in _PANEL_ENTRIES:
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))
        real_pack = L.hg_panel_pack

        def pack_(n, arr, stream):
            self.packs += [(self.phase, int(arr[i].planes)) for i in range(n)]
            return real_pack(n, arr, stream)
        monkeypatch.setattr(L, "hg_panel_pack", pack_)

    def _wrap(self, name, real):
        def call(*args):
            if name == "hg_conv_panel":
                rec = (int(args[0]), int(args[1].products), int(args[1].planes))
            elif name in ("hg_panel_multi", "hg_panel_sum"):
                rec = (0, int(args[0]._obj.products), int(args[0]._obj.planes))
            else:
                rec = (0, int(args[-3]), int(args[-2]))
            self.calls.append((self.phase, name) + rec)
            return real(*args)
        return call

    def take(self):
        out = (self.calls, self.packs)
        self.calls, self.packs, self.phase = [], [], "forward"
        return out


def _node_model(method):
    from common import fill_state_dict, zero_dropouts
    from equihgnn_amd import models
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.registry import default_args
    m = models.MODELS[method](1, default_args(method=method, MLP_hidden=64, output_hidden=32))
    fill_state_dict(m, 21)
    zero_dropouts(m)
    m.to(DEV).train()
    return m, synth_batch(24, 4321).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["egnn_equihnns", "mhnnm"])
def test_the_autograd_nodes_multiply_forward_and_backward_with_the_count_of_their_forward_pass(method, monkeypatch):
    """The model step that test_conv_stack_on_panel_kernels_matches_the_unfused_path drives (forward, MSE, backward: the merged
    conv stack and the EGNN node update of egnn_equihnns, the MHNNConv node of mhnnm, every parameter gradient), per mode with
    the flag.  What the library receives is recorded: EVERY panel launch of the forward AND the backward pass carries the
    mode's product count and images of exactly its planes, and the backward stages (B3, B1, the node update's) are among them
    -- each of those entry points with that count is held to the float64 model of the mode by the operator tests above.
    Six products are the earlier path bit for bit (output and every gradient), a second run repeats the first bit for bit,
    "medium" moves output and gradients further than "high".  The flag CHANGED between forward and backward (the word stays,
    so that products outside the panel kernels, which follow the word at call time, are the same): the backward launches still
    carry the forward's count and the gradients are bitwise those of the unchanged flag, both ways."""
    import equihgnn_amd
    from equihgnn_amd import hip
    model, b = _node_model(method)
    spy = _Spy(monkeypatch)
    backward_stages = {hip.HG_CONV_B3, hip.HG_CONV_B1, hip.HG_EGNN_NODE_B} if method == "egnn_equihnns" else {hip.HG_CONV_B3}

    def step(mode, panels, switch_to=None):
        for p in model.parameters():
            p.grad = None
        b._hyper_index = None
        equihgnn_amd.set_float32_matmul_precision(mode, panels=panels)
        try:
            out = model(b)
            loss = torch.nn.functional.mse_loss(out, b.y)
            if switch_to is not None:
                equihgnn_amd.set_float32_matmul_precision(*switch_to[:1], panels=switch_to[1])
            spy.phase = "backward"
            loss.backward()
            torch.cuda.synchronize()
        finally:
            equihgnn_amd.set_float32_matmul_precision("highest")
        calls, packs = spy.take()
        return out.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, calls, packs

    def same(x, y):
        return torch.equal(x[0], y[0]) and x[1].keys() == y[1].keys() and all(torch.equal(x[1][n], y[1][n]) for n in x[1])

    def check_calls(calls, packs, products):
        fwd = [c for c in calls if c[0] == "forward"]
        bwd = [c for c in calls if c[0] == "backward"]
        assert len(fwd) >= 4 and len(bwd) >= 4 and packs, (len(fwd), len(bwd), len(packs))
        assert backward_stages <= {c[2] for c in bwd if c[1] == "hg_conv_panel"}
        for c in calls:
            assert c[3:] == (products, PLANES[products]), c
        assert {p for _, p in packs} == {PLANES[products]} and all(ph == "forward" for ph, _ in packs)

    base = step("highest", False)
    check_calls(base[2], base[3], 6)
    assert len(base[1]) > 10
    runs = {}
    for mode in MODES:
        runs[mode] = r = step(mode, True)
        check_calls(r[2], r[3], MODES[mode])
        assert all(bool(torch.isfinite(g).all()) for g in r[1].values())
        assert same(step(mode, True), r), f"{mode}: a second run differs"
    assert same(runs["highest"], base)
    off = {}
    for mode in REDUCED:                             # the word without the flag: six products in every panel launch
        off[mode] = step(mode, False)
        check_calls(off[mode][2], off[mode][3], 6)
        assert not same(off[mode], runs[mode]), f"{mode}: the flag does not reach the nodes"
    dev = {m: (float((runs[m][0] - base[0]).abs().max()),
               max(float((runs[m][1][n] - base[1][n]).abs().max() / base[1][n].abs().max().clamp(min=1e-30)) for n in base[1]))
           for m in REDUCED}
    print(f"{method}: output / gradient (of each parameter's largest entry) moved by {dev}")
    assert 0.0 < dev["high"][0] < dev["medium"][0] and 0.0 < dev["high"][1] < dev["medium"][1]
    # the flag changes between the forward and the backward pass
    for mode in REDUCED:
        r = step(mode, True, switch_to=(mode, False))
        check_calls(r[2], r[3], MODES[mode])
        assert same(r, runs[mode]), mode
        r = step(mode, False, switch_to=(mode, True))
        check_calls(r[2], r[3], 6)
        assert same(r, off[mode]), mode


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the models
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["egnn_equihnns_c64", "mhnnm_c64_eval"])
def test_model_forward_with_the_panels_under_the_reduced_modes(name, monkeypatch):
    """eval-mode forward of a hidden-64 golden case whose conv products run on the panel kernels (every other eligible product on
    the x6 kernel: X6_MIN_OUTPUTS = 0, as the oracle's truncation takes every F.linear): ("highest", panels) keeps the 1e-5
    parity, "high" and "medium" move the output, "medium" further, both within 4 x the reference side's deviation; with the
    flag off the panel products do not move (the output differs from the one with the flag on)"""
    import equihgnn_amd
    from equihgnn_amd import models
    from equihgnn_amd.ops import products as P
    monkeypatch.setattr(P, "X6_MIN_OUTPUTS", 0)
    case = load_case(name)
    model = build_case_model(case, models.MODELS).eval().to(DEV)
    data = batch_from_case(case).to(DEV)
    ref = case["out"].astype(np.float64)

    def forward(mode, panels):
        equihgnn_amd.set_float32_matmul_precision(mode, panels=panels)
        if hasattr(data, "_hyper_index"):
            data._hyper_index = None
        with torch.no_grad():
            return model(data).cpu().numpy().astype(np.float64)
    outs = {mode: forward(mode, True) for mode in MODES}
    assert_close(outs["highest"], ref, 1e-5, "highest + panels")
    assert np.array_equal(outs["highest"], forward("highest", False))
    for mode in REDUCED:
        moved = float(np.abs(outs[mode] - outs["highest"]).max())
        dev = float((np.abs(outs[mode] - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(f"{name} {mode} + panels: differs from highest by {moved:.3e}, from the fixture by {dev:.3e} (tolerance {MODEL_TOL[name, mode]:.3e})")
        assert moved > 0.0, f"{mode}: the output is the one of highest -- the mode is not engaged"
        assert dev <= MODEL_TOL[name, mode], (mode, dev)
        assert not np.array_equal(outs[mode], forward(mode, False)), f"{mode}: the flag does not reach the panel kernels"
    assert np.abs(outs["medium"] - outs["highest"]).max() > np.abs(outs["high"] - outs["highest"]).max()


@pytest.mark.gpu
def test_training_recaptures_when_the_flag_changes_and_replays_the_old_graph_when_it_goes_back(monkeypatch):
    """GraphedTrainStep on egnn_equihnns hidden 64: two steps, two under ("medium", panels=True), two after switching back --
    two captures for the bucket with slot keys that differ in the flag, finite gradients, and the replay after switching back
    bitwise the replay before (same weights, same batch: the first graph, not the arithmetic of the second)"""
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
    raw = synth_batch(8, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 8
    tr = GraphedTrainStep(model, lr=0.0, keep_grads=True)       # lr 0: the weights stay, so equal graphs give equal bits
    tr.index_prefetch = False
    captures = []
    real = tr._capture
    monkeypatch.setattr(tr, "_capture", lambda static: (captures.append(
        (equihgnn_amd.get_float32_matmul_precision(), equihgnn_amd.get_float32_matmul_precision_panels())), real(static))[1])

    def snap():
        torch.cuda.synchronize()
        return [p.grad.clone() for p in model.parameters() if p.grad is not None]
    equihgnn_amd.set_float32_matmul_precision("highest")
    losses = [float(tr.step(batch)) for _ in range(3)]            # bootstrap, capture, replay
    before = (losses[-1], snap())
    assert captures == [("highest", False)] and len(tr.slots) == 1
    equihgnn_amd.set_float32_matmul_precision("medium", panels=True)
    losses += [float(tr.step(batch)) for _ in range(2)]            # capture under the flag, replay
    medium = (losses[-1], snap())
    assert captures == [("highest", False), ("medium", True)] and len(tr.slots) == 2
    assert sorted((k[-1], k[-2]) for k in tr.slots) == [("highest", False), ("medium", True)]
    assert len(medium[1]) > 10 and all(bool(torch.isfinite(g).all()) for g in medium[1])
    assert any(float(g.abs().max()) > 0 for g in medium[1])
    assert any(not torch.equal(a, b) for a, b in zip(medium[1], before[1])), "the step under the flag is the step without it"
    equihgnn_amd.set_float32_matmul_precision("highest")
    losses += [float(tr.step(batch)) for _ in range(2)]            # the first graph again: nothing new
    after = (losses[-1], snap())
    assert captures == [("highest", False), ("medium", True)] and len(tr.slots) == 2
    assert after[0] == before[0] and all(torch.equal(a, b) for a, b in zip(after[1], before[1]))
    assert all(np.isfinite(losses)), losses
