"""Training dropout on the MHNNConv panel kernels (the DROP forms of HG_CONV_F3 / HG_CONV_B3, hg_conv_panel_drop; csrc/panel.hip,
ops/panel.py, ops/mhnn_panel.py): the stages against float64, the element a decision belongs to, bit for bit, the product
counts, and the layer / the models with an active dropout on the panel path.

The keep matrix of a site is what ``ops.dropout_add(ones[R, C], None, p, seed)`` returns, as in tests/test_hip_conv_dropout.py;
expectations are float64 torch with that matrix multiplied in behind ``layer_norm``.  Tolerances are those of the p = 0 test of
the same stage in tests/test_hip_kernels.py (test_conv_f3_incidence_prologue_matches_float64_and_the_separate_launch,
test_conv_panel_forward_stages_match_float64, test_conv_panel_backward_stages_match_autograd_float64) with the absolute part
times 1 / (1 - p): every kept value and its gradient carries that factor.

Shapes (C, output rows, source rows): 70 rows are three panels, the last of 6 rows; 33 rows put one row into the second panel.
The incidence lists give the output rows 0, 1, 2, 3 and 5 incidences in turn (2.2 per row; the prologue walks two at a time) and
are shuffled, so the CSR's perm is not the identity."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, make_batch  # noqa: E402
from test_hip_conv_dropout import P, _check_layer, _keep, _mlp64, _model, _pool_draws, _seed  # noqa: E402
from test_matmul_precision import PLANES, TRUNC, planes  # noqa: E402

from oracle import ref_models as O  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional
SHAPES = [(64, 70, 33), (128, 33, 70), (256, 70, 70)]


def _ops():
    from equihgnn_amd import ops
    return ops


def _keep1(rows, C, p, seed):
    return _keep(rows, C, p, seed) if p > 0 else torch.ones(rows, C, dtype=torch.float64)


def _ln64(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


@functools.lru_cache(maxsize=None)
def _case(C, rows, src, one_each=False):
    """Operands of one F3 / B3 stage over ``rows`` output rows that gather from ``src`` source rows (host tensors, fp32) and
    the incidence lists (o: output row, c: source row of every incidence, in shuffled order).  ``one_each``: exactly one
    incidence per output row."""
    g = torch.Generator().manual_seed(1000 * C + 10 * rows + src)
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g) * s
    deg = torch.ones(rows, dtype=torch.long) if one_each else torch.tensor([0, 1, 2, 3, 5])[torch.arange(rows) % 5]
    o = torch.repeat_interleave(torch.arange(rows), deg)
    o = o[torch.randperm(o.numel(), generator=g)]
    c = torch.randint(0, src, (o.numel(),), generator=g)
    t = dict(own=rn(rows, C), oth=rn(src, C), g_inc=1 + rn(C, s=0.2), be_inc=rn(C, s=0.2), cw=rn(rows, C, s=0.5),
             w23=rn(C, C, s=C ** -0.5), W3b=rn(C, C, s=C ** -0.5), b3a=rn(C, s=0.3), g3=1 + rn(C, s=0.2), be3=rn(C, s=0.2),
             b3b=rn(C, s=0.3), dxn=rn(rows, C))
    return t, o, c


def _csr(o, c, rows):
    ops = _ops()
    csr = ops.csr_build(o.to(DEV), c.to(DEV), rows)
    assert not torch.equal(csr.perm.cpu().long(), torch.arange(o.numel())), "the shuffle must leave a perm that is not the identity"
    return csr


def _run_f3(C, rows, t, csr, p_inc, seed_inc, p, seed, products=None, img_planes=3, relu=True, **over):
    """HG_CONV_F3 with the incidence prologue on the device; returns (s, u, x3, xn) as host float64"""
    from equihgnn_amd import hip
    ops = _ops()
    dv = {k: v.to(DEV) for k, v in {**t, **over}.items()}
    iw23, iW3b = ops.panel_pack([(dv["w23"], True), (dv["W3b"], True)], planes=img_planes)
    s, u, x3, xn = (torch.empty(rows, C, device=DEV) for _ in range(4))
    kw = {} if p_inc is None else dict(drop=(p_inc, seed_inc, csr.perm, p, seed))
    ops.conv_panel(hip.HG_CONV_F3, rows, C, DEV, scale=0.5, relu=relu, tail=False, in0=dv["own"], in2=dv["oth"], rowptr=csr.rowptr,
                   col=csr.col, g_inc=dv["g_inc"], be_inc=dv["be_inc"], eps_inc=1e-5, out6=s, in1=dv["cw"], w0=iw23, b0=dv["b3a"],
                   g0=dv["g3"], be0=dv["be3"], w1=iW3b, bias_out=dv["b3b"], out0=u, out1=x3, out2=xn, products=products, **kw)
    torch.cuda.synchronize()
    return s, u, x3, xn


# ---------------------------------------------------------------------------------------------------------------------
# F3: both sites against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_inc,p", [(0.25, 0.25), (0.5, 0.0), (0.0, 0.5)])
@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_f3_with_both_dropout_sites_matches_float64(C, rows, src, p_inc, p):
    """s (masked per incidence, element perm[q] * C + c), u (unmasked), x3 (masked per row element, as stored) and Xn (the
    product of the masked x3), link by link from the kernel's own rows as the p = 0 tests do; at (0.25, 0.25) s also against
    hg_incidence_ln_reduce_drop_fwd_col under the same seed."""
    from equihgnn_amd import hip
    ops = _ops()
    t, o, c = _case(C, rows, src)
    cnt = torch.bincount(o, minlength=rows)
    for n in (0, 1, 2, 3):
        assert bool((cnt == n).any()), f"the case must hold a row with {n} incidences"
    assert bool((cnt >= 5).any())
    nnz = o.numel()
    assert abs(nnz / rows - 2.2) < 0.15
    csr = _csr(o, c, rows)
    seed_inc, seed = _seed(500 + C), _seed(600 + C)
    s, u, x3, xn = (x.double().cpu() for x in _run_f3(C, rows, t, csr, p_inc, seed_inc if p_inc > 0 else None, p, seed if p > 0 else None))
    d = {k: v.double() for k, v in t.items()}
    k_inc, k_row = _keep1(nnz, C, p_inc, seed_inc), _keep1(rows, C, p, seed)
    h = _ln64(torch.relu(d["own"][o] + d["oth"][c]), d["g_inc"], d["be_inc"]) * k_inc
    s64 = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, o, h) / cnt.clamp(min=1).double()[:, None]
    sc = 1.0 / (1.0 - max(p_inc, p))
    err = lambda a, b: float((a - b).abs().max())
    print(f"F3 C={C} rows={rows} p_inc={p_inc} p={p}: |s - s64| {err(s, s64):.2e}")
    assert torch.allclose(s, s64, rtol=1e-5, atol=1e-5 * sc)
    assert float(s[cnt == 0].abs().max()) == 0.0                       # a row without incidences gives 0
    u64 = 0.5 * (s @ d["w23"].t()) + d["cw"]
    x3_64 = _ln64(torch.relu(u + d["b3a"]), d["g3"], d["be3"]) * k_row
    xn64 = torch.relu(x3 @ d["W3b"].t() + d["b3b"])
    print(f"   |u - u64| {err(u, u64):.2e}  |x3 - x3_64| {err(x3, x3_64):.2e}  |xn - xn64| {err(xn, xn64):.2e}")
    assert torch.allclose(u, u64, rtol=1e-5, atol=1e-5 * sc)
    assert torch.allclose(x3, x3_64, rtol=1e-4, atol=2e-5 * sc)
    if p > 0:
        assert bool(((x3 == 0) == (k_row == 0)).all())                 # the stored x3 is the masked one
    assert torch.allclose(xn, xn64, rtol=1e-5, atol=2e-5 * sc)
    if (p_inc, p) == (0.25, 0.25):
        s_sep = torch.empty(rows, C, device=DEV)
        own, oth, gi, bi = (t[k].to(DEV) for k in ("own", "oth", "g_inc", "be_inc"))
        hip.check(hip.lib().hg_incidence_ln_reduce_drop_fwd_col(
            ops._ptr(own), ops._ptr(oth), ops._ptr(csr.rowptr), ops._ptr(csr.col), ops._ptr(csr.perm), 1, ops._ptr(gi), ops._ptr(bi),
            rows, C, 1, 1e-5, p_inc, ops._ptr(seed_inc), ops._ptr(s_sep), ops._stream(torch.device(DEV))), "drop_fwd_col")
        print(f"   |s - s_sep| {err(s, s_sep.double().cpu()):.2e}")
        assert torch.allclose(s, s_sep.double().cpu(), rtol=1e-5, atol=2e-6 / (1.0 - p_inc))


# ---------------------------------------------------------------------------------------------------------------------
# which element a decision belongs to, bit for bit; seeds; p = 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("products", [6, 3, 1])
@pytest.mark.parametrize("C", [64, 256])
def test_zero_gamma_and_unit_beta_return_the_keep_matrix_bit_for_bit(C, products):
    """g0 = 0, be0 = 1: the stored x3 IS the keep matrix of [rows, C] (element row * C + c), under every product count (images
    of as many planes as the count reads).  Xn = keep W3b^T + b3b then stays within the bound the header states for the count,
    applied to sum |a||b| (3 2^-14 for three products, 2 2^-7 + 2^-14 for one, nothing for six), plus the fp32 accumulation
    of C terms and the bias addition, (C + 2) 2^-23 of sum |a||b| + |b3b|."""
    ops = _ops()
    rows, src, p = 70, 70, 0.25
    t, o, c = _case(C, rows, src)
    csr = _csr(o, c, rows)
    seed = _seed(41 + C)
    z, one = torch.zeros(C), torch.ones(C)
    s, u, x3, xn = _run_f3(C, rows, t, csr, 0.0, None, p, seed, products=products, img_planes=PLANES[products], relu=False, g3=z, be3=one)
    keep = ops.dropout_add(torch.ones(rows, C, device=DEV), None, p, seed)
    assert torch.equal(x3, keep)
    assert sorted(set(x3.unique().tolist())) == [0.0, float(np.float32(1.0) / np.float32(1.0 - p))]
    W, b = t["W3b"].double(), t["b3b"].double()
    full = keep.double().cpu() @ W.t() + b
    scale = keep.double().cpu().abs() @ W.abs().t()
    bound = TRUNC[PLANES[products]] * scale + (C + 2) * 2.0 ** -23 * (scale + b.abs())
    dev = (xn.double().cpu() - full).abs()
    print(f"C={C} products={products}: |Xn - keep W^T - b| / bound {float((dev / bound).max()):.3f}")
    assert bool((dev <= bound).all())


@pytest.mark.parametrize("C", [64, 256])
def test_one_incidence_per_row_returns_the_keep_row_of_its_position_in_the_lists(C):
    """g_inc = 0, be_inc = 1 and exactly one incidence per output row, in shuffled order: out6[r] is the keep row of that
    incidence's position in the ORIGINAL lists (element perm[q] * C + c), exactly."""
    ops = _ops()
    rows, src, p_inc = 70, 33, 0.25
    t, o, c = _case(C, rows, src, True)
    assert sorted(o.tolist()) == list(range(rows)) and o.tolist() != list(range(rows))
    csr = _csr(o, c, rows)
    seed_inc = _seed(43 + C)
    s = _run_f3(C, rows, t, csr, p_inc, seed_inc, 0.0, None, g_inc=torch.zeros(C), be_inc=torch.ones(C))[0]
    keep = ops.dropout_add(torch.ones(rows, C, device=DEV), None, p_inc, seed_inc)       # row i: the incidence at position i
    assert torch.equal(s[o.to(DEV)], keep)
    assert 0.0 < float((s == 0).float().mean()) < 1.0


def test_same_seed_repeats_bit_for_bit_another_seed_does_not_and_zero_probabilities_are_the_plain_call():
    C, rows, src = 128, 33, 70
    t, o, c = _case(C, rows, src)
    csr = _csr(o, c, rows)
    a = _run_f3(C, rows, t, csr, 0.25, _seed(5), 0.25, _seed(6))
    b = _run_f3(C, rows, t, csr, 0.25, _seed(5), 0.25, _seed(6))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    other = _run_f3(C, rows, t, csr, 0.25, _seed(5), 0.25, _seed(7))
    assert torch.equal(other[0], a[0]) and not torch.equal(other[2], a[2])
    assert not torch.equal(_run_f3(C, rows, t, csr, 0.25, _seed(8), 0.25, _seed(6))[0], a[0])
    plain = _run_f3(C, rows, t, csr, None, None, None, None)
    for x, y in zip(_run_f3(C, rows, t, csr, 0.0, None, 0.0, None), plain):
        assert torch.equal(x, y)
    assert not torch.equal(plain[2], a[2])


# ---------------------------------------------------------------------------------------------------------------------
# B3
# ---------------------------------------------------------------------------------------------------------------------
def _run_b3(C, rows, t, u, xn, p, seed, products=None, img_planes=3):
    from equihgnn_amd import hip
    ops = _ops()
    dv = {k: v.to(DEV) for k, v in t.items()}
    iW3b_n, iw23_n = ops.panel_pack([(dv["W3b"], False), (dv["w23"], False)], planes=img_planes)
    gout, dpre, ds = (torch.empty(rows, C, device=DEV) for _ in range(3))
    acc, vec = torch.ones(rows, C, device=DEV), torch.zeros(3, C, device=DEV)
    ops.conv_panel(hip.HG_CONV_B3, rows, C, DEV, scale=0.5, acc_first=False, in0=dv["dxn"], in1=xn, w0=iW3b_n, w1=iw23_n,
                   in2=u, b0=dv["b3a"], g0=dv["g3"], out0=gout if xn is not None else None, out1=dpre, out2=ds, acc_out=acc,
                   slab=ops.conv_panel_slab(rows, C, DEV), dbias=vec[0], dgamma=vec[1], dbeta=vec[2], products=products,
                   drop=(0.0, None, None, p, seed))
    torch.cuda.synchronize()
    return gout, dpre, ds, acc, vec


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_b3_with_dropout_matches_float64_autograd(C, rows, src, masked):
    """Xn = act(keep . LN(relu(u + b)) W^T + b'), u = scale s w23^T + cw, act = ReLU through the in1 mask or the identity: ds,
    dpre (= d cw), acc_out and the three vector gradients."""
    p, seed = 0.25, _seed(700 + C)
    t, _, _ = _case(C, rows, src)
    d = {k: v.double() for k, v in t.items()}
    keep = _keep(rows, C, p, seed)
    leaves = {k: d[k].clone().requires_grad_() for k in ("b3a", "g3", "be3")}
    s64, cw64 = d["own"].clone().requires_grad_(), d["cw"].clone().requires_grad_()
    u64 = 0.5 * (s64 @ d["w23"].t()) + cw64
    x3_64 = _ln64(torch.relu(u64 + leaves["b3a"]), leaves["g3"], leaves["be3"]) * keep
    xn64 = x3_64 @ d["W3b"].t() + d["b3b"]
    if masked:
        xn64 = torch.relu(xn64)
    xn64.backward(d["dxn"])
    u, xn = u64.detach().float().contiguous().to(DEV), xn64.detach().float().contiguous().to(DEV)
    gout, dpre, ds, acc, vec = (x.double().cpu() for x in _run_b3(C, rows, t, u, xn if masked else None, p, seed))
    sc = 1.0 / (1.0 - p)
    tol = dict(rtol=2e-4, atol=2e-4 * sc)
    err = lambda a, b: float((a - b).abs().max())
    print(f"B3 C={C} rows={rows} masked={masked}: ds {err(ds, s64.grad):.2e} dpre {err(dpre, cw64.grad):.2e}")
    if masked:
        assert torch.equal(gout, d["dxn"] * (xn64.detach() > 0))
    assert torch.allclose(ds, s64.grad, **tol)
    assert torch.allclose(dpre, cw64.grad, **tol) and torch.allclose(acc, 1 + cw64.grad, **tol)
    for i, k in enumerate(("b3a", "g3", "be3")):
        gmax = float(leaves[k].grad.abs().max())
        print(f"   d{k}: {err(vec[i], leaves[k].grad) / gmax:.2e} of the largest entry")
        assert torch.allclose(vec[i], leaves[k].grad, rtol=1e-3, atol=1e-3 * gmax), k


def _prod(a, b, n_planes):
    """sum_{i + j < n_planes} a_i @ b_j in float64: the terms a product count keeps (tests/test_panel_precision.py)"""
    pa, pb = [x.double() for x in planes(a, n_planes)], [x.double() for x in planes(b.contiguous(), n_planes)]
    return sum(pa[i] @ pb[j] for i in range(n_planes) for j in range(n_planes - i))


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("C", [64, 256])
def test_b3_with_dropout_under_three_and_one_products(C, products):
    """The DROP forms of the reduced product counts: g = dXn [Xn > 0] exactly; dpre against float64 autograd of the masked
    LayerNorm over the count's own dx3 = P(g, W3b) at the p = 0 tolerance times 1 / (1 - p); ds = scale dpre w23 within the
    header's bound for the count applied to sum |a||b| (plus the accumulation of C terms, C 2^-23 of it)."""
    rows, src, p, seed = 70, 70, 0.25, _seed(800 + C)
    n_pl = PLANES[products]
    t, _, _ = _case(C, rows, src)
    d = {k: v.double() for k, v in t.items()}
    u = (0.5 * (t["own"] @ t["w23"].t()) + t["cw"]).contiguous()
    xprev = t["oth"][:rows].contiguous()
    gout, dpre, ds, acc, vec = (x.cpu() for x in _run_b3(C, rows, t, u.to(DEV), xprev.to(DEV), p, seed, products=products, img_planes=n_pl))
    assert torch.equal(gout, t["dxn"] * (xprev > 0))
    keep = _keep(rows, C, p, seed)
    ub = (u.double() + d["b3a"]).requires_grad_()
    (_ln64(torch.relu(ub), d["g3"], d["be3"]) * keep).backward(_prod(gout, t["W3b"], n_pl))
    assert torch.allclose(dpre.double(), ub.grad, rtol=2e-4, atol=2e-4 / (1.0 - p))
    scale = dpre.double().abs() @ d["w23"].abs()
    bound = 0.5 * (TRUNC[n_pl] + (C + 1) * 2.0 ** -23) * scale
    dev = (ds.double() - 0.5 * (dpre.double() @ d["w23"])).abs()
    print(f"C={C} products={products}: |ds - scale dpre w23| / bound {float((dev / bound.clamp(min=1e-30)).max()):.3f}")
    assert bool((dev <= bound).all())


# ---------------------------------------------------------------------------------------------------------------------
# the layer and the models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 256])
def test_mhnn_conv_one_application_on_the_panel_path_matches_float64_and_the_row_kernels(C, monkeypatch):
    """conv.py:87-101 with four 2-layer MLPs and an active dropout: the seeds go W1 ([nnz, C]), W2 ([M, C]), W3 ([nnz, C]),
    W4 ([N, C]); the panel path runs (two F3 and two B3 launches that carry `drop`); with PANEL_DROPOUT off the row kernels
    make the same keep decisions under the same seeds."""
    from equihgnn_amd import hip
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import MHNNConv
    from equihgnn_amd.ops import mhnn_panel
    ops = _ops()
    conv = MHNNConv(C, 2, 2, 2, 2, aggr="mean", dropout=P, normalization="ln")
    fill_state_dict(conv, 17)
    conv.to(DEV).train()
    data = make_batch(11, 6).to(DEV)
    index = HyperIndex.from_batch(data)
    N, v, e = data.x.shape[0], data.edge_index0.cpu(), data.edge_index1.cpu()
    M, nnz = int(data.edge_attr.shape[0]), v.numel()
    g = torch.Generator().manual_seed(5)
    xh, eh = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    wx, we = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    calls = []
    real = mhnn_panel.conv_panel

    def counted(stage, *a, drop=None, **kw):
        if drop is not None and (drop[0] > 0 or drop[3] > 0):
            calls.append(stage)
        return real(stage, *a, drop=drop, **kw)
    monkeypatch.setattr(mhnn_panel, "conv_panel", counted)

    def run():
        for q in conv.parameters():
            q.grad = None
        draws = _pool_draws(78)
        x, ee = xh.to(DEV).requires_grad_(True), eh.to(DEV).requires_grad_(True)
        with ops.dropout_seeds(DEV, 64):
            xo, eo = conv(x, ee, index)
        ((xo * wx.to(DEV)).sum() + (eo * we.to(DEV)).sum()).backward()
        got = {n: q.grad.clone() for n, q in conv.named_parameters()}
        got["x"], got["e"] = x.grad, ee.grad
        return torch.cat((xo, eo)).detach(), got, draws

    out, got, draws = run()
    assert calls == [hip.HG_CONV_F3, hip.HG_CONV_F3, hip.HG_CONV_B3, hip.HG_CONV_B3], "the panel path must run under an active dropout"
    prm = {n: q.detach().cpu().double().requires_grad_(True) for n, q in conv.named_parameters()}
    keep = lambda i, rows: _keep(rows, C, P, draws[i:i + 1])
    X, E = xh.double().requires_grad_(True), eh.double().requires_grad_(True)
    me = O.segment_reduce(_mlp64(prm, "W1", torch.cat((X[v], E[e]), -1), keep(0, nnz)), e, M, "mean")
    E1 = _mlp64(prm, "W2", torch.cat((E, me), -1), keep(1, M))
    mv = O.segment_reduce(_mlp64(prm, "W3", torch.cat((X[v], E1[e]), -1), keep(2, nnz)), v, N, "mean")
    X1 = _mlp64(prm, "W4", torch.cat((X, mv), -1), keep(3, N))
    ((X1 * wx.double()).sum() + (E1 * we.double()).sum()).backward()
    ref = {n: q.grad for n, q in prm.items()}
    ref["x"], ref["e"] = X.grad, E.grad
    _check_layer(out, torch.cat((X1, E1)), got, ref)
    # the row kernels under the same seeds: the same keep decisions
    del calls[:]
    monkeypatch.setattr(ops, "PANEL_DROPOUT", False)
    out_rows, got_rows, _ = run()
    assert calls == []
    _check_layer(out_rows, out.cpu().double(), got_rows, {n: t.cpu().double() for n, t in got.items()})


def test_padding_leaves_the_masks_of_the_real_rows_where_they_were_on_the_panel_path():
    """mhnn (LayerNorm model, paired tail): masks are keyed by row * C + c / incidence position * C + c and batch.pad_batch
    appends its rows and its (null) incidences at the end, so under one seed the real molecules of a padded batch get the
    unpadded result (tolerances of test_padding_leaves_the_masks_of_the_real_rows_where_they_were)."""
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    m = _model("mhnn", P).train()
    b = synth_batch(12, 4242)
    p = pad_batch(b, *bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz, 64)).to(DEV)
    p.num_real_graphs = 12
    b = b.to(DEV)
    torch.manual_seed(9)
    out = m(b)
    F.mse_loss(out, b.y).backward()
    g0 = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
    for q in m.parameters():
        q.grad = None
    torch.manual_seed(9)
    outp = m(p)
    assert outp.shape[0] == 13
    F.mse_loss(outp[:12], p.y[:12]).backward()
    np.testing.assert_allclose(outp[:12].detach().cpu().numpy(), out.detach().cpu().numpy(), atol=2e-6, rtol=1e-6)
    gmax = max(float(g.abs().max()) for g in g0.values())
    for n, q in m.named_parameters():
        if n in g0:
            scale = max(float(g0[n].abs().max()), 1e-3 * gmax) + 1e-12
            assert float((q.grad - g0[n]).abs().max()) / scale < 1e-4, n


def test_graphed_mhnnm_steps_draw_new_seeds_per_replay_and_eval_is_the_eager_eval():
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedEvalStep, GraphedTrainStep
    m = _model("mhnnm", 0.1).train()
    raw = synth_batch(32, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 32
    tr = GraphedTrainStep(m, lr=0.0)        # the parameters stay put: the losses differ by their dropout draws alone
    tr.index_prefetch = False
    losses = [float(tr.step(batch)) for _ in range(5)]      # eager first step, capture, three replays
    print("mhnnm losses over replays with dropout 0.1:", losses)
    assert all(np.isfinite(losses)) and len(tr.slots) == 1
    assert len(set(losses[2:])) == 3, losses
    m.eval()
    with torch.no_grad():
        want = m(batch).clone()
    batch._hyper_index = None
    ev = GraphedEvalStep(m)
    for _ in range(2):
        torch.testing.assert_close(ev(batch)[:32], want[:32], rtol=1e-5, atol=1e-6)
    ev.close()
