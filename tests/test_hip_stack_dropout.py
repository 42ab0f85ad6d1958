"""Training dropout on the S-tail conv stack's panel kernels (the dropout forms of HG_CONV_F1 / HG_CONV_F3 with its F1 tail /
HG_CONV_B1 with and without its B3 tail, hg_conv_stack_drop; csrc/panel.hip, ops/panel.py, ops/conv_stack.py, layers.py,
models.py): the stages against float64, the element a decision belongs to, bit for bit, and the stack / the models with an active
dropout on the panel path.

The keep matrix of a site is what ``ops.dropout_add(ones[R, C], None, p, seed)`` returns, as in tests/test_hip_conv_dropout.py;
expectations are float64 torch.  Tolerances are those of the p = 0 test of the same stage in tests/test_hip_kernels.py
(test_conv_panel_forward_stages_match_float64, test_conv_f3_incidence_prologue_matches_float64_and_the_separate_launch,
test_conv_panel_backward_stages_match_autograd_float64) with the absolute part times 1 / (1 - p), p the largest probability of
the call, as tests/test_hip_panel_dropout.py has them.

Shapes are those of tests/test_hip_panel_dropout.py (its ``_case``): 70 rows are three panels, the last of 6 rows; 33 rows put one
row into the second panel; the incidence lists give the rows 0, 1, 2, 3 and 5 incidences in turn, shuffled.  An HG_CONV_F3 with
a tail runs chained with the next F1 or as two launches, whichever the library built for the shape
(hg_conv_stack_drop_f3_launches): the checks are the same."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, golden_args, make_batch  # noqa: E402
from test_hip_conv_dropout import P, _check_layer, _keep, _mlp64, _model, _pool_draws, _seed  # noqa: E402
from test_hip_panel_dropout import SHAPES, _case, _csr, _keep1, _ln64  # noqa: E402
from test_matmul_precision import PLANES, TRUNC, planes  # noqa: E402

from oracle import ref_models as O  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def _ops():
    from equihgnn_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _f1_weights(C):
    """W1a, W2v, b1a, gamma1, beta1 of the F1 / B1 stages and w12 of the folded B2 (host tensors, fp32)"""
    g = torch.Generator().manual_seed(77 + C)
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g) * s
    return dict(W1a=rn(C, C, s=C ** -0.5), W2v=rn(C, C, s=C ** -0.5), b1a=rn(C, s=0.3), g1=1 + rn(C, s=0.2), be1=rn(C, s=0.2),
                w12=rn(C, C, s=C ** -0.5))


def _err(a, b):
    return float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# F1
# ---------------------------------------------------------------------------------------------------------------------
def _run_f1(C, rows, x, w, p1, seed1, products=None, img_planes=3, sites=None, **over):
    from equihgnn_amd import hip
    ops = _ops()
    dv = {k: v.to(DEV) for k, v in {**w, **over}.items()}
    iW1a, iW2v = ops.panel_pack([(dv["W1a"], True), (dv["W2v"], True)], planes=img_planes)
    h1, h1n, pa = (torch.empty(rows, C, device=DEV) for _ in range(3))
    ops.conv_panel(hip.HG_CONV_F1, rows, C, DEV, in0=x.to(DEV), w0=iW1a, w1=iW2v, b0=dv["b1a"], g0=dv["g1"], be0=dv["be1"], out0=h1,
                   out1=h1n, out2=pa, products=products, stack_drop=dict(p1=p1, seed1=seed1, **(sites or {})))
    torch.cuda.synchronize()
    return h1, h1n, pa


@pytest.mark.parametrize("p1", [0.25, 0.5])
@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_f1_stores_the_masked_h1n_and_leaves_h1_and_pa_unmasked(C, rows, src, p1):
    t, _, _ = _case(C, rows, src)
    w = _f1_weights(C)
    seed1 = _seed(900 + C)
    h1, h1n, pa = (x.double().cpu() for x in _run_f1(C, rows, t["own"], w, p1, seed1))
    d = {k: v.double() for k, v in w.items()}
    x = t["own"].double()
    keep = _keep(rows, C, p1, seed1)
    sc = 1.0 / (1.0 - p1)
    h1n64 = _ln64(torch.relu(h1 + d["b1a"]), d["g1"], d["be1"]) * keep
    print(f"F1 C={C} rows={rows} p1={p1}: |h1| {_err(h1, x @ d['W1a'].t()):.2e} |pa| {_err(pa, x @ d['W2v'].t()):.2e} "
          f"|h1n| {_err(h1n, h1n64):.2e}")
    assert torch.allclose(h1, x @ d["W1a"].t(), rtol=1e-5, atol=1e-5)           # unmasked: the p = 0 tolerance itself
    assert torch.allclose(pa, x @ d["W2v"].t(), rtol=1e-5, atol=1e-5)
    assert torch.allclose(h1n, h1n64, rtol=1e-4, atol=2e-5 * sc)
    assert bool(((h1n == 0) == (keep == 0)).all())


@pytest.mark.parametrize("products", [6, 3, 1])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_f1_zero_gamma_and_unit_beta_return_the_keep_matrix_bit_for_bit(C, products):
    """g1 = 0, be1 = 1: the stored h1n IS the keep matrix of [rows, C] (element row * C + c), under every product count
    (images of as many planes as the count reads)."""
    ops = _ops()
    rows, p1 = 70, 0.25
    t, _, _ = _case(C, rows, 70)
    seed1 = _seed(910 + C)
    h1, h1n, pa = _run_f1(C, rows, t["own"], _f1_weights(C), p1, seed1, products=products, img_planes=PLANES[products],
                          g1=torch.zeros(C), be1=torch.ones(C))
    keep = ops.dropout_add(torch.ones(rows, C, device=DEV), None, p1, seed1)
    assert torch.equal(h1n, keep)
    assert sorted(set(h1n.unique().tolist())) == [0.0, float(np.float32(1.0) / np.float32(1.0 - p1))]


# ---------------------------------------------------------------------------------------------------------------------
# F3 with the next application's F1
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _plain_calls_through_the_new_entry():
    """While open, every hg_conv_panel call of ops.conv_panel is made as hg_conv_stack_drop(stage, args, <all zero>, stream):
    the C entry itself with every probability 0 (ops.conv_panel alone never calls it then).  Yields the list of stages so
    called."""
    from equihgnn_amd import hip
    L = hip.lib()
    plain, seen = L.hg_conv_panel, []

    def through(stage, a, stream):
        seen.append(stage)
        return L.hg_conv_stack_drop(stage, a, hip.HgConvStackDrop(), stream)
    L.hg_conv_panel = through
    try:
        yield seen
    finally:
        L.hg_conv_panel = plain


def _run_f3s(C, rows, t, w, csr, probs, seeds, tail=True, entry="stack", products=None, img_planes=3, **over):
    """HG_CONV_F3 with the incidence prologue and the F1 tail.  ``probs`` = (p_inc, p3, p_x, p1), ``seeds`` alike;
    ``entry``: "stack" (stack_drop), "panel" (hg_conv_panel_drop: no tail, p_inc / p3 only) or "plain".
    Returns (s, u, x3, xn, h1, h1n, pa) on the device."""
    from equihgnn_amd import hip
    ops = _ops()
    dv = {k: v.to(DEV) for k, v in {**t, **w, **over}.items()}
    iw23, iW3b, iW1a, iW2v = ops.panel_pack([(dv["w23"], True), (dv["W3b"], True), (dv["W1a"], True), (dv["W2v"], True)],
                                            planes=img_planes)
    s, u, x3, xn, h1, h1n, pa = (torch.zeros(rows, C, device=DEV) for _ in range(7))
    p_inc, p3, p_x, p1 = probs
    sd = lambda p, x: x if p > 0 else None
    kw = {}
    if entry == "stack":
        kw["stack_drop"] = dict(p_inc=p_inc, seed_inc=sd(p_inc, seeds[0]), perm=csr.perm, p3=p3, seed3=sd(p3, seeds[1]), p_x=p_x,
                                seed_x=sd(p_x, seeds[2]), p1=p1, seed1=sd(p1, seeds[3]))
    elif entry == "panel":
        kw["drop"] = (p_inc, sd(p_inc, seeds[0]), csr.perm, p3, sd(p3, seeds[1]))
    ops.conv_panel(hip.HG_CONV_F3, rows, C, DEV, scale=0.5, relu=True, tail=tail, in0=dv["own"], in2=dv["oth"], rowptr=csr.rowptr,
                   col=csr.col, g_inc=dv["g_inc"], be_inc=dv["be_inc"], eps_inc=1e-5, out6=s, in1=dv["cw"], w0=iw23, b0=dv["b3a"],
                   g0=dv["g3"], be0=dv["be3"], w1=iW3b, bias_out=dv["b3b"], out0=u, out1=x3, out2=xn, w2=iW1a, w3=iW2v,
                   b1=dv["b1a"], g1=dv["g1"], be1=dv["be1"], out3=h1, out4=h1n, out5=pa, products=products, **kw)
    torch.cuda.synchronize()
    return s, u, x3, xn, h1, h1n, pa


PROBS = [(0.25, 0.25, 0.25, 0.25), (0.5, 0.0, 0.0, 0.0), (0.0, 0.0, 0.5, 0.0), (0.0, 0.0, 0.0, 0.5)]


@pytest.mark.parametrize("probs", PROBS)
@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_f3_with_the_next_f1_matches_float64_link_by_link(C, rows, src, probs):
    """s (masked per incidence), u (unmasked), x3 (masked, as stored), Xn = keep_x . relu(x3 W3b^T + b3b) (as stored: the next
    application's input), the next h1 / pa (products of the MASKED Xn) and the masked next h1n, each from the kernel's own rows
    as the p = 0 tests do; s, u, x3 also against hg_conv_panel_drop's F3 under the same seeds."""
    t, o, c = _case(C, rows, src)
    w = _f1_weights(C)
    csr = _csr(o, c, rows)
    nnz, cnt = o.numel(), torch.bincount(o, minlength=rows)
    seeds = [_seed(1100 + 10 * i + C) for i in range(4)]          # four DIFFERENT seeds
    p_inc, p3, p_x, p1 = probs
    s, u, x3, xn, h1, h1n, pa = (x.double().cpu() for x in _run_f3s(C, rows, t, w, csr, probs, seeds))
    d = {k: v.double() for k, v in {**t, **w}.items()}
    k_inc, k3 = _keep1(nnz, C, p_inc, seeds[0]), _keep1(rows, C, p3, seeds[1])
    k_x, k1 = _keep1(rows, C, p_x, seeds[2]), _keep1(rows, C, p1, seeds[3])
    sc = 1.0 / (1.0 - max(probs))
    h = _ln64(torch.relu(d["own"][o] + d["oth"][c]), d["g_inc"], d["be_inc"]) * k_inc
    s64 = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, o, h) / cnt.clamp(min=1).double()[:, None]
    u64 = 0.5 * (s @ d["w23"].t()) + d["cw"]
    x3_64 = _ln64(torch.relu(u + d["b3a"]), d["g3"], d["be3"]) * k3
    xn64 = torch.relu(x3 @ d["W3b"].t() + d["b3b"]) * k_x
    h1n64 = _ln64(torch.relu(h1 + d["b1a"]), d["g1"], d["be1"]) * k1
    print(f"F3+F1 C={C} rows={rows} probs={probs}: |s| {_err(s, s64):.2e} |u| {_err(u, u64):.2e} |x3| {_err(x3, x3_64):.2e} "
          f"|xn| {_err(xn, xn64):.2e} |h1| {_err(h1, xn @ d['W1a'].t()):.2e} |pa| {_err(pa, xn @ d['W2v'].t()):.2e} "
          f"|h1n| {_err(h1n, h1n64):.2e}")
    assert torch.allclose(s, s64, rtol=1e-5, atol=1e-5 * sc)
    assert torch.allclose(u, u64, rtol=1e-5, atol=1e-5 * sc)
    assert torch.allclose(x3, x3_64, rtol=1e-4, atol=2e-5 * sc)
    assert torch.allclose(xn, xn64, rtol=1e-5, atol=2e-5 * sc)
    assert bool(((xn == 0) | (k_x != 0)).all())                      # (Xn == 0) contains (keep_x == 0)
    assert torch.allclose(h1, xn @ d["W1a"].t(), rtol=1e-5, atol=2e-5 * sc)          # products of the MASKED Xn
    assert torch.allclose(pa, xn @ d["W2v"].t(), rtol=1e-5, atol=2e-5 * sc)
    assert torch.allclose(h1n, h1n64, rtol=1e-4, atol=2e-5 * sc)
    if p3 > 0:
        assert bool(((x3 == 0) == (k3 == 0)).all())
    if p1 > 0:
        assert bool(((h1n == 0) == (k1 == 0)).all())
    # the existing dropout form of F3 (no tail) under the same seeds
    ref = [x.double().cpu() for x in _run_f3s(C, rows, t, w, csr, probs, seeds, tail=False, entry="panel")[:3]]
    for name, a, b in zip(("s", "u", "x3"), (s, u, x3), ref):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * sc), name
    if p_x > 0:
        # a bias so large that the ReLU zeroes nothing: the zeros of the stored Xn are the dropped elements, no others
        big = _run_f3s(C, rows, t, w, csr, probs, seeds, b3b=torch.full((C,), 100.0))[3].cpu()
        assert bool(((big == 0) == (k_x == 0)).all()) and 0.0 < float((big == 0).double().mean()) < 1.0


def test_f3_seeds_reach_their_own_site_and_what_lies_downstream_and_zero_probabilities_are_the_plain_call():
    C, rows, src = 128, 33, 70
    t, o, c = _case(C, rows, src)
    w = _f1_weights(C)
    csr = _csr(o, c, rows)
    probs = PROBS[0]
    seeds = [_seed(21 + i) for i in range(4)]
    base = _run_f3s(C, rows, t, w, csr, probs, seeds)
    for x, y in zip(base, _run_f3s(C, rows, t, w, csr, probs, seeds)):
        assert torch.equal(x, y)
    names = ("s", "u", "x3", "xn", "h1", "h1n", "pa")
    # site -> the outputs a new seed there must leave alone (everything upstream of the site, and its unmasked neighbours)
    untouched = {0: (), 1: ("s", "u"), 2: ("s", "u", "x3"), 3: ("s", "u", "x3", "xn", "h1", "pa")}
    changed = {0: "s", 1: "x3", 2: "xn", 3: "h1n"}
    for site in range(4):
        other = list(seeds)
        other[site] = _seed(99 + site)
        got = dict(zip(names, _run_f3s(C, rows, t, w, csr, probs, other)))
        for n, b in zip(names, base):
            if n in untouched[site]:
                assert torch.equal(got[n], b), (site, n)
        assert not torch.equal(got[changed[site]], dict(zip(names, base))[changed[site]]), site
        if site == 2:
            assert not torch.equal(got["h1"], base[4]) and not torch.equal(got["pa"], base[6])
    plain = _run_f3s(C, rows, t, w, csr, probs, seeds, entry="plain")
    assert not torch.equal(plain[2], base[2])
    for tail in (True, False):
        a = _run_f3s(C, rows, t, w, csr, (0.0, 0.0, 0.0, 0.0), seeds, tail=tail)         # (ops.conv_panel: the plain call itself)
        b = _run_f3s(C, rows, t, w, csr, probs, seeds, tail=tail, entry="plain")
        for n, x, y in zip(names, a, b):
            assert torch.equal(x, y), (tail, n)


@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_zero_probabilities_through_the_c_entry_itself_are_the_plain_call(C, rows, src):
    """hg_conv_stack_drop with an all-zero HgConvStackDrop, called directly (ops.conv_panel calls the entry only when a
    probability is not 0): F3 with and without its tail and F1, bit for bit the hg_conv_panel call.  Likewise when only a site
    the stage does not read is active: the W1 site on an F3 without a tail, the W3 / input sites on F1 -- no seed is asked
    for, nothing is masked."""
    from equihgnn_amd import hip
    t, o, c = _case(C, rows, src)
    w = _f1_weights(C)
    csr = _csr(o, c, rows)
    names = ("s", "u", "x3", "xn", "h1", "h1n", "pa")
    zero = (0.0, 0.0, 0.0, 0.0)
    for tail in (True, False):
        want = _run_f3s(C, rows, t, w, csr, zero, [None] * 4, tail=tail, entry="plain")
        with _plain_calls_through_the_new_entry() as seen:
            got = _run_f3s(C, rows, t, w, csr, zero, [None] * 4, tail=tail, entry="plain")
        assert seen == [hip.HG_CONV_F3]
        for n, x, y in zip(names, got, want):
            assert torch.equal(x, y), (tail, n)
        assert float(want[3].abs().max()) > 0 and (not tail or float(want[5].abs().max()) > 0)
    # a site the stage ignores: through ops.conv_panel, which calls the entry as soon as one probability is not 0
    want = _run_f3s(C, rows, t, w, csr, zero, [None] * 4, tail=False, entry="plain")
    got = _run_f3s(C, rows, t, w, csr, (0.0, 0.0, 0.0, 0.5), [None] * 4, tail=False)
    for n, x, y in zip(names, got, want):
        assert torch.equal(x, y), n
    f1 = _run_f1(C, rows, t["own"], w, 0.0, None)
    with _plain_calls_through_the_new_entry() as seen:
        f1_direct = _run_f1(C, rows, t["own"], w, 0.0, None)
    assert seen == [hip.HG_CONV_F1]
    f1_ignored = _run_f1(C, rows, t["own"], w, 0.0, None, sites=dict(p3=0.5, p_x=0.5))
    for x, y, z in zip(f1, f1_direct, f1_ignored):
        assert torch.equal(x, y) and torch.equal(x, z)


def _prod(a, b, n_planes):
    """sum_{i + j < n_planes} a_i @ b_j in float64: the terms a product count keeps (tests/test_hip_panel_dropout.py)"""
    pa, pb = [x.double() for x in planes(a, n_planes)], [x.double() for x in planes(b.contiguous(), n_planes)]
    return sum(pa[i] @ pb[j] for i in range(n_planes) for j in range(n_planes - i))


def _within(got, a, w_t, n_pl, K, lead=1.0, extra=None, more=0):
    """|got - lead (a @ w_t) - extra| within the header's bound for the count applied to lead sum |a||w| (TRUNC), plus the fp32
    accumulation of K terms and ``more`` + 2 further roundings (the scale, the addend) on lead sum |a||w| + |extra|: the
    bound of test_zero_gamma_and_unit_beta_return_the_keep_matrix_bit_for_bit.  Returns the largest deviation / bound."""
    full = lead * (a @ w_t)
    scale = lead * (a.abs() @ w_t.abs())
    tail = scale
    if extra is not None:
        full, tail = full + extra, scale + extra.abs()
    bound = TRUNC[n_pl] * scale + (K + 2 + more) * 2.0 ** -23 * tail
    dev = (got - full).abs()
    assert bool((dev <= bound).all()), float((dev / bound.clamp(min=1e-30)).max())
    return float((dev / bound.clamp(min=1e-30)).max())


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("C", [64, 256])
def test_f3_with_the_next_f1_under_three_and_one_products(C, products):
    """The stack's F3 with its tail at the reduced product counts (C = 256: the only width whose 6-product form runs
    unchained, so its chained forms are these).  Link by link from the kernel's own rows: the four products within the header's
    bound for the count, the rows between them (the prologue, the two LayerNorms and their masks, the input dropout on the
    stored Xn) at the tolerances of the 6-product test -- no product lies inside those links."""
    rows, src = 70, 70
    n_pl = PLANES[products]
    probs = PROBS[0]
    t, o, c = _case(C, rows, src)
    w = _f1_weights(C)
    csr = _csr(o, c, rows)
    nnz, cnt = o.numel(), torch.bincount(o, minlength=rows)
    seeds = [_seed(1700 + 10 * i + C) for i in range(4)]
    s, u, x3, xn, h1, h1n, pa = (x.double().cpu() for x in _run_f3s(C, rows, t, w, csr, probs, seeds, products=products,
                                                                     img_planes=n_pl))
    d = {k: v.double() for k, v in {**t, **w}.items()}
    k_inc, k3, k_x, k1 = (_keep(r, C, p, sd) for r, p, sd in zip((nnz, rows, rows, rows), probs, seeds))
    sc = 1.0 / (1.0 - max(probs))
    h = _ln64(torch.relu(d["own"][o] + d["oth"][c]), d["g_inc"], d["be_inc"]) * k_inc
    s64 = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, o, h) / cnt.clamp(min=1).double()[:, None]
    assert torch.allclose(s, s64, rtol=1e-5, atol=1e-5 * sc)
    r_u = _within(u, s, d["w23"].t(), n_pl, C, lead=0.5, extra=d["cw"])
    x3_64 = _ln64(torch.relu(u + d["b3a"]), d["g3"], d["be3"]) * k3
    assert torch.allclose(x3, x3_64, rtol=1e-4, atol=2e-5 * sc) and bool(((x3 == 0) == (k3 == 0)).all())
    # Xn = keep_x . relu(pre): where it is not zero it is keep_x . pre (one more rounding: the keep factor)
    kept = xn != 0
    assert bool((kept <= (k_x != 0)).all())
    pre = torch.where(kept, xn / k_x.clamp(min=1.0), torch.zeros_like(xn))
    full = x3 @ d["W3b"].t() + d["b3b"]
    scale = x3.abs() @ d["W3b"].abs().t()
    bound = TRUNC[n_pl] * scale + (C + 3) * 2.0 ** -23 * (scale + d["b3b"].abs())
    assert bool(((pre - full).abs() <= bound)[kept].all())
    assert bool((full <= bound)[~kept & (k_x != 0)].all())            # a kept zero: the ReLU's
    r_h1 = _within(h1, xn, d["W1a"].t(), n_pl, C)
    r_pa = _within(pa, xn, d["W2v"].t(), n_pl, C)
    h1n64 = _ln64(torch.relu(h1 + d["b1a"]), d["g1"], d["be1"]) * k1
    assert torch.allclose(h1n, h1n64, rtol=1e-4, atol=2e-5 * sc) and bool(((h1n == 0) == (k1 == 0)).all())
    print(f"F3+F1 C={C} products={products}: deviation / bound: u {r_u:.3f} h1 {r_h1:.3f} pa {r_pa:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# B1 with and without its B3 tail
# ---------------------------------------------------------------------------------------------------------------------
def _run_b1(C, rows, t, w, by_v, ew, dqb, dpa, h1, u, xn, probs, seeds, tail, products=None, img_planes=3):
    """HG_CONV_B1 (with the folded w12 product) through stack_drop; ``probs`` = (p1, p3, p_x), ``seeds`` = (seed1, seed3);
    h1, u, xn: the stored rows on the device.  Returns (dh1, dX, g, dpre, ds, acc_out [started at 1], vec1, vec3) on the device."""
    from equihgnn_amd import hip
    ops = _ops()
    p1, p3, p_x = probs
    dv = {k: v.to(DEV) for k, v in {**t, **w}.items()}
    iW3b_n, iw23_n, iw12_n = ops.panel_pack([(dv["W3b"], False), (dv["w23"], False), (dv["w12"], False)], planes=img_planes)
    (istack,) = ops.panel_pack([[(dv["W1a"], False), (dv["W2v"], False)]], planes=img_planes)
    new = lambda: torch.empty(rows, C, device=DEV)
    dh1, dX, gout, dpre, ds, acc = new(), new(), new(), new(), new(), torch.ones(rows, C, device=DEV)
    vec1, vec3 = torch.zeros(3, C, device=DEV), torch.zeros(3, C, device=DEV)
    ops.conv_panel(hip.HG_CONV_B1, rows, C, DEV, scale=0.5, tail=tail, acc_first=False, in0=dqb.to(DEV), w3=iw12_n,
                   rowptr=by_v.rowptr, col=by_v.col, wq=ew, in1=h1, b0=dv["b1a"], g0=dv["g1"], in2=dpa.to(DEV), w0=istack,
                   out0=dh1, out1=dX, slab=ops.conv_panel_slab(rows, C, DEV), dbias=vec1[0], dgamma=vec1[1], dbeta=vec1[2],
                   in3=xn, w1=iW3b_n, w2=iw23_n, out5=u, b1=dv["b3a"], g1=dv["g3"], out2=gout, out3=dpre, out4=ds, acc_out=acc,
                   slab2=ops.conv_panel_slab(rows, C, DEV), dbias2=vec3[0], dgamma2=vec3[1], dbeta2=vec3[2], products=products,
                   stack_drop=dict(p1=p1, seed1=seeds[0] if p1 > 0 else None, p3=p3, seed3=seeds[1] if p3 > 0 else None, p_x=p_x))
    torch.cuda.synchronize()
    return dh1, dX, gout, dpre, ds, acc, vec1, vec3


@pytest.mark.parametrize("probs", [(0.25, 0.25, 0.25), (0.5, 0.0, 0.5)])
@pytest.mark.parametrize("C,rows,src", SHAPES)
def test_b1_with_and_without_tail_matches_float64_autograd(C, rows, src, probs):
    """The chain dqb -> (gathered, w12) -> keep1 . LN1 backward -> [dh1 | dpa] . [W1a ; W2v] -> dX -> g = dX [Xn > 0] /
    (1 - p_x) -> keep3 . LN3 backward -> ds, as float64 autograd of the forward it belongs to: the application before stores
    Xn = keep_x . relu(keep3 . LN3(relu(u + b3a)) W3b^T + b3b), this one h1 = Xn W1a^T, h1n = keep1 . LN1(relu(h1 + b1a)),
    qb = mean_{v in e}(h1n) w12^T, pa = Xn W2v^T.  ``probs`` = (p1, p3, p_x)."""
    from equihgnn_amd import hip
    ops = _ops()
    p1, p3, p_x = probs
    t, o, c = _case(C, rows, src)          # o: node of an incidence, c: its hyperedge (src hyperedges)
    w = _f1_weights(C)
    d = {k: v.double() for k, v in {**t, **w}.items()}
    by_v, by_e = _csr(o, c, rows), ops.csr_build(c.to(DEV), o.to(DEV), src)
    g = torch.Generator().manual_seed(5 + C)
    dqb, dpa = torch.randn(src, C, generator=g), torch.randn(rows, C, generator=g)
    seed1, seed3, seed_x = _seed(1300 + C), _seed(1400 + C), _seed(1500 + C)
    k1, k3, kx = _keep1(rows, C, p1, seed1), _keep1(rows, C, p3, seed3), _keep1(rows, C, p_x, seed_x)
    lv = {k: d[k].clone().requires_grad_() for k in ("b1a", "g1", "be1", "b3a", "g3", "be3")}
    s64, cw64 = d["own"].clone().requires_grad_(), d["cw"].clone().requires_grad_()
    u64 = 0.5 * (s64 @ d["w23"].t()) + cw64
    x3_64 = _ln64(torch.relu(u64 + lv["b3a"]), lv["g3"], lv["be3"]) * k3
    pre64 = x3_64 @ d["W3b"].t() + d["b3b"]
    xn64 = torch.relu(pre64) * kx
    h1_64 = xn64 @ d["W1a"].t()
    h1n64 = _ln64(torch.relu(h1_64 + lv["b1a"]), lv["g1"], lv["be1"]) * k1
    deg_e = torch.bincount(c, minlength=src).clamp(min=1).double()
    hbar64 = torch.zeros(src, C, dtype=torch.float64).index_add(0, c, h1n64[o]) / deg_e[:, None]
    pa64 = xn64 @ d["W2v"].t()
    for x in (pre64, xn64, h1_64):
        x.retain_grad()
    (((hbar64 @ d["w12"].t()) * dqb.double()).sum() + (pa64 * dpa.double()).sum()).backward()

    ew = ops.entry_weights(by_v, by_e)
    h1, u, xn = (x.detach().float().contiguous().to(DEV) for x in (h1_64, u64, xn64))
    sc = 1.0 / (1.0 - max(probs))
    tol = dict(rtol=2e-4, atol=2e-4 * sc)
    kept = {}
    for tail in (False, True):
        dh1, dX, gout, dpre, ds, acc, vec1, vec3 = _run_b1(C, rows, t, w, by_v, ew, dqb, dpa, h1, u, xn, probs,
                                                           (seed1, seed3), tail)
        kept[tail] = dX.clone()
        dh1_, dX_ = dh1.double().cpu(), dX.double().cpu()
        print(f"B1 C={C} rows={rows} probs={probs} tail={tail}: dh1 {_err(dh1_, h1_64.grad):.2e} dX {_err(dX_, xn64.grad):.2e}")
        assert torch.allclose(dh1_, h1_64.grad, **tol)
        assert torch.allclose(dX_, xn64.grad, **tol)
        for i, k in enumerate(("b1a", "g1", "be1")):
            gmax = float(lv[k].grad.abs().max())
            print(f"   d{k}: {_err(vec1[i].double().cpu(), lv[k].grad) / gmax:.2e} of the largest entry")
            assert torch.allclose(vec1[i].double().cpu(), lv[k].grad, rtol=1e-3, atol=1e-3 * gmax), k
        if not tail:
            continue
        gout_, dpre_, ds_, acc_ = (x.double().cpu() for x in (gout, dpre, ds, acc))
        print(f"   g {_err(gout_, pre64.grad):.2e} dpre {_err(dpre_, cw64.grad):.2e} ds {_err(ds_, s64.grad):.2e}")
        assert torch.allclose(gout_, pre64.grad, **tol)
        assert torch.allclose(dpre_, cw64.grad, **tol) and torch.allclose(acc_, 1 + cw64.grad, **tol)
        assert torch.allclose(ds_, s64.grad, **tol)
        for i, k in enumerate(("b3a", "g3", "be3")):
            gmax = float(lv[k].grad.abs().max())
            print(f"   d{k}: {_err(vec3[i].double().cpu(), lv[k].grad) / gmax:.2e} of the largest entry")
            assert torch.allclose(vec3[i].double().cpu(), lv[k].grad, rtol=1e-3, atol=1e-3 * gmax), k
        # g exactly: the dX the kernel stored without the tail, the mask of the STORED Xn, fl(1 / (1 - p_x))
        assert torch.equal(kept[False], kept[True])
        inv = torch.tensor(np.float32(1.0) / np.float32(1.0 - p_x), device=DEV)
        assert torch.equal(gout, kept[False] * inv * (xn > 0))


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("C", [64, 256])
def test_b1_with_its_tail_under_three_and_one_products(C, products):
    """The dropout forms of B1 at the reduced product counts, with the chained B3, as
    test_b3_with_dropout_under_three_and_one_products has the lone B3: dh1 against float64 autograd of the masked LayerNorm 1
    over the count's own d h1n = P(gathered dqb, w12), dpre likewise over P(g, W3b), both at the p = 0 tolerance times
    1 / (1 - p); dX = [dh1 | dpa] [W1a ; W2v] and ds = scale dpre w23 from the kernel's own rows within the header's bound for
    the count; g exactly; the vector gradients to 1e-3 of their largest entry."""
    ops = _ops()
    rows, src = 70, 70
    n_pl = PLANES[products]
    probs = p1, p3, p_x = (0.25, 0.25, 0.25)
    t, o, c = _case(C, rows, src)
    w = _f1_weights(C)
    d = {k: v.double() for k, v in {**t, **w}.items()}
    by_v, by_e = _csr(o, c, rows), ops.csr_build(c.to(DEV), o.to(DEV), src)
    ew = ops.entry_weights(by_v, by_e)
    g = torch.Generator().manual_seed(6 + C)
    dqb, dpa = torch.randn(src, C, generator=g), torch.randn(rows, C, generator=g)
    seed1, seed3 = _seed(1800 + C), _seed(1900 + C)
    k1, k3 = _keep(rows, C, p1, seed1), _keep(rows, C, p3, seed3)
    # the stored rows of the forward pass: any will do, the stage reads nothing else of it
    h1 = (t["own"] @ w["W1a"].t()).contiguous()
    u = (0.5 * (t["own"] @ t["w23"].t()) + t["cw"]).contiguous()
    xn = (torch.relu(t["oth"][:rows]) * _keep(rows, C, p_x, _seed(2000 + C)).float()).contiguous()
    run = lambda tail: _run_b1(C, rows, t, w, by_v, ew, dqb, dpa, h1.to(DEV), u.to(DEV), xn.to(DEV), probs, (seed1, seed3), tail,
                               products=products, img_planes=n_pl)
    dX_lone = run(False)[1]
    dh1, dX, gout, dpre, ds, acc, vec1, vec3 = run(True)
    assert torch.equal(dX, dX_lone)
    inv = torch.tensor(np.float32(1.0) / np.float32(1.0 - p_x), device=DEV)
    assert torch.equal(gout, dX * inv * (xn.to(DEV) > 0)) and 0.0 < float((gout == 0).float().mean()) < 1.0
    dh1, dX, gout, dpre, ds, acc, vec1, vec3 = (x.cpu() for x in (dh1, dX, gout, dpre, ds, acc, vec1, vec3))
    sc = 1.0 / (1.0 - max(probs))
    tol = dict(rtol=2e-4, atol=2e-4 * sc)

    def ln_bwd(pre, bias, gamma, beta, keep, dy):
        """gradients of keep . LN(relu(pre + bias)) under dy, float64: (d pre, d bias, d gamma, d beta)"""
        lv = [x.double().clone().requires_grad_() for x in (pre, bias, gamma, beta)]
        (_ln64(torch.relu(lv[0] + lv[1]), lv[2], lv[3]) * keep).backward(dy)
        return [x.grad for x in lv]

    def vecs(got, want, names):
        for i, (k, ref) in enumerate(zip(names, want)):
            gmax = float(ref.abs().max())
            print(f"   d{k}: {_err(got[i].double(), ref) / gmax:.2e} of the largest entry")
            assert torch.allclose(got[i].double(), ref, rtol=1e-3, atol=1e-3 * gmax), k

    # B1: the mean over a node's hyperedges of dqb / |e| (the backward of the F2 gather), times w12 with the count's terms
    deg_e = torch.bincount(c, minlength=src).clamp(min=1).double()
    gathered = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, o, dqb.double()[c] / deg_e[c][:, None])
    want = ln_bwd(h1, w["b1a"], w["g1"], w["be1"], k1, _prod(gathered.float(), w["w12"], n_pl))
    print(f"B1 C={C} products={products}: dh1 {_err(dh1.double(), want[0]):.2e}")
    assert torch.allclose(dh1.double(), want[0], **tol)
    vecs(vec1, want[1:], ("b1a", "g1", "be1"))
    r_dx = _within(dX.double(), torch.cat((dh1, dpa), 1).double(), torch.cat((d["W1a"], d["W2v"]), 0), n_pl, 2 * C, more=-2)
    # its B3 tail
    want = ln_bwd(u, t["b3a"], t["g3"], t["be3"], k3, _prod(gout, t["W3b"], n_pl))
    print(f"   dpre {_err(dpre.double(), want[0]):.2e}")
    assert torch.allclose(dpre.double(), want[0], **tol)
    assert torch.allclose(acc.double(), 1 + dpre.double(), rtol=2.0 ** -23, atol=0.0)
    vecs(vec3, want[1:], ("b3a", "g3", "be3"))
    r_ds = _within(ds.double(), dpre.double(), d["w23"], n_pl, C, lead=0.5, more=-1)
    print(f"   deviation / bound: dX {r_dx:.3f} ds {r_ds:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# the stack
# ---------------------------------------------------------------------------------------------------------------------
def _mhnns(C, L, dropout=P):
    from equihgnn_amd import models
    m = models.MODELS["mhnns"](1, golden_args("mhnns", C, dropout=dropout, All_num_layers=L))
    fill_state_dict(m, 13)
    return m.to(DEV)


def _count_stack_calls(monkeypatch):
    """Every conv_panel call of the stack: (stage, tail, with an active stack_drop), and the row operators that must not run"""
    from equihgnn_amd.ops import conv_stack
    ops = _ops()
    calls, rows_ops = [], []
    real = conv_stack.conv_panel

    def counted(stage, *a, stack_drop=None, **kw):
        active = stack_drop is not None and any(float(stack_drop.get(k) or 0.0) > 0 for k in ("p_inc", "p3", "p_x", "p1"))
        calls.append((stage, bool(kw.get("tail")), active))
        return real(stage, *a, stack_drop=stack_drop, **kw)
    monkeypatch.setattr(conv_stack, "conv_panel", counted)
    real_colsum = conv_stack.colsum

    def colsum(x, *a, **kw):          # (a row-weighted column sum -- a rowptr follows the rows: the d beta2 launch of the p = 0 path)
        if a:
            rows_ops.append("colsum(ds, rowptr)")
        return real_colsum(x, *a, **kw)
    monkeypatch.setattr(conv_stack, "colsum", colsum)
    for name in ("gather_ln_reduce", "linear_add_relu_ln"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **kw: (rows_ops.append(_n), _fn(*a, **kw))[1])
    return calls, rows_ops


def _run_conv_layers(m, x_host, w_host, index, seed):
    from equihgnn_amd import models
    for q in m.parameters():
        q.grad = None
    draws = _pool_draws(seed)
    x = x_host.to(DEV).requires_grad_(True)
    with m._dropout_scope(x):
        res = m.conv.prepare(x, index)
        assert isinstance(res, dict), "the merged path must stay on under an active dropout"
        out = models._conv_layers(m, x, index, x, res, True, None)
    (out * w_host.to(DEV)).sum().backward()
    got = {n: q.grad.clone() for n, q in m.conv.named_parameters()}
    got["x"] = x.grad.clone()
    return out.detach(), got, draws


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("C", [64, 256])
def test_the_stack_runs_under_dropout_and_matches_float64_and_the_row_kernels(C, L, monkeypatch):
    """models._conv_layers on mhnns, P = 0.3: the stack's stages carry the dropout (no gather_ln_reduce / linear_add_relu_ln
    inside the loop, at most four panel launches per application and direction); output and every gradient against the float64
    restatement of tests/test_hip_conv_dropout.py generalised to L applications, draws 4a .. 4a + 3; with STACK_DROPOUT off the
    row-kernel path agrees under the same seeds."""
    from equihgnn_amd import hip
    from equihgnn_amd.index import HyperIndex
    ops = _ops()
    alpha = 0.5
    monkeypatch.setattr(ops, "STACK_DROPOUT", True)
    m = _mhnns(C, L).train()
    assert m.conv.alpha == alpha
    data = make_batch(11, 6).to(DEV)
    index = HyperIndex.from_batch(data)
    N, v, e = data.x.shape[0], data.edge_index0.cpu(), data.edge_index1.cpu()
    M, nnz = int(data.edge_attr.shape[0]), v.numel()
    x_host = torch.randn(N, C, generator=torch.Generator().manual_seed(3))
    w_host = torch.randn(N, C, generator=torch.Generator().manual_seed(4))
    calls, rows_ops = _count_stack_calls(monkeypatch)
    out, got, draws = _run_conv_layers(m, x_host, w_host, index, 77)
    # --- the path: this is what fails without the feature
    assert any(active for _, _, active in calls), "the stack must run under an active dropout (hg_conv_stack_drop)"
    assert rows_ops == [], rows_ops
    F1, F2, F3, B3, B1 = hip.HG_CONV_F1, hip.HG_CONV_F2, hip.HG_CONV_F3, hip.HG_CONV_B3, hip.HG_CONV_B1
    assert [c[0] for c in calls] == [F1] + [F2, F3] * L + [B3] + [B1] * L
    assert all(active for stage, _, active in calls if stage != F2)
    assert [c[1] for c in calls if c[0] == F3] == [True] * (L - 1) + [False] and [c[1] for c in calls if c[0] == B1] == [True] * (L - 1) + [False]
    f3_launches = hip.lib().hg_conv_stack_drop_f3_launches(C, 0)
    assert f3_launches in (1, 2)
    # launches per application: forward F2 + F3 (+ a lone F1 where the shape runs unchained: the last application has no
    # tail, so this is the largest count); backward B1 (its B3 chained) + the incidence backward
    fwd = sum(c[0] in (F2, F3) for c in calls) // L - 1 + f3_launches
    bwd = sum(c[0] == B1 for c in calls) // L + 1
    assert fwd <= 4 and bwd <= 4, (fwd, bwd)
    # --- float64, draws 4a .. 4a + 3
    prm = {n: q.detach().cpu().double().requires_grad_(True) for n, q in m.conv.named_parameters()}
    keep = lambda i, rows: _keep(rows, C, P, draws[i:i + 1])
    x64 = x_host.double().requires_grad_(True)
    X = x64
    for a in range(L):
        Xin = X * keep(4 * a, N)
        xe = O.segment_reduce(_mlp64(prm, "W1", Xin, keep(4 * a + 1, N))[v], e, M, "mean")
        xev = _mlp64(prm, "W2", torch.cat((Xin[v], xe[e]), -1), keep(4 * a + 2, nnz))
        xv = O.segment_reduce(xev, v, N, "mean")
        X = torch.relu(_mlp64(prm, "W3", (1 - alpha) * xv + alpha * x64, keep(4 * a + 3, N)))
    (X * w_host.double()).sum().backward()
    ref = {n: q.grad for n, q in prm.items()}
    ref["x"] = x64.grad
    _check_layer(out, X, got, ref)
    # --- the row kernels under the same seeds
    del calls[:]
    monkeypatch.setattr(ops, "STACK_DROPOUT", False)
    out_rows, got_rows, _ = _run_conv_layers(m, x_host, w_host, index, 77)
    assert calls == [] and "gather_ln_reduce" in rows_ops and "linear_add_relu_ln" in rows_ops
    _check_layer(out_rows, out.cpu().double(), got_rows, {n: t.cpu().double() for n, t in got.items()})


@pytest.mark.parametrize("dropout,mode", [(0.0, "train"), (P, "eval")])
def test_without_an_active_dropout_the_new_entry_is_never_called_and_the_switch_changes_nothing(dropout, mode, monkeypatch):
    from equihgnn_amd.index import HyperIndex
    ops = _ops()
    C, L = 64, 2
    m = _mhnns(C, L, dropout).train(mode == "train")
    data = make_batch(11, 6).to(DEV)
    index = HyperIndex.from_batch(data)
    N = data.x.shape[0]
    x_host = torch.randn(N, C, generator=torch.Generator().manual_seed(3))
    w_host = torch.randn(N, C, generator=torch.Generator().manual_seed(4))
    calls, rows_ops = _count_stack_calls(monkeypatch)
    got = []
    for switch in (True, False):
        monkeypatch.setattr(ops, "STACK_DROPOUT", switch)
        got.append(_run_conv_layers(m, x_host, w_host, index, 77)[:2])
    assert len(calls) == 2 * (1 + 2 * L + 1 + L) and not any(active for _, _, active in calls)
    assert rows_ops == ["colsum(ds, rowptr)"] * (2 * L), rows_ops
    (oa, ga), (ob, gb) = got
    assert torch.equal(oa, ob) and sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_padding_leaves_the_masks_of_the_real_rows_where_they_were_on_the_stack(monkeypatch):
    """egnn_equihnns at P (tolerances of test_padding_leaves_the_masks_of_the_real_rows_where_they_were_on_the_panel_path): masks
    are keyed by row * C + c / incidence position * C + c and batch.pad_batch appends its rows and its (null) incidences at the
    end, so under one seed the real molecules of a padded batch get the unpadded result."""
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    monkeypatch.setattr(_ops(), "STACK_DROPOUT", True)
    m = _model("egnn_equihnns", P).train()
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


def test_graphed_egnn_equihnns_steps_draw_new_seeds_per_replay_and_eval_is_the_eager_eval(monkeypatch):
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedEvalStep, GraphedTrainStep
    ops = _ops()
    monkeypatch.setattr(ops, "STACK_DROPOUT", True)
    m = _model("egnn_equihnns", 0.1).train()
    raw = synth_batch(32, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 32
    tr = GraphedTrainStep(m, lr=0.0)        # the parameters stay put: the losses differ by their dropout draws alone
    tr.index_prefetch = False
    losses = [float(tr.step(batch)) for _ in range(5)]      # eager first step, capture, three replays
    print("egnn_equihnns losses over replays with dropout 0.1 on the stack:", losses)
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
