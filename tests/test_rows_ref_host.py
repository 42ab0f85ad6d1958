"""Host (no GPU): rows_ref, the reference of test_hip_row_bounds.py, checked against float64 autograd of the unfused torch
formulation (F.layer_norm, torch.relu, index_add_, F.batch_norm: what test_hip_kernels.py compares with); its magnitudes A
bound the values and vanish only where the structure makes the value 0; and the fixtures of test_hip_row_bounds.py (the
degree ladder, the row menagerie, the exact inputs) have the properties they are built for."""
import pytest
import torch
import torch.nn.functional as F

import rows_ref
import test_hip_row_bounds as B

pytestmark = []          # (test_hip_row_bounds marks its own tests, not these)
WIDTHS = B.WIDTHS
D = torch.float64


def _seg(vals, idx, n, mean):
    out = torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype).index_add(0, idx, vals)
    if mean:
        out = out / torch.bincount(idx, minlength=n).clamp(min=1).to(vals.dtype)[:, None]
    return out


def _leaves(a, *names):
    return [a[n].to(D).clone().requires_grad_(True) for n in names]


def _autograd(case):
    """The case through float64 autograd of the unfused formulation, under rows_ref's keys."""
    a = case.args
    g = a["g"].to(D)
    eps = a["eps"]
    if case.name == "layer_norm_rows":
        x, gamma, beta = t = _leaves(a, "x", "gamma", "beta")
        y = F.layer_norm(x, (x.shape[1],), gamma, beta, eps)
        keys = ("dx", "dgamma", "dbeta")
        out = {"y": y}
    elif case.name == "bias_relu_ln":
        h, bias, gamma, beta = t = _leaves(a, "h", "bias", "gamma", "beta")
        y = F.layer_norm(torch.relu(h + bias), (h.shape[1],), gamma, beta, eps)
        keys = ("dh", "dbias", "dgamma", "dbeta")
        out = {"y": y}
    elif case.name == "gather_ln_reduce":
        h, bias, gamma, beta = t = _leaves(a, "h", "bias", "gamma", "beta")
        y = _seg(F.layer_norm(torch.relu(h + bias), (h.shape[1],), gamma, beta, eps)[a["v"]], a["e"], a["n_out"], a["mean"])
        keys = ("dh", "dbias", "dgamma", "dbeta")
        out = {"out": y}
    elif case.name == "incidence_ln_reduce":
        pa, qb, gamma, beta = t = _leaves(a, "pa", "qb", "gamma", "beta")
        y = _seg(F.layer_norm(torch.relu(pa[a["ia"]] + qb[a["ib"]]), (pa.shape[1],), gamma, beta, eps), a["okey"], a["n_out"],
                 a["mean"])
        keys = ("dpa", "dqb", "dgamma", "dbeta")
        out = {"out": y}
    else:
        raise AssertionError(case.name)
    y.backward(g)
    out = {k: v.detach() for k, v in out.items()}
    out.update({k: leaf.grad for k, leaf in zip(keys, t)})
    return out


def _close(got, want, what):
    assert got.shape == want.shape, what
    if want.numel() == 0:
        return
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300), what


LN_NAMES = ("layer_norm_rows", "bias_relu_ln", "gather_ln_reduce", "incidence_ln_reduce")


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", LN_NAMES)
def test_layer_norm_references_agree_with_autograd(name, C):
    for case in B.ROUNDED[name](C):
        got, want = case.reference(), _autograd(case)
        assert set(got) == set(want)
        for key in want:
            _close(got[key], want[key], (case.label, key))


@pytest.mark.parametrize("C", WIDTHS)
def test_batch_norm_reference_agrees_with_autograd(C):
    """nn.BatchNorm1d's functional form on the counted rows alone (the padded rows reach no loss): outputs, gradients and
    running buffers of the counted rows; the padded rows are the same affine map, with a zero gradient."""
    for case in B.ROUNDED["batch_norm_rows"](C):
        a = case.args
        nr = a["x"].shape[0] if a["mask"] is None else int(a["mask"].sum())
        x, gamma, beta = _leaves(a, "x", "gamma", "beta")
        rm, rv = a["running_mean"].to(D).clone(), a["running_var"].to(D).clone()
        y = F.batch_norm(x[:nr], rm, rv, gamma, beta, True, a["momentum"], a["eps"])
        y = torch.relu(y) if a["relu"] else y
        y.backward(a["g"].to(D)[:nr])
        got = case.reference()
        _close(got["y"][:nr], y.detach(), (case.label, "y"))
        _close(got["dx"][:nr], x.grad[:nr], (case.label, "dx"))
        _close(got["dgamma"], gamma.grad, (case.label, "dgamma"))
        _close(got["dbeta"], beta.grad, (case.label, "dbeta"))
        _close(got["running_mean"], rm, (case.label, "running_mean"))
        _close(got["running_var"], rv, (case.label, "running_var"))
        xr = a["x"].to(D)[:nr]
        pad = (a["x"].to(D)[nr:] - xr.mean(0)) / torch.sqrt(xr.var(0, unbiased=False) + a["eps"]) * a["gamma"].to(D) + a["beta"].to(D)
        _close(got["y"][nr:], torch.relu(pad) if a["relu"] else pad, (case.label, "padded y"))
        assert bool((got["dx"][nr:] == 0).all())


@pytest.mark.parametrize("mean", [False, True])
def test_index_references_agree_with_autograd(mean):
    lad = B.ladder()
    C = 8
    gen = torch.Generator().manual_seed(3)
    X, S = torch.randn(lad.N, C, generator=gen, dtype=D), torch.randn(lad.nnz, C, generator=gen, dtype=D)
    gM, gN, gS = (torch.randn(n, C, generator=gen, dtype=D) for n in (lad.M, lad.N, lad.nnz))
    x = X.clone().requires_grad_(True)
    y = _seg(x[lad.v], lad.e, lad.M, mean)
    y.backward(gM)
    got = rows_ref.reduce_gathered(X, lad.v, lad.e, lad.M, gM, mean)
    _close(got["out"], y.detach(), "reduce_gathered")
    _close(got["dsrc"], x.grad, "reduce_gathered backward")
    s = S.clone().requires_grad_(True)
    y = _seg(s, lad.v, lad.N, mean)
    y.backward(gN)
    got = rows_ref.reduce_entries(S, lad.v, lad.N, gN, mean)
    _close(got["out"], y.detach(), "reduce_entries")
    _close(got["dsrc"], s.grad, "reduce_entries backward")
    x = X.clone().requires_grad_(True)
    y = x[lad.v]
    y.backward(gS)
    got = rows_ref.gather_rows(X, lad.v, gS)
    _close(got["out"], y.detach(), "gather_rows")
    _close(got["dsrc"], x.grad, "gather_rows backward")
    for mode in (0, 1, 2):
        w = (torch.ones(lad.N) if mode == 0 else (lad.deg_v > 0) if mode == 1 else lad.deg_v).to(D)[:, None]
        _close(rows_ref.colsum(X, lad.deg_v, mode, 0.7)["out"], 0.7 * (w * X).sum(0), ("colsum", mode))
        if mode:
            x0, b = X.clone().requires_grad_(True), torch.randn(C, generator=gen, dtype=D).requires_grad_(True)
            y = 0.3 * x0 + (1 - 0.3) * w * b
            y.backward(gN)
            got = rows_ref.residual_mix(X, b.detach(), lad.deg_v, mode, 0.3, gN)
            _close(got["out"], y.detach(), ("residual_mix", mode))
            _close(got["dx0"], x0.grad, ("residual_mix dx0", mode))
            _close(got["dbias"], b.grad, ("residual_mix dbias", mode))


# ----------------------------------------------------------------------------------------------------------------------
# the magnitudes
# ----------------------------------------------------------------------------------------------------------------------
def _same_structure(case, seed):
    """The case with other magnitudes and the same structure: the rows (and bias) times one positive scalar, so every
    ReLU keeps its decision; gamma, beta and the upstream gradient times positive factors per element, so zeros stay zeros
    and signs stay signs.  BatchNorm's fused ReLU decides on gamma xhat + beta: there only the gradient changes."""
    gen = torch.Generator().manual_seed(seed)
    a = dict(case.args)

    def factors(t):
        return 0.5 + 1.5 * torch.rand(t.shape, generator=gen)

    a["g"] = a["g"] * factors(a["g"])
    if case.name != "batch_norm_rows":
        for k in ("x", "h", "bias", "pa", "qb"):
            if k in a:
                a[k] = a[k] * 2.0
        a["gamma"], a["beta"] = a["gamma"] * factors(a["gamma"]), a["beta"] * factors(a["beta"])
    return a


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", list(B.ROUNDED))
def test_magnitudes_bound_the_values_and_vanish_only_by_structure(name, C):
    for case in B.ROUNDED[name](C):
        want, mag = case.reference(), case.reference(magnitude=True)
        other = _same_structure(case, C)
        want2, mag2 = case.fn(**other), case.fn(**other, magnitude=True)
        for key in want:
            assert bool((mag[key] >= want[key].abs()).all()), (case.label, key)
            assert bool((mag[key] >= 0).all()) and bool(torch.isfinite(mag[key]).all()), (case.label, key)
            zero = mag[key] == 0
            assert bool((want[key][zero] == 0).all()), (case.label, key)
            # the same elements, and no others, for other values on the same index structure and ReLU pattern
            assert torch.equal(zero, mag2[key] == 0), (case.label, key)
            assert bool((want2[key][zero] == 0).all()), (case.label, key)
        for label, key, mask in case.zeros:        # what the GPU test asserts exactly is where A is 0
            assert int(mask.sum()) > 0 and bool((mag[key][mask] == 0).all()), (case.label, label)
        for label, key, row, row_want in case.equals:
            assert torch.equal(want[key][row].float(), row_want.float()) or \
                float((want[key][row] - row_want.double()).abs().max()) <= 1e-6 * float(row_want.abs().max()), (case.label, label)


# ----------------------------------------------------------------------------------------------------------------------
# the fixtures
# ----------------------------------------------------------------------------------------------------------------------
def _longest_empty_run(deg):
    best = run = 0
    for d in deg.tolist():
        run = run + 1 if d == 0 else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("pow2", [False, True])
def test_ladder_has_its_degrees(pow2):
    lad = B.ladder(pow2)
    rungs = B.POW2_LADDER if pow2 else B.LADDER
    assert 190 <= lad.N <= 210 and 180 <= lad.M <= 200 and lad.nnz < 2000
    assert int(lad.v.min()) >= 0 and int(lad.v.max()) < lad.N and int(lad.e.min()) >= 0 and int(lad.e.max()) < lad.M
    for deg in (lad.deg_v, lad.deg_e):
        assert set(rungs) <= set(deg.tolist())
        for d in rungs:
            assert int(deg[lad.row(d)]) == d
        assert int(deg[0]) == 0 and int(deg[-1]) == 0 and _longest_empty_run(deg[1:-1]) >= 4
        assert int(deg.sum()) == lad.nnz
        if pow2:
            assert all(d == 0 or d & (d - 1) == 0 for d in deg.tolist())
    assert int((lad.deg_v == 0).sum()) >= 7                           # source rows that no entry gathers
    pairs = lad.v * lad.M + lad.e
    assert int((torch.bincount(pairs) == 2).sum()) >= 1              # an incidence listed twice
    assert not bool((lad.v[1:] >= lad.v[:-1]).all())                 # listed in no sorted order
    # a degree-1 row sits next to the hub on both sides (a mean weight taken from the neighbouring row would show)
    for deg in (lad.deg_v, lad.deg_e):
        hub = lad.row(rungs[-1])
        assert 1 in (int(deg[hub - 1]), int(deg[hub + 1]))
    big = lad.tiled(12)
    assert big.N == 12 * lad.N > 2048 and torch.equal(big.deg_v, lad.deg_v.repeat(12))
    assert bool((big.v // lad.N == big.e // lad.M).all())            # block-diagonal


@pytest.mark.parametrize("C", WIDTHS)
def test_menagerie_rows_are_what_they_are_called(C):
    bias, gamma, beta = B.parameters(C, 5)
    assert int((gamma == 0).sum()) == 1 and int((gamma < 0).sum()) == 1 and int((beta == 0).sum()) == 1
    assert bool((bias * 8 == (bias * 8).round()).all())
    for b in (bias, None):
        h = B.menagerie(150, C, 3, b)
        pre = h + (b if b is not None else 0.0)              # fp32, as the kernels add
        k = {kind: pre[i] for i, kind in enumerate(B.KINDS)}
        assert bool((k["dead"] < 0).all())
        assert int((k["one_live"] > 0).sum()) == 1
        assert bool((k["constant"] == 0.75).all())
        assert float(k["times_2^10"].abs().max()) > 500 and float(k["times_2^-10"].abs().max()) < 0.01
        assert float(k["plus_100"].min()) > 90
        assert bool((k["size_1e-3"] > 0).all()) and float(k["size_1e-3"].max()) < 0.01
        zc = B.zero_channels(C)
        assert len(zc) == min(4, C) and bool((k["zeros"][zc] == 0).all())
        if b is not None:
            assert torch.equal(h[B.KINDS.index("zeros")][zc], -b[zc])
        assert abs(float(pre[len(B.KINDS):].std()) - 1.0) < 0.2 if b is None else True
    g = B.upstream(150, C, 1, zero_row=9)
    assert int((g.abs().sum(-1) == 0).sum()) == 1


@pytest.mark.parametrize("C", WIDTHS)
def test_relu_decides_alike_in_fp32_and_float64(C):
    """h + bias and pa + qb are one rounded add of two fp32 numbers: the rounded sum has the sign of the exact one."""
    seen = 0
    for name in ("bias_relu_ln", "gather_ln_reduce", "incidence_ln_reduce"):
        for case in B.ROUNDED[name](C):
            a = case.args
            if name == "incidence_ln_reduce":
                lo, hi = (a["pa"][a["ia"]], a["qb"][a["ib"]])
            else:
                lo, hi = a["h"], a["bias"].expand_as(a["h"])
            assert lo.dtype == hi.dtype == torch.float32
            assert torch.equal(torch.sign(lo + hi).double(), torch.sign(lo.double() + hi.double())), case.label
            seen += int(((lo + hi) == 0).sum())
    assert seen > 0             # pre-activations that are exactly 0 are among them


def test_special_rows_sit_in_the_hub_and_in_a_degree_one_row():
    lad = B.ladder()
    places = dict(B.ladder_places(lad))
    assert places[lad.row(129)] == "dead" and places[lad.row(1)] == "times_2^10"
    assert sorted(set(places.values())) == sorted(B.KINDS)
    C = 64
    for mean in (False, True):
        case = B.incidence_case(C, mean, "a")
        a = case.args
        for row, kind in places.items():
            mine = a["ia"] == row
            alone = mine & (a["qb"][a["ib"]].abs().sum(-1) == 0)           # incidences whose pre-activation is pa's row itself
            assert int(alone.sum()) >= 1, (row, kind)
            pre = a["pa"][row]
            if kind == "dead":
                assert bool((a["pa"][a["ia"][mine]] + a["qb"][a["ib"][mine]] < 0).all())       # with every hyperedge row
            if kind == "constant":
                assert bool((pre == 0.75).all())
            if kind == "zeros":
                assert bool((pre[B.zero_channels(C)] == 0).all())
        case = B.gather_case(C, mean)
        g = case.args["g"]
        assert int((g.abs().sum(-1) == 0).sum()) == 1


@pytest.mark.parametrize("relu_C", WIDTHS)
def test_batch_norm_relu_is_decided_away_from_zero(relu_C):
    """The fused ReLU of batch_norm_rows decides on gamma xhat + beta, a rounded quantity: in every case that value is more
    than K 2^-24 A away from 0, so a device that meets the bound decides as the reference does."""
    for case in B.ROUNDED["batch_norm_rows"](relu_C):
        if not case.args["relu"]:
            continue
        args = {**case.args, "relu": False}
        y, A = rows_ref.batch_norm_rows(**args)["y"], rows_ref.batch_norm_rows(**args, magnitude=True)["y"]
        assert bool((y.abs() > B.K["batch_norm_rows"] * B.EPS * A).all()), (case.label, float((y.abs() / (B.EPS * A)).min()))


@pytest.mark.parametrize("C", [4, 260])
def test_exact_inputs_are_exact(C):
    """Inputs in {-1, 0, 1}: every float64 result of the exact operators is an fp32 number (sums on the ladder, means on
    the ladder of powers of two)."""
    for mean, lad in ((False, B.ladder()), (True, B.ladder(pow2=True))):
        X, gM, S, gN = B._ints((lad.N, C), 1), B._ints((lad.M, C), 2), B._ints((lad.nnz, C), 3), B._ints((lad.N, C), 4)
        for t in (X, gM, S, gN):
            assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
        res = [rows_ref.reduce_gathered(X, lad.v, lad.e, lad.M, gM, mean), rows_ref.reduce_entries(S, lad.v, lad.N, gN, mean),
               rows_ref.colsum(gN, lad.deg_v, 2), rows_ref.residual_mix(X, B._ints((C,), 6), lad.deg_v, 2, 0.5, gN)]
        for r in res:
            for key, t in r.items():
                assert torch.equal(t.float().double(), t), key
                assert float(t.abs().max()) > 0


def test_constants_are_four_times_the_reference():
    """K cites the fp32 reference's own worst ratio over all widths (test_hip_row_bounds.py's __main__ prints it).  Here
    two widths are measured again: no case may lose more than K / 4 allows, give or take the summation order of the
    host's vector units (a tenth)."""
    for name in B.ROUNDED:
        for C in (4, 260):
            for case in B.ROUNDED[name](C):
                r = B.reference_ratios(case)
                assert max(r.values()) <= 1.1 * B.K[name] / 4, (case.label, r)
