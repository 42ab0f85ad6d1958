"""Training dropout of the hypergraph convs on the fused row kernels (csrc/incidence.hip, ops/rows.py, layers.py,
models.py): the dropout forms of bias_relu_ln / linear_add_relu_ln, gather_ln_reduce and incidence_ln_reduce against float64,
the properties of the hashed masks, p = 0 left as it was, and the layers / models in training mode with p > 0.

The keep matrix of a site is what ``ops.dropout_add(ones[R, C], None, p, seed)`` returns (faf_dropout_add hashes the flat
element index, csrc/faformer_ew.hip): the expectations below are plain torch in float64 with that matrix multiplied in
behind ``layer_norm``.  Tolerances are those of the p = 0 tests of the same kernel in tests/test_hip_kernels.py times
1 / (1 - p): every kept value and its gradient carries that factor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, golden_args, make_batch  # noqa: E402

from oracle import ref_models as O  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def _ops():
    from equihgnn_amd import ops
    return ops


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _keep(rows, C, p, seed):
    """[rows, C] float64 on the host: 0 or 1 / (1 - p), the decisions of flat index r * C + c under ``seed``"""
    ops = _ops()
    return ops.dropout_add(torch.ones(rows, C, device=DEV), None, p, seed).double().cpu()


def _grad_err(x, r):
    return float((x.grad.cpu().double() - r.grad).abs().max() / r.grad.abs().max().clamp(min=1e-9))


# ---------------------------------------------------------------------------------------------------------------------
# kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("R,C", [(1, 64), (150, 64), (150, 68), (150, 256), (1, 1024), (150, 1024)])
def test_bias_relu_ln_dropout_matches_float64_reference(R, C, p):
    ops = _ops()
    g = torch.Generator().manual_seed(R + C)
    h, b = torch.randn(R, C, generator=g), 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(R, C, generator=g)
    seed = _seed(1000 + R + C)
    keep = _keep(R, C, p, seed)
    t = [x.double().requires_grad_(True) for x in (h, b, gamma, beta)]
    ref = F.layer_norm(torch.relu(t[0] + t[1]), (C,), t[2], t[3], 1e-5) * keep
    (ref * w.double()).sum().backward()
    d = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    out = ops.bias_relu_ln(d[0], d[1], d[2], d[3], p=p, seed=seed)
    (out * w.to(DEV)).sum().backward()
    s = 1.0 / (1.0 - p)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-5 * s, rtol=1e-5)
    for name, x, r in zip(("dh", "dbias", "dgamma", "dbeta"), d, t):
        err = _grad_err(x, r)
        print(f"bias_relu_ln R={R} C={C} p={p} {name}: {err:.2e}")
        assert err < 3e-5 * s, (name, err)


def test_linear_add_relu_ln_dropout_matches_float64_reference():
    """The generalised form (h_scale != 1, pre_add) behind a GEMM, applied twice to one fanned-out addend: its gradient is
    the sum of the two applications' pre-activation gradients, delivered through the GradFan."""
    ops = _ops()
    R, K, C, p, scale = 150, 64, 68, 0.25, 0.5
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(R, K, generator=g) for _ in range(2)]
    W, c = torch.randn(C, K, generator=g) / 8, torch.randn(R, C, generator=g)
    b, gamma, beta = 0.3 * torch.randn(C, generator=g), 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    ws = [torch.randn(R, C, generator=g) for _ in range(2)]
    seeds = [_seed(71), _seed(72)]
    keeps = [_keep(R, C, p, s) for s in seeds]
    t = [x.double().requires_grad_(True) for x in (xs[0], xs[1], W, c, b, gamma, beta)]
    refs = [F.layer_norm(torch.relu(scale * (t[i] @ t[2].T) + t[3] + t[4]), (C,), t[5], t[6], 1e-5) * keeps[i] for i in range(2)]
    sum((r * w.double()).sum() for r, w in zip(refs, ws)).backward()
    d = [x.to(DEV).requires_grad_(True) for x in (xs[0], xs[1], W, c, b, gamma, beta)]
    cf, fan = ops.fanout(d[3])
    outs = [ops.linear_add_relu_ln(d[i], d[2], cf, scale, d[4], d[5], d[6], fan=fan, p=p, seed=seeds[i]) for i in range(2)]
    sum((o * w.to(DEV)).sum() for o, w in zip(outs, ws)).backward()
    s = 1.0 / (1.0 - p)
    for o, r in zip(outs, refs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), r.detach().numpy(), atol=2e-5 * s, rtol=1e-5)
    for name, x, r in zip(("dx0", "dx1", "dW", "dc", "dbias", "dgamma", "dbeta"), d, t):
        err = _grad_err(x, r)
        print(f"linear_add_relu_ln {name}: {err:.2e}")
        assert err < 3e-5 * s, (name, err)


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("C", [64, 68, 256, 1024])
def test_gather_ln_reduce_dropout_matches_float64_reference(C, reduce, p):
    """The decision belongs to the SOURCE row: dropout of the [N, C] hidden tensor, then the gather (index construction of
    test_gather_ln_reduce_matches_float64_reference: unused source rows, empty output rows, rows longer than 64 entries)."""
    ops = _ops()
    N = 150
    g = torch.Generator().manual_seed(N + C)
    M, nnz = N - 7, 3 * N
    v = torch.randint(0, N - 10, (nnz,), generator=g)      # the last 10 source rows are never gathered
    e = torch.randint(0, M - 5, (nnz,), generator=g)       # the last 5 output rows are empty
    v[:150] = 3                                            # a source row with 150 entries
    e[200:300] = 11                                        # an output row with 100 entries
    h, b = torch.randn(N, C, generator=g), 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(M, C, generator=g)
    seed = _seed(2000 + C)
    keep = _keep(N, C, p, seed)
    t = [x.double().requires_grad_(True) for x in (h, b, gamma, beta)]
    y = F.layer_norm(torch.relu(t[0] + t[1]), (C,), t[2], t[3], 1e-5) * keep
    ref = O.segment_reduce(y[v], e, M, reduce)
    (ref * w.double()).sum().backward()
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    d = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    out = ops.gather_ln_reduce(d[0], d[1], d[2], d[3], by_e, by_v, reduce, p=p, seed=seed)
    (out * w.to(DEV)).sum().backward()
    s = 1.0 / (1.0 - p)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=3e-5 * s, rtol=1e-5)
    assert float(out[-5:].detach().abs().max()) == 0.0
    assert float(d[0].grad[-10:].abs().max()) == 0.0
    for name, x, r in zip(("dh", "dbias", "dgamma", "dbeta"), d, t):
        err = _grad_err(x, r)
        print(f"gather_ln_reduce C={C} {reduce} p={p} {name}: {err:.2e}")
        assert err < 3e-5 * s, (name, err)


def _incidence_case(C):
    g = torch.Generator().manual_seed(C)
    N, M, nnz = 150, 140, 420
    v = torch.randint(0, N - 10, (nnz,), generator=g)      # the last 10 node rows have no incidence
    e = torch.randint(0, M, (nnz,), generator=g)
    v[:70] = 3                                             # one long row (> 64 incidences)
    pa, qb = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    return g, N, M, nnz, v, e, pa, qb, gamma, beta


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("C", [64, 68, 256, 1024])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("path", ["generic", "rows_are_a", "rows_are_b"])
def test_incidence_ln_reduce_dropout_matches_float64_reference(C, reduce, path, p):
    """The decision belongs to the INCIDENCE (its position in ia / ib), as F.dropout of the [nnz, C] tensor gives it; all
    three forward forms and the backward (d beta from the kernel's own slab) against the unfused float64 formulation."""
    ops = _ops()
    g, N, M, nnz, v, e, pa, qb, gamma, beta = _incidence_case(C)
    by_rows_of_b = path == "rows_are_b"
    R = M if by_rows_of_b else N
    w = torch.randn(R, C, generator=g)
    seed = _seed(3000 + C)
    keep = _keep(nnz, C, p, seed)
    t = [x.double().requires_grad_(True) for x in (pa, qb, gamma, beta)]
    h = F.layer_norm(torch.relu(t[0][v] + t[1][e]), (C,), t[2], t[3], 1e-5) * keep
    ref = O.segment_reduce(h, e if by_rows_of_b else v, R, reduce)
    (ref * w.double()).sum().backward()
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    d = [x.to(DEV).requires_grad_(True) for x in (pa, qb, gamma, beta)]
    v32, e32 = v.to(DEV).int(), e.to(DEV).int()
    okey = {"generic": v.to(DEV).int(), "rows_are_a": v32, "rows_are_b": e32}[path]
    out = ops.incidence_ln_reduce(d[0], d[1], d[2], d[3], v32, e32, by_v, by_e, by_e if by_rows_of_b else by_v, okey, reduce,
                                  p=p, seed=seed)
    (out * w.to(DEV)).sum().backward()
    s = 1.0 / (1.0 - p)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=3e-5 * s, rtol=1e-5)
    if not by_rows_of_b:
        assert float(out[-10:].detach().abs().max()) == 0.0
    for name, x, r in zip(("dpa", "dqb", "dgamma", "dbeta"), d, t):
        err = _grad_err(x, r)
        print(f"incidence_ln_reduce C={C} {reduce} {path} p={p} {name}: {err:.2e}")
        assert err < 2e-5 * s, (name, err)


# ---------------------------------------------------------------------------------------------------------------------
# mask properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [68, 256, 1024])
def test_dense_kernel_with_zero_gamma_and_unit_beta_returns_the_keep_matrix_bit_for_bit(C):
    ops = _ops()
    R, p, seed = 150, 0.25, _seed(41)
    h = torch.randn(R, C, device=DEV)
    out = ops.bias_relu_ln(h, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), p=p, seed=seed)
    keep = ops.dropout_add(torch.ones(R, C, device=DEV), None, p, seed)
    assert torch.equal(out, keep)
    assert sorted(set(out.unique().tolist())) == [0.0, float(np.float32(1.0) / np.float32(1.0 - p))]


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_incidence_kernel_on_one_incidence_per_row_returns_keep_of_the_incidence(reduce):
    """okey = arange(nnz): output row p holds incidence p alone, so with gamma = 0, beta = 1 it IS keep[p] (general form)."""
    ops = _ops()
    C, p, seed = 68, 0.5, _seed(43)
    g, N, M, nnz, v, e, pa, qb, _, _ = _incidence_case(C)
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    okey = torch.arange(nnz, device=DEV)
    out_csr = ops.csr_build(okey, None, nnz)
    out = ops.incidence_ln_reduce(pa.to(DEV), qb.to(DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), v.to(DEV).int(),
                                  e.to(DEV).int(), by_v, by_e, out_csr, okey.int(), reduce, p=p, seed=seed)
    assert torch.equal(out, ops.dropout_add(torch.ones(nnz, C, device=DEV), None, p, seed))


def test_same_seed_is_bit_identical_and_two_seeds_are_independent():
    ops = _ops()
    R, C = 2048, 256
    n = R * C
    h = torch.randn(R, C, device=DEV)
    z, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    for p in (0.25, 0.5):
        q = round(p * 65536) / 65536                     # the realised drop probability
        a = ops.bias_relu_ln(h, z, 1 + z, 0.1 * one, p=p, seed=_seed(5))
        assert torch.equal(a, ops.bias_relu_ln(h, z, 1 + z, 0.1 * one, p=p, seed=_seed(5)))
        ka = ops.bias_relu_ln(h, z, z, one, p=p, seed=_seed(5)) > 0
        kb = ops.bias_relu_ln(h, z, z, one, p=p, seed=_seed(6)) > 0
        sd = (q * (1 - q) / n) ** 0.5
        for k in (ka, kb):
            assert abs(float(k.double().mean()) - (1 - q)) <= 5 * sd
        agree = q * q + (1 - q) * (1 - q)
        assert abs(float((ka == kb).double().mean()) - agree) <= 5 * (agree * (1 - agree) / n) ** 0.5


def test_three_forward_forms_decide_per_incidence_whatever_order_they_walk():
    """A permutation of the incidence arrays together with the keep rows leaves every form's output where it was: with
    gamma = 0, beta = 1 the output is the reduction of the keep rows alone, compared against the permuted expectation."""
    ops = _ops()
    C, p, seed = 64, 0.5, _seed(47)
    g, N, M, nnz, v, e, pa, qb, _, _ = _incidence_case(C)
    perm = torch.randperm(nnz, generator=g)
    keep = _keep(nnz, C, p, seed)
    zeros, ones = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    for vv, ee in ((v, e), (v[perm], e[perm])):
        by_v = ops.csr_build(vv.to(DEV), ee.to(DEV), N)
        by_e = ops.csr_build(ee.to(DEV), vv.to(DEV), M)
        v32, e32 = vv.to(DEV).int(), ee.to(DEV).int()
        want_v = O.segment_reduce(keep, vv, N, "sum").numpy()
        want_e = O.segment_reduce(keep, ee, M, "sum").numpy()
        for okey, csr, want in ((vv.to(DEV).int(), by_v, want_v), (v32, by_v, want_v), (e32, by_e, want_e)):
            out = ops.incidence_ln_reduce(pa.to(DEV), qb.to(DEV), zeros, ones, v32, e32, by_v, by_e, csr, okey, "sum", p=p,
                                          seed=seed)
            np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# p = 0 is untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_p_zero_is_the_call_without_the_argument():
    ops = _ops()
    C = 68
    g, N, M, nnz, v, e, pa, qb, gamma, beta = _incidence_case(C)
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    v32, e32 = v.to(DEV).int(), e.to(DEV).int()
    bias = 0.3 * torch.randn(C, generator=g)
    W, x = torch.randn(C, 64, generator=g) / 8, torch.randn(N, 64, generator=g)
    w = torch.randn(N, C, generator=g).to(DEV)

    def run(op, **kw):
        d = [t.to(DEV).requires_grad_(True) for t in (pa, qb, gamma, beta, bias, W, x)]
        if op == "bias_relu_ln":
            out = ops.bias_relu_ln(d[0], d[4], d[2], d[3], **kw)
        elif op == "linear_add_relu_ln":
            out = ops.linear_add_relu_ln(d[6], d[5], d[0], 0.5, d[4], d[2], d[3], **kw)
        elif op == "gather_ln_reduce":
            out = ops.gather_ln_reduce(d[1], d[4], d[2], d[3], by_v, by_e, "mean", **kw)
        else:
            out = ops.incidence_ln_reduce(d[0], d[1], d[2], d[3], v32, e32, by_v, by_e, by_v, v32, "mean", **kw)
        (out * w).sum().backward()
        return [out.detach()] + [t.grad for t in d if t.grad is not None]

    for op in ("bias_relu_ln", "linear_add_relu_ln", "gather_ln_reduce", "incidence_ln_reduce"):
        a, b = run(op), run(op, p=0.0)
        assert len(a) == len(b) and len(a) >= 4, op
        for s, t in zip(a, b):
            assert torch.equal(s, t), op


def _model(method, dropout, layers=2, seed=13):
    from equihgnn_amd import models
    m = models.MODELS[method](1, golden_args(method, 64, dropout=dropout, All_num_layers=layers))
    fill_state_dict(m, seed)
    return m.to(DEV)


def _step(m, data):
    for q in m.parameters():
        q.grad = None
    out = m(data)
    loss = F.mse_loss(out, data.y)
    loss.backward()
    return out.detach().clone(), float(loss.detach()), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("method", ["egnn_equihnns", "mhnnm"])
@pytest.mark.parametrize("dropout,mode", [(0.0, "train"), (0.3, "eval")])
def test_switch_changes_nothing_without_an_active_dropout(method, dropout, mode, monkeypatch):
    ops = _ops()
    data = make_batch(11, 6).to(DEV)
    m = _model(method, dropout)
    m.train(mode == "train")
    buf = {n: t.clone() for n, t in m.named_buffers()}
    got = []
    for switch in (True, False):
        monkeypatch.setattr(ops, "FUSED_DROPOUT", switch)
        for n, t in m.named_buffers():
            t.copy_(buf[n])
        data._hyper_index = None
        got.append(_step(m, data))
    (oa, la, ga), (ob, lb, gb) = got
    assert torch.equal(oa, ob) and la == lb and sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


# ---------------------------------------------------------------------------------------------------------------------
# layers and models in training mode, p = 0.3
# ---------------------------------------------------------------------------------------------------------------------
P = 0.3


def _mlp64(prm, name, x, keep):
    """mlp.py:91-99 with two Linears: Linear -> ReLU -> LayerNorm -> dropout -> Linear, in float64"""
    g = lambda k: prm[f"{name}.{k}"]
    h = x @ g("lins.0.weight").T + g("lins.0.bias")
    h = F.layer_norm(torch.relu(h), (h.shape[-1],), g("normalizations.1.weight"), g("normalizations.1.bias"), 1e-5) * keep
    return h @ g("lins.1.weight").T + g("lins.1.bias")


def _check_layer(got_out, ref_out, got_grads, ref_grads):
    """Output at the golden tests' forward tolerance (common.assert_close, 1e-5) and gradients at their training tolerance
    (test_hip_models.py: grad_rtol 3e-4 of the entry scale, floored at 1e-3 of the largest gradient), both times 1 / (1 - p)."""
    s = 1.0 / (1.0 - P)
    err = (got_out.detach().cpu().double() - ref_out.detach()).abs() / ref_out.detach().abs().clamp(min=1.0)
    print(f"layer output: {float(err.max()):.2e}")
    assert float(err.max()) <= 1e-5 * s
    gmax = max(float(r.abs().max()) for r in ref_grads.values())
    for n, r in ref_grads.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((got_grads[n].cpu().double() - r).abs().max()) / scale
        print(f"layer gradient {n}: {e:.2e}")
        assert e <= 3e-4 * s, (n, e)


def _pool_draws(s):
    """the 64 draws ops.dropout_seeds makes after torch.manual_seed(s); leaves the generator reseeded"""
    torch.manual_seed(s)
    draws = torch.randint(0, 2 ** 62, (64,), dtype=torch.int64, device=DEV)
    torch.manual_seed(s)
    return draws


def test_mhnns_conv_through_the_s_tail_loop_matches_float64_with_the_documented_seed_order():
    """conv.py:169-182 + mlp.py:91-99 + the wrapper's loop (dropout -> conv -> ReLU) restated in float64, the keep matrices
    taken in the documented order: per application input dropout, W1 ([N, C]), W2 ([nnz, C]), W3 ([N, C])."""
    from equihgnn_amd import models
    from equihgnn_amd.index import HyperIndex
    L, C, alpha = 2, 64, 0.5
    m = _model("mhnns", P, layers=L).train()
    assert m.conv.alpha == alpha
    data = make_batch(11, 6).to(DEV)
    index = HyperIndex.from_batch(data)
    N, v, e = data.x.shape[0], data.edge_index0.cpu(), data.edge_index1.cpu()
    M, nnz = int(data.edge_attr.shape[0]), v.numel()
    x_host = torch.randn(N, C, generator=torch.Generator().manual_seed(3))
    draws = _pool_draws(77)
    x = x_host.to(DEV).requires_grad_(True)
    with m._dropout_scope(x):
        res = m.conv.prepare(x, index)
        assert isinstance(res, dict), "the merged path must stay on under an active dropout"
        out = models._conv_layers(m, x, index, x, res, True, None)
    w = torch.randn(N, C, generator=torch.Generator().manual_seed(4))
    (out * w.to(DEV)).sum().backward()

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
    (X * w.double()).sum().backward()
    got = {n: q.grad for n, q in m.conv.named_parameters()}
    got["x"], ref = x.grad, {n: q.grad for n, q in prm.items()}
    ref["x"] = x64.grad
    _check_layer(out, X, got, ref)


def test_mhnn_conv_one_application_matches_float64_with_the_documented_seed_order():
    """conv.py:87-101 with four 2-layer MLPs: the seeds go W1 ([nnz, C]), W2 ([M, C]), W3 ([nnz, C]), W4 ([N, C])."""
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import MHNNConv
    ops = _ops()
    C = 64
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
    draws = _pool_draws(78)
    x, ee = xh.to(DEV).requires_grad_(True), eh.to(DEV).requires_grad_(True)
    with ops.dropout_seeds(DEV, 64):
        xo, eo = conv(x, ee, index)
    ((xo * wx.to(DEV)).sum() + (eo * we.to(DEV)).sum()).backward()

    prm = {n: q.detach().cpu().double().requires_grad_(True) for n, q in conv.named_parameters()}
    keep = lambda i, rows: _keep(rows, C, P, draws[i:i + 1])
    X, E = xh.double().requires_grad_(True), eh.double().requires_grad_(True)
    me = O.segment_reduce(_mlp64(prm, "W1", torch.cat((X[v], E[e]), -1), keep(0, nnz)), e, M, "mean")
    E1 = _mlp64(prm, "W2", torch.cat((E, me), -1), keep(1, M))
    mv = O.segment_reduce(_mlp64(prm, "W3", torch.cat((X[v], E1[e]), -1), keep(2, nnz)), v, N, "mean")
    X1 = _mlp64(prm, "W4", torch.cat((X, mv), -1), keep(3, N))
    ((X1 * wx.double()).sum() + (E1 * we.double()).sum()).backward()
    got = {n: q.grad for n, q in conv.named_parameters()}
    got["x"], got["e"] = x.grad, ee.grad
    ref = {n: q.grad for n, q in prm.items()}
    ref["x"], ref["e"] = X.grad, E.grad
    _check_layer(torch.cat((xo, eo)), torch.cat((X1, E1)), got, ref)


@pytest.mark.parametrize("method", ["egnn_equihnns", "mhnnm", "mhnn"])
def test_one_training_step_with_dropout_reaches_every_parameter_and_repeats_under_one_seed(method):
    data = make_batch(11, 6).to(DEV)
    _, _, g0 = _step(_model(method, 0.0).train(), data)
    m = _model(method, P).train()
    data._hyper_index = None
    buf = {n: t.clone() for n, t in m.named_buffers()}
    torch.manual_seed(5)
    out, loss, g = _step(m, data)
    assert np.isfinite(loss) and bool(torch.isfinite(out).all())
    assert sorted(g) == sorted(g0)
    assert all(bool(torch.isfinite(t).all()) for t in g.values())
    for n, t in m.named_buffers():
        t.copy_(buf[n])
    torch.manual_seed(5)
    out2, loss2, g2 = _step(m, data)
    assert torch.equal(out, out2) and loss == loss2
    for n in g:
        assert torch.equal(g[n], g2[n]), n
    for n, t in m.named_buffers():
        t.copy_(buf[n])
    torch.manual_seed(6)
    assert not torch.equal(out, _step(m, data)[0])


def test_padding_leaves_the_masks_of_the_real_rows_where_they_were():
    """Masks are keyed by row * C + c / incidence * C + c and batch.pad_batch appends its rows and its (null) incidences at
    the end, so under one seed the real molecules of a padded batch get the unpadded result (tolerances of
    test_padded_batch_is_exact for the LayerNorm models)."""
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
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


def test_graphed_steps_draw_new_seeds_per_replay_and_eval_is_the_eager_eval():
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedEvalStep, GraphedTrainStep
    m = _model("egnn_equihnns", 0.1).train()
    raw = synth_batch(32, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 32
    tr = GraphedTrainStep(m, lr=0.0)        # the parameters stay put: the losses differ by their dropout draws alone
    tr.index_prefetch = False
    losses = [float(tr.step(batch)) for _ in range(5)]      # eager first step, capture, three replays
    print("losses over replays with dropout 0.1:", losses)
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
