"""GPU: the hypergraph row kernels (csrc/incidence.hip + rowln.h, segment_reduce.hip, bn_rows.hip, the column sums and
the residual mix of dense_aux.hip) held to per-element bounds, on index structures and rows built to sit on the kernels'
internal boundaries.

* ``ladder``: a hand-built incidence list over ~200 node rows and ~190 hyperedge rows with, on each side, rows of degree
  0, 1, ..., 9, 63, 64, 65 and 129 (the forward bodies unroll by four, the backward bodies fetch 64 incidences at a time),
  empty rows at index 0, at the last index and in a run of five, incidences listed twice; ``ladder(pow2=True)`` has only
  degrees that are 0 or a power of two (the mean and its backward are then exact).
* ``menagerie``: unit-normal rows with a row ReLU kills, a row with one live channel, a constant row, rows times 2^10 and
  2^-10, a row plus 100, a positive row of size 1e-3 and a row with pre-activations that are exactly 0; gamma carries a 0
  and a negative entry, beta a 0, the upstream gradient a zero row.

Over them: the operators without a rounding compared bit for bit with float64 on inputs in {-1, 0, 1}; the LayerNorm and
BatchNorm operators under ``|got - want| <= K 2^-24 A`` for EVERY element (A: rows_ref's ``magnitude=True``), the
structural zeros exactly; the same with every output and workspace poisoned; rows bitwise independent of the rest of
their batch; outputs bitwise unchanged under a power-of-two rescaling of the rows and eps.

``PYTHONPATH=. python tests/test_hip_row_bounds.py`` measures, on the CPU, the figures K is set from."""
import contextlib
import functools
import math

import pytest
import torch

import rows_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24
LN_EPS = 1e-5
WIDTHS = (4, 64, 260, 520, 1024)
ROW_COUNTS = (1, 7, 150)
LADDER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 129)
POW2_LADDER = (0, 1, 2, 4, 8, 16, 32, 64, 128)

# K of the per-element bound |got - want| <= K 2^-24 A: 4 x the largest |fp32 - float64| / (2^-24 A) of rows_ref's own
# function evaluated in fp32 on the CPU, over every output and gradient element of every case of test_rounded_operators
# (measured by this file's __main__; [measured]).  The factor 4 covers the device's division and square root differing
# from the host's by a few ulp, and a different but fixed summation order (the rule of test_hip_visnet_extents.py).
K = {"layer_norm_rows": 52.9,        # [13.20]  (the kernels: 12.39)
     "bias_relu_ln": 18.5,           # [4.61]   (4.34)
     "gather_ln_reduce": 18.8,       # [4.70]   (3.53)
     "incidence_ln_reduce": 34.2,    # [8.53]   (8.53)
     "batch_norm_rows": 66.5}        # [16.61]  (7.94)


# ----------------------------------------------------------------------------------------------------------------------
# the degree ladder
# ----------------------------------------------------------------------------------------------------------------------
class Ladder:
    """v, e int64 [nnz]: the node and the hyperedge row of each incidence; N node rows, M hyperedge rows."""

    def __init__(self, v, e, N, M, rungs):
        self.v, self.e, self.N, self.M, self.rungs = v, e, N, M, rungs
        self.nnz = v.numel()
        self.deg_v = torch.bincount(v, minlength=N)
        self.deg_e = torch.bincount(e, minlength=M)

    @staticmethod
    def rung(d, rungs):
        """the row (of either side) that carries ladder degree ``d``"""
        return 2 + 3 * rungs.index(d)

    def row(self, d):
        return Ladder.rung(d, self.rungs)

    def tiled(self, copies):
        """``copies`` disjoint copies, one after the other (block-diagonal: no incidence joins two copies)"""
        k = torch.arange(copies).repeat_interleave(self.nnz)
        return Ladder(self.v.repeat(copies) + k * self.N, self.e.repeat(copies) + k * self.M, copies * self.N,
                      copies * self.M, self.rungs)

    def tail(self, copies, keep):
        """(the last ``keep`` of ``copies`` tiled copies as a ladder of their own, first node row, first hyperedge row,
        first incidence)"""
        return self.tiled(keep), (copies - keep) * self.N, (copies - keep) * self.M, (copies - keep) * self.nnz


def _degrees(n_rows, rungs, fill):
    """Row 0, the last row and five rows in the middle empty; ladder degree k at row 2 + 3 k; the rest from ``fill``."""
    deg = [None] * n_rows
    deg[0] = deg[-1] = 0
    for i in range(n_rows // 2, n_rows // 2 + 5):
        deg[i] = 0
    for d in rungs:
        deg[Ladder.rung(d, rungs)] = d
    fillers = [i for i in range(n_rows) if deg[i] is None]
    for k, i in enumerate(fillers):
        deg[i] = fill[k % len(fill)]
    return deg, fillers


def _coprime(start, n):
    while math.gcd(start, n) != 1:
        start += 1
    return start


@functools.lru_cache(maxsize=None)
def ladder(pow2=False, n_nodes=200, n_edges=190):
    rungs = POW2_LADDER if pow2 else LADDER
    fill = (1, 2, 1, 4, 2, 1) if pow2 else (1, 2, 3, 1, 2, 4)
    dv, fv = _degrees(n_nodes, rungs, fill)
    de, fe = _degrees(n_edges, rungs, fill)
    # both sides need one total: raise fillers of the smaller side (by 1; by doubling where every degree is a power of two)
    small, fillers = (de, fe) if sum(de) < sum(dv) else (dv, fv)
    diff = abs(sum(dv) - sum(de))
    for i in reversed(fillers):             # (from the far end: the fillers next to the ladder rows keep their degree)
        if diff == 0:
            break
        step = small[i] if pow2 else 1
        if step <= diff:
            small[i] += step
            diff -= step
    assert diff == 0 and sum(dv) == sum(de)
    nnz = sum(dv)
    stub_v = torch.arange(n_nodes).repeat_interleave(torch.tensor(dv))
    stub_e = torch.arange(n_edges).repeat_interleave(torch.tensor(de))
    j = torch.arange(nnz)
    e_of = stub_e[(j * _coprime(37, nnz) + 11) % nnz]        # node stub j meets a hyperedge stub far from its neighbours'
    order = (j * _coprime(101, nnz) + 5) % nnz               # the order in which the incidences are listed
    return Ladder(stub_v[order].clone(), e_of[order].clone(), n_nodes, n_edges, rungs)


# ----------------------------------------------------------------------------------------------------------------------
# the row menagerie
# ----------------------------------------------------------------------------------------------------------------------
KINDS = ("dead", "one_live", "constant", "times_2^10", "times_2^-10", "plus_100", "size_1e-3", "zeros")


def zero_channels(C):
    return sorted({0, 1, C // 2, C - 1})


def menagerie(R, C, seed, bias=None, places=None, margin=0.5):
    """fp32 [R, C] unit-normal rows h; for (row, kind) in ``places`` (default: kind k at row k) the PRE-ACTIVATION h + bias
    of that row is the special of that kind."""
    z = torch.randn(R, C, generator=torch.Generator().manual_seed(seed))
    b = torch.zeros(C) if bias is None else bias
    places = [(k, KINDS[k]) for k in range(min(R, len(KINDS)))] if places is None else places
    h = z.clone()
    for row, kind in places:
        zr = z[row]
        if kind == "dead":
            t = -(zr.abs() + margin)
        elif kind == "one_live":
            t = -(zr.abs() + margin)
            t[2] = margin + 1.0
        elif kind == "constant":
            t = torch.full((C,), 0.75)
        elif kind == "times_2^10":
            t = zr * 1024.0
        elif kind == "times_2^-10":
            t = zr / 1024.0
        elif kind == "plus_100":
            t = zr + 100.0
        elif kind == "size_1e-3":
            t = 1e-3 * (zr.abs() + 0.1)
        else:
            t = zr.clone()
            t[zero_channels(C)] = 0.0
        h[row] = t - b
    return h


def parameters(C, seed):
    """(bias, gamma, beta): bias in multiples of 1/8 (0.75 - bias and its sum with bias are exact), gamma[1] = 0,
    gamma[2] < 0, beta[3] = 0."""
    gen = torch.Generator().manual_seed(seed)
    bias = (torch.randint(-4, 5, (C,), generator=gen)).float() / 8
    gamma = 1 + 0.2 * torch.randn(C, generator=gen)
    beta = 0.3 * torch.randn(C, generator=gen)
    gamma[1] = 0.0
    gamma[2] = -gamma[2].abs() - 0.25
    beta[3] = 0.0
    return bias, gamma, beta


def upstream(R, C, seed, zero_row=None):
    g = torch.randn(R, C, generator=torch.Generator().manual_seed(seed))
    if zero_row is not None:
        g[zero_row] = 0.0
    return g


def ladder_places(lad, offset=0):
    """Every kind in a long row of the ladder, five of them again in the short ones: the dead row in the hub (degree 129)
    and in the degree-2 row, the 2^10 row in the degree-1 row."""
    long_rows = [(lad.row(d) + offset, k) for d, k in zip((129, 65, 64, 63, 9, 8, 7, 6), KINDS)]
    short_rows = [(lad.row(d) + offset, k) for d, k in zip((1, 2, 3, 4, 5), ("times_2^10", "dead", "plus_100", "one_live",
                                                                              "zeros"))]
    return long_rows + short_rows


# ----------------------------------------------------------------------------------------------------------------------
# cases: the arguments of one call, its reference and what must hold exactly
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """``args``: keyword arguments of rows_ref's function ``fn`` (fp32 CPU tensors and indices); ``dev(args, poison)``
    the same call on the GPU; ``zeros``: (label, key, bool mask) of elements that are exactly 0; ``equals``: (label, key,
    row, fp32 row) of rows given exactly; ``per_row``: the keys whose rows belong to one row of the batch."""

    def __init__(self, label, name, fn, args, dev, zeros=(), equals=(), per_row=()):
        self.label, self.name, self.fn, self.args, self.dev = label, name, fn, args, dev
        self.zeros, self.equals, self.per_row = list(zeros), list(equals), tuple(per_row)

    def reference(self, dtype=torch.float64, magnitude=False):
        return self.fn(**self.args, dtype=dtype, magnitude=magnitude)

    def device(self, poison=False, **changed):
        return self.dev({**self.args, **changed}, poison)


def _pos(pre):
    return pre.double() > 0


def _zero_pre(h, bias):
    """the pre-activations that are exactly 0 (none in a batch of the dead row alone)"""
    zero = h.double() + bias.double() == 0
    return [("pre-activation exactly 0: dh", "dh", zero)] if bool(zero.any()) else []


def dense_case(name, R, C):
    bias, gamma, beta = parameters(C, 1000 + C)
    relu = name == "bias_relu_ln"
    h = menagerie(R, C, 7 * R + C, bias if relu else None)
    g = upstream(R, C, 9 * R + C, zero_row={1: None, 7: 6}.get(R, 9))
    zeros, equals = [], []
    if relu:
        args = dict(h=h, bias=bias, gamma=gamma, beta=beta, g=g, eps=LN_EPS)
        closed = ~_pos(h.double() + bias.double())
        zeros.append(("ReLU closed: dh", "dh", closed))
        zeros += _zero_pre(h, bias)
        equals.append(("dead row: y = beta", "y", 0, beta))
        per_row = ("y", "dh")
    else:
        args = dict(x=h, gamma=gamma, beta=beta, g=g, eps=LN_EPS)
        per_row = ("y", "dx")
    if g.abs().sum(-1).min() == 0:
        zeros.append(("zero upstream row", per_row[1], (g.abs().sum(-1) == 0)[:, None].expand(R, C)))
    return Case(f"{name} R={R} C={C}", name, getattr(rows_ref, name), args, functools.partial(_dev_dense, name), zeros,
                equals, per_row)


def _seg_any(mask, idx, n):
    """[n, C] bool: whether any entry p with idx[p] = i has mask[p]"""
    return torch.zeros(n, mask.shape[1]).index_add_(0, idx, mask.float()) > 0


def gather_case(C, mean, lad=None, places=None):
    lad = ladder() if lad is None else lad
    bias, gamma, beta = parameters(C, 2000 + C)
    h = menagerie(lad.N, C, 11 + C, bias, ladder_places(lad) if places is None else places)
    g = upstream(lad.M, C, 13 + C, zero_row=lad.row(4))
    args = dict(h=h, bias=bias, gamma=gamma, beta=beta, v=lad.v, e=lad.e, n_out=lad.M, g=g, mean=mean, eps=LN_EPS)
    closed = ~_pos(h.double() + bias.double())
    zeros = _zero_pre(h, bias) + [("ReLU closed: dh", "dh", closed),
             ("never gathered: dh", "dh", (lad.deg_v == 0)[:, None].expand(lad.N, C)),
             ("empty output rows", "out", (lad.deg_e == 0)[:, None].expand(lad.M, C))]
    what = "mean" if mean else "sum"
    return Case(f"gather_ln_reduce {what} C={C}", "gather_ln_reduce", rows_ref.gather_ln_reduce, args, _dev_gather, zeros,
                (), ("out", "dh"))


def incidence_case(C, mean, key, lad=None, places=None):
    """``key``: "a" (output rows = node rows), "b" (hyperedge rows) or "sep" (a separate key vector: the node rows again,
    through the general form of the forward).  qb is 0 in the hub hyperedge and in the hyperedges of the special node
    rows (all of them where the row's degree is <= 2, else the first), so those incidences' pre-activation is the special row itself."""
    lad = ladder() if lad is None else lad
    _, gamma, beta = parameters(C, 3000 + C)
    places = ladder_places(lad) if places is None else places
    pa = menagerie(lad.N, C, 17 + C, None, places, margin=8.5)
    qb = torch.randn(lad.M, C, generator=torch.Generator().manual_seed(19 + C))
    qb[lad.row(129)] = 0.0
    for row, _ in places:
        mine = lad.e[lad.v == row]
        qb[mine if mine.numel() <= 2 else mine[:1]] = 0.0
    by_b = key == "b"
    n_out, okey, deg_o = (lad.M, lad.e, lad.deg_e) if by_b else (lad.N, lad.v, lad.deg_v)
    g = upstream(n_out, C, 23 + C, zero_row=lad.row(4))
    args = dict(pa=pa, qb=qb, gamma=gamma, beta=beta, ia=lad.v, ib=lad.e, okey=okey, n_out=n_out, g=g, mean=mean,
                eps=LN_EPS)
    live = _pos(pa.double()[lad.v] + qb.double()[lad.e]) & (g.abs().sum(-1) > 0)[okey][:, None]
    zeros = [("no open incidence: dpa", "dpa", ~_seg_any(live, lad.v, lad.N)),
             ("no open incidence: dqb", "dqb", ~_seg_any(live, lad.e, lad.M)),
             ("empty output rows", "out", (deg_o == 0)[:, None].expand(n_out, C))]
    equals = []
    if not by_b:        # every incidence of a dead node row gives beta: the row is beta (mean) or its degree times beta (sum)
        for row, kind in places:
            if kind == "dead":
                equals.append((f"dead row {row}", "out", row, beta * (1.0 if mean else float(lad.deg_v[row]))))
    what = "mean" if mean else "sum"
    return Case(f"incidence_ln_reduce {what} key={key} C={C}", "incidence_ln_reduce", rows_ref.incidence_ln_reduce, args,
                functools.partial(_dev_incidence, key), zeros, equals, ("out", "dpa", "dqb"))


BN_SEED = 4000         # (a draw whose fused ReLU is decided far from 0: test_rows_ref_host.py asserts it)


def batch_norm_case(R, C, masked, relu):
    """The statistics over the first rows only with ``masked`` (a padded batch; padded rows reach no loss).  R = 150 has
    129 real rows: two partial chunks of 128 rows, the mask ending in the second."""
    _, gamma, beta = parameters(C, 4000 + C)
    x = menagerie(R, C, BN_SEED + 29 * R + C)
    n_real = {7: 5, 150: 129}[R] if masked else R
    mask = (torch.arange(R) < n_real).float() if masked else None
    g = upstream(R, C, 31 * R + C, zero_row=3)
    g[n_real:] = 0.0
    gen = torch.Generator().manual_seed(37 + C)
    rm, rv = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    args = dict(x=x, mask=mask, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, g=g, relu=relu, momentum=0.1,
                eps=LN_EPS)
    zeros = []
    if masked:
        zeros.append(("padded rows: dx", "dx", (torch.arange(R) >= n_real)[:, None].expand(R, C)))
    label = f"batch_norm_rows{' masked' if masked else ''}{' relu' if relu else ''} R={R} C={C}"
    return Case(label, "batch_norm_rows", rows_ref.batch_norm_rows, args, _dev_batch_norm, zeros)


ROUNDED = {"layer_norm_rows": lambda C: [dense_case("layer_norm_rows", R, C) for R in ROW_COUNTS],
           "bias_relu_ln": lambda C: [dense_case("bias_relu_ln", R, C) for R in ROW_COUNTS],
           "gather_ln_reduce": lambda C: [gather_case(C, mean) for mean in (False, True)],
           "incidence_ln_reduce": lambda C: [incidence_case(C, mean, key) for mean in (False, True) for key in "ab"]
           + [incidence_case(C, True, "sep")],
           "batch_norm_rows": lambda C: [batch_norm_case(R, C, masked, relu) for R in (7, 150) for masked in (False, True)
                                         for relu in (False, True)]}


# ----------------------------------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------------------------------
class _PoisonedWorkspace:
    def __init__(self, make):
        self.make, self.made = make, 0

    def __call__(self, nbytes, device):
        self.made += 1
        return self.make(nbytes, device).fill_(0xFF)         # every float and every double of it a NaN


@contextlib.contextmanager
def _poisoned():
    """Inside: every torch.empty / empty_like of ops.rows and ops.aggregate, and the workspaces they draw, are NaN."""
    from test_hip_visnet_extents import _PoisonedTorch
    from equihgnn_amd.ops import aggregate, rows
    keep = [(m, m.torch, m._workspace) for m in (rows, aggregate)]
    made = []
    try:
        for m, _, ws in keep:
            m.torch, m._workspace = _PoisonedTorch(), _PoisonedWorkspace(ws)
            made.append(m.torch)
        yield
        assert sum(t.made for t in made) > 0
    finally:
        for m, t, ws in keep:
            m.torch, m._workspace = t, ws


def _maybe(poison):
    return _poisoned() if poison else contextlib.nullcontext()


def _leaves(*ts):
    return [t.float().to(DEV).requires_grad_(True) for t in ts]


def _cpu(**named):
    return {k: t.detach().cpu() for k, t in named.items()}


def _csrs(v, e, N, M):
    from equihgnn_amd import ops
    vd, ed = v.to(DEV), e.to(DEV)
    return ops.csr_build(vd, ed, N), ops.csr_build(ed, vd, M)


def _dev_dense(name, a, poison):
    from equihgnn_amd import ops
    g = a["g"].float().to(DEV)
    if name == "layer_norm_rows":
        x, gamma, beta = _leaves(a["x"], a["gamma"], a["beta"])
        with _maybe(poison):
            y = ops.layer_norm_rows(x, gamma, beta, a["eps"])
            y.backward(g)
        return _cpu(y=y, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    h, bias, gamma, beta = _leaves(a["h"], a["bias"], a["gamma"], a["beta"])
    with _maybe(poison):
        y = ops.bias_relu_ln(h, bias, gamma, beta, a["eps"])
        y.backward(g)
    return _cpu(y=y, dh=h.grad, dbias=bias.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _dev_gather(a, poison):
    from equihgnn_amd import ops
    by_v, by_e = _csrs(a["v"], a["e"], a["h"].shape[0], a["n_out"])
    h, bias, gamma, beta = _leaves(a["h"], a["bias"], a["gamma"], a["beta"])
    g = a["g"].float().to(DEV)
    with _maybe(poison):
        out = ops.gather_ln_reduce(h, bias, gamma, beta, by_e, by_v, "mean" if a["mean"] else "sum", a["eps"])
        out.backward(g)
    return _cpu(out=out, dh=h.grad, dbias=bias.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _dev_incidence(key, a, poison):
    from equihgnn_amd import ops
    N, M = a["pa"].shape[0], a["qb"].shape[0]
    by_v, by_e = _csrs(a["ia"], a["ib"], N, M)
    v32, e32 = a["ia"].to(DEV).int(), a["ib"].to(DEV).int()
    okey = {"a": v32, "b": e32, "sep": a["ia"].to(DEV).int()}[key]      # "sep": equal values, another tensor
    pa, qb, gamma, beta = _leaves(a["pa"], a["qb"], a["gamma"], a["beta"])
    g = a["g"].float().to(DEV)
    with _maybe(poison):
        out = ops.incidence_ln_reduce(pa, qb, gamma, beta, v32, e32, by_v, by_e, by_e if key == "b" else by_v, okey,
                                      "mean" if a["mean"] else "sum", a["eps"])
        out.backward(g)
    return _cpu(out=out, dpa=pa.grad, dqb=qb.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _dev_batch_norm(a, poison):
    from equihgnn_amd import ops
    C = a["x"].shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=a["eps"], momentum=a["momentum"])
    with torch.no_grad():
        bn.weight.copy_(a["gamma"]); bn.bias.copy_(a["beta"])
        bn.running_mean.copy_(a["running_mean"]); bn.running_var.copy_(a["running_var"])
    bn.to(DEV).train()
    (x,) = _leaves(a["x"])
    mask = None if a["mask"] is None else a["mask"].float()[:, None].to(DEV)
    assert ops.batch_norm_rows_supported(x, bn)
    with _maybe(poison):
        y = ops.batch_norm_rows(x, mask, bn, relu=a["relu"])
        y.backward(a["g"].float().to(DEV))
    assert int(bn.num_batches_tracked) == 1
    return _cpu(y=y, dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
                running_var=bn.running_var)


# ----------------------------------------------------------------------------------------------------------------------
# a. exact operators
# ----------------------------------------------------------------------------------------------------------------------
def _ints(shape, seed):
    return (torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(seed)) - 1).float()


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert torch.equal(got.double(), want), what


@pytest.mark.parametrize("C", WIDTHS)
def test_exact_operators(C):
    """No rounding: inputs in {-1, 0, 1}; sums on the ladder, means on the ladder whose degrees are powers of two (the
    backward of a mean multiplies by 1 / deg); alpha = 0.5."""
    from equihgnn_amd import ops
    for mean, lad in ((False, ladder()), (True, ladder(pow2=True))):
        red = "mean" if mean else "sum"
        by_v, by_e = _csrs(lad.v, lad.e, lad.N, lad.M)
        v32, e32 = lad.v.to(DEV).int(), lad.e.to(DEV).int()
        X, gM, S, gN = _ints((lad.N, C), 1), _ints((lad.M, C), 2), _ints((lad.nnz, C), 3), _ints((lad.N, C), 4)
        gS = _ints((lad.nnz, C), 5)

        (x,) = _leaves(X)
        out = ops.reduce_gathered(x, by_e, by_v, red)
        out.backward(gM.to(DEV))
        want = rows_ref.reduce_gathered(X, lad.v, lad.e, lad.M, gM, mean)
        _same(out.detach().cpu(), want["out"], ("reduce_gathered", red))
        _same(x.grad.cpu(), want["dsrc"], ("reduce_gathered backward", red))
        assert float(want["dsrc"].abs().max()) > 0

        (s,) = _leaves(S)
        out = ops.reduce_entries(s, by_v, v32, red)
        out.backward(gN.to(DEV))
        want = rows_ref.reduce_entries(S, lad.v, lad.N, gN, mean)
        _same(out.detach().cpu(), want["out"], ("reduce_entries", red))
        _same(s.grad.cpu(), want["dsrc"], ("reduce_entries backward", red))

        if not mean:
            (x,) = _leaves(X)
            out = ops.gather_rows(x, v32, by_v)
            out.backward(gS.to(DEV))
            want = rows_ref.gather_rows(X, lad.v, gS)
            _same(out.detach().cpu(), want["out"], "gather_rows")
            _same(x.grad.cpu(), want["dsrc"], "gather_rows backward")
            assert bool((want["dsrc"][lad.deg_v == 0] == 0).all())

            _same(ops.colsum(gN.to(DEV)).cpu(), rows_ref.colsum(gN)["out"], "colsum")
            for mode in (1, 2):
                _same(ops.colsum(gN.to(DEV), by_v.rowptr, mode).cpu(), rows_ref.colsum(gN, lad.deg_v, mode)["out"],
                      ("colsum", mode))
                x0, b = _leaves(X, _ints((C,), 6))
                out = ops.residual_mix(x0, b, by_v.rowptr, mode, 0.5)
                out.backward(gN.to(DEV))
                want = rows_ref.residual_mix(X, b.detach().cpu(), lad.deg_v, mode, 0.5, gN)
                _same(out.detach().cpu(), want["out"], ("residual_mix", mode))
                _same(x0.grad.cpu(), want["dx0"], ("residual_mix dx0", mode))
                _same(b.grad.cpu(), want["dbias"], ("residual_mix dbias", mode))


# ----------------------------------------------------------------------------------------------------------------------
# b. rounded operators
# ----------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, scale):
    """Largest |got - want| / (2^-24 A); an element with A = 0 must be met exactly (inf otherwise)."""
    err = (got.double() - want).abs()
    r = torch.where(scale > 0, err / (EPS * scale.clamp_min(1e-300)), torch.full_like(err, float("inf")))
    r = torch.where((scale > 0) | (err > 0), r, torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def _exact_checks(case, got):
    for label, key, mask in case.zeros:
        assert int(mask.sum()) > 0, (case.label, label, "the fixture has none")
        assert bool((got[key][mask] == 0).all()), (case.label, label)
    for label, key, row, want in case.equals:
        assert torch.equal(got[key][row], want.float()), (case.label, label)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", list(ROUNDED))
def test_rounded_operators(name, C):
    for case in ROUNDED[name](C):
        got = case.device()
        want = case.reference()
        mag = case.reference(magnitude=True)
        assert set(got) == set(want) == set(mag)
        worst = {}
        for key in want:
            assert got[key].shape == want[key].shape and bool(torch.isfinite(got[key]).all()), (case.label, key)
            worst[key] = _ratio(got[key], want[key], mag[key])         # every element: none is left out
        print(f"{case.label}: |got - want| / (2^-24 A) = " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
        assert max(worst.values()) <= K[name], (case.label, worst, K[name])
        _exact_checks(case, got)


# ----------------------------------------------------------------------------------------------------------------------
# c. poisoned memory
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", list(ROUNDED))
def test_results_land_on_poisoned_memory(name, C):
    """Every output, gradient and workspace the operators allocate is NaN before its kernel runs."""
    for case in ROUNDED[name](C):
        got = case.device(poison=True)
        for key, t in got.items():
            assert bool(torch.isfinite(t).all()), (case.label, key)
        _exact_checks(case, got)


# ----------------------------------------------------------------------------------------------------------------------
# d. rows alone and among neighbours
# ----------------------------------------------------------------------------------------------------------------------
def _rows_of(t, a0):
    return t[a0:] if torch.is_tensor(t) and t.dim() == 2 else t


@pytest.mark.parametrize("C", WIDTHS)
def test_a_row_does_not_depend_on_its_neighbours(C):
    """The second half of a batch as a batch of its own: per-row results (not the parameter gradients) agree bit for bit,
    since each row's summation order is fixed and no accumulator outlives its row.  Dense rows: the last 75 of 150.  The
    ladder: the last half of 2 and of 12 block-diagonal copies; 12 copies are 2400 node rows, where a wavefront of the
    incidence backward owns two consecutive rows and carries its accumulator from one to the next, against 1200 rows
    where it owns one."""
    for name in ("layer_norm_rows", "bias_relu_ln"):
        case = dense_case(name, 150, C)
        whole = case.device()
        part = case.device(**{k: _rows_of(t, 75) for k, t in case.args.items()})
        for key in case.per_row:
            assert torch.equal(whole[key][75:], part[key]), (case.label, key)
    one = ladder()
    for copies in (2, 12):
        lad = one.tiled(copies)
        half, n0, m0, p0 = one.tail(copies, copies // 2)
        assert torch.equal(lad.v[p0:] - n0, half.v) and torch.equal(lad.e[p0:] - m0, half.e)
        places = ladder_places(one, (copies - 1) * one.N)
        places_half = [(row - n0, kind) for row, kind in places]
        cases = [(gather_case(C, mean, lad, places), gather_case(C, mean, half, places_half)) for mean in (False, True)]
        cases += [(incidence_case(C, mean, key, lad, places), incidence_case(C, mean, key, half, places_half))
                  for mean in (False, True) for key in ("a", "b", "sep")]
        for big, small in cases:
            first = {"h": n0, "pa": n0, "qb": m0, "g": m0 if big.args["n_out"] == lad.M else n0}
            changed = {k: big.args[k][first[k]:] for k in first if k in big.args}       # the same values, not a new draw
            whole, part = big.device(), small.device(**changed)
            for key in big.per_row:
                a0 = whole[key].shape[0] - part[key].shape[0]
                assert a0 in (n0, m0) and float(part[key].abs().max()) > 0
                assert torch.equal(whole[key][a0:], part[key]), (big.label, copies, key)


# ----------------------------------------------------------------------------------------------------------------------
# e. scaling by powers of two
# ----------------------------------------------------------------------------------------------------------------------
SCALED = {"layer_norm_rows": (("x",), ("dx",)), "bias_relu_ln": (("h", "bias"), ("dh", "dbias")),
          "gather_ln_reduce": (("h", "bias"), ("dh", "dbias")), "incidence_ln_reduce": (("pa", "qb"), ("dpa", "dqb"))}


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", list(SCALED))
def test_power_of_two_scaling(name, C):
    """Rows (and bias) times 2^6 and 2^-6 with eps times 4^6 and 4^-6: xhat, and with it the output, dgamma and dbeta,
    keeps every bit, and the input gradients are scaled by exactly 2^-6 and 2^6 -- eps enters under the square root and
    nowhere else, and no other constant hides in the kernels."""
    scaled_in, scaled_grad = SCALED[name]
    for case in ROUNDED[name](C):
        base = case.device()
        for s in (2.0 ** 6, 2.0 ** -6):
            got = case.device(eps=case.args["eps"] * s * s, **{k: case.args[k] * s for k in scaled_in})
            for key in base:
                want = base[key] / s if key in scaled_grad else base[key]
                assert torch.equal(got[key], want), (case.label, s, key, float((got[key] - want).abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# the measured figures (CPU)
# ----------------------------------------------------------------------------------------------------------------------
def reference_ratios(case):
    """per key: the largest |fp32 - float64| / (2^-24 A) of the case's reference evaluated in fp32"""
    want, mag, f32 = case.reference(), case.reference(magnitude=True), case.reference(dtype=torch.float32)
    return {key: _ratio(f32[key], want[key], mag[key]) for key in want}


def _measure():
    worst = {}
    for name in ROUNDED:
        for C in WIDTHS:
            for case in ROUNDED[name](C):
                r = reference_ratios(case)
                worst[name] = max(worst.get(name, 0.0), max(r.values()))
                print(f"{case.label}: fp32 reference |fp32 - fp64| / (2^-24 A) = " + ", ".join(f"{k} {v:.2f}" for k, v in r.items()),
                      flush=True)
    print("K measured:", {k: round(v, 2) for k, v in worst.items()}, " x4:", {k: round(4 * v, 1) for k, v in worst.items()})


if __name__ == "__main__":
    _measure()
