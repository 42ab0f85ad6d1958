"""GPU: the vis_* kernels at training sizes, at every kind of width, and by symmetry.

The row kernels launch min(N, 16384) workgroups and stride over the rest, so a batch of more than 16384 atoms is the
first to run a second pass of that loop.  ``lattice_batch`` builds such batches: molecules of 1, 2, 15, 16, 17 and 40
atoms plus synth_molecule ones, on a lattice of 1/4 A (every squared distance is exact in fp32, so the strict d2 < 25
is decided alike in fp32 and float64, pairs at exactly 5 A included).  Over them:

* the radius graph and its geometry against visnet_ref, the by-source lists, zeros in empty slots of poisoned outputs;
* the two operators without a transcendental (neighbour sum, edge embedding) bit for bit against float64 on inputs in
  {-1, 0, 1} and a dyadic cutoff;
* the attention, vector and edge-update operators under a per-element bound ``k 2^-24 A``, A the float64 sum of the
  absolute values of the element's terms (visnet_ref's references with ``magnitude=True``), k from ROUNDING_K;
* every output and gradient poisoned (NaN) before its kernel runs: finite everywhere, exactly 0 in the rows of empty slots;
* rows of the third grid pass bitwise equal to the same molecules in a batch of one pass.

The whole front-end is turned and shifted (test_front_end_is_equivariant), and the edge update, which the model's zero
start of ``vec`` silences in the first layer, is driven end to end (test_edge_update_reaches_the_gradients).

``PYTHONPATH=. python tests/test_hip_visnet_extents.py`` measures, on the CPU, the figures ROUNDING_K and SYMMETRY_BOUND are set
from."""
import contextlib

import numpy as np
import pytest
import torch

import visnet_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 16
EPS = 2.0 ** -24
GRID_CAP = 16384
CAP_SIZES = (GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 40000)
WIDTHS = (8, 72, 128, 320, 512)

# k of the per-element bound |got - want| <= k 2^-24 A: 4 x the largest |fp32 - float64| / (2^-24 A) of the float64
# reference itself evaluated in fp32 on the CPU, over every output and gradient element of every case of
# test_rounded_operators (measured by this file's __main__; [measured]).  The factor 4 covers the device's expf and
# division differing from the host's by a few ulp, and a different but fixed summation order.
ROUNDING_K = {"attn": 68.0,      # [16.89]  (the kernels: 15.8)
              "vec": 27.0,       # [6.72]   (6.7)
              "eupd": 23.0}      # [5.71]   (6.2)

# Rotated against unrotated, max-norm relative: 4 x what visnet_ref.visnet in fp32 on the CPU shows on the same two
# batches (measured by this file's __main__; [measured]).
SYMMETRY_BOUND = {
    64: {"x": 6.9e-6, "out": 3.0e-6, "vec1": 2.4e-6, "vec2": 3.0e-6, "grad": 1.2e-5},      # [1.7e-6, 7.6e-7, 5.9e-7, 7.6e-7, 3.0e-6]
    128: {"x": 2.6e-6, "out": 2.2e-6, "vec1": 1.2e-6, "vec2": 1.0e-6, "grad": 1.0e-5}}     # [6.5e-7, 5.5e-7, 3.1e-7, 2.6e-7, 2.6e-6]


# ----------------------------------------------------------------------------------------------------------------------
# batches
# ----------------------------------------------------------------------------------------------------------------------
def lattice_batch(N, seed, n_real=None):
    """(pos fp32 [N, 3], batch int64 [N], rowptr int64 [B + 1]): molecules of mixed size on a lattice of 1/4 A around the
    origin, the points of one molecule distinct.  Two-atom molecules sit alternately at exactly 5 A, offset (3, 4, 0): no
    edge, and at (3, 3.75, 0): an edge; the 40-atom ones fill a box of 5 A, so the 16-slot truncation binds, low atoms
    are kept by more than 16 targets and high ones keep atoms that do not keep them.  Atoms past ``n_real`` are one more
    molecule, all on one far point (a padded batch's tail)."""
    from equihgnn_amd.batch import synth_molecule
    rng = np.random.default_rng(seed)
    n_real = N if n_real is None else n_real
    kinds = (1, 2, 15, 16, 17, 40, 0, 0)
    mols, total, two = [], 0, 0

    def box(n, side):
        pts = set()
        while len(pts) < n:
            pts.add(tuple(int(v) for v in rng.integers(0, side + 1, size=3)))
        p = np.array(sorted(pts), dtype=np.float64)
        return rng.permutation(p) * 0.25 - side * 0.125

    while total < n_real:
        kind = kinds[len(mols) % len(kinds)]
        if kind == 0:
            p = np.round(synth_molecule(rng, "qm9").pos.astype(np.float64) * 4) / 4
            _, first = np.unique(p, axis=0, return_index=True)
            p = p[np.sort(first)]
        elif kind == 2:
            p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0 if two % 2 == 0 else 3.75, 0.0]])
            two += 1
        else:
            p = box(kind, 20 if kind == 40 else 24)
        if total + len(p) > n_real:
            p = box(n_real - total, 24)
        mols.append(p)
        total += len(p)
    if n_real < N:
        mols.append(np.full((N - n_real, 3), 3.0e4))
    pos = torch.from_numpy(np.concatenate(mols, 0).astype(np.float32))
    sizes = torch.tensor([len(p) for p in mols])
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    return pos, torch.repeat_interleave(torch.arange(len(mols)), sizes), rowptr


def _smearing():
    from equihgnn_amd.visnet import ExpNormalSmearing
    return ExpNormalSmearing(5.0, 32)


def _reference_graph(pos, batch, n_real=None):
    """(slot [N, 16], cnt [N], src, dst, eid) of visnet_ref.radius_graph."""
    N = pos.shape[0]
    src, dst = visnet_ref.radius_graph(pos, batch, n_real=n_real)
    cnt = torch.bincount(dst, minlength=N)
    first = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)[:-1]])
    eid = dst * K + (torch.arange(dst.numel()) - first[dst])
    slot = torch.full((N * K,), -1, dtype=torch.int64)
    slot[eid] = src
    return slot.view(N, K), cnt, src, dst, eid


def _reference_geometry(pos, src, dst):
    """float64 (r, cut, rbf, sh) of the kept edges."""
    de = _smearing()
    p = pos.double()
    vec = p[src] - p[dst]
    w = vec.norm(dim=-1)
    mask = src != dst
    rbf = visnet_ref._cut(w).unsqueeze(-1) * torch.exp(-de.betas.double() * (torch.exp(-w).unsqueeze(-1)
                                                                             - de.means.double()) ** 2)
    vec[mask] = vec[mask] / w[mask].unsqueeze(-1)
    return w, visnet_ref._cut(w), rbf, visnet_ref._sphere(vec)


def _cpu_edges(pos, batch, n_real=None):
    """visnet_ref.EdgeList of the reference graph with the geometry rounded to fp32, as the kernels hold it."""
    N = pos.shape[0]
    _, _, src, dst, eid = _reference_graph(pos, batch, n_real)
    _, cut, _, sh = _reference_geometry(pos, src, dst)
    cut_s = torch.zeros(N * K, dtype=torch.float64)
    cut_s[eid] = cut.float().double()
    sh_s = torch.zeros(N * K, 8, dtype=torch.float64)
    sh_s[eid] = sh.float().double()
    return visnet_ref.EdgeList(N, src, dst, eid, cut_s, sh_s)


# ----------------------------------------------------------------------------------------------------------------------
# poisoned memory
# ----------------------------------------------------------------------------------------------------------------------
class _PoisonedTorch:
    """torch, as ops.visnet sees it, with empty / empty_like filled: NaN (floating) or -7 (integer).  The caching
    allocator hands a freed block of NaNs back only now and then (it splits and merges blocks), so the ops' uninitialised
    outputs are poisoned where they are made."""

    def __init__(self):
        self.made = 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _fill(self, t):
        self.made += 1
        return t.fill_(float("nan") if t.is_floating_point() else -7)

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


@contextlib.contextmanager
def _poisoned(allocations):
    """Inside: every torch.empty / empty_like of ops.visnet is poisoned; ``allocations`` of them must happen."""
    from equihgnn_amd.ops import visnet as V
    keep, V.torch = V.torch, _PoisonedTorch()
    try:
        yield
        assert V.torch.made == allocations, (V.torch.made, allocations)
    finally:
        V.torch = keep


# ----------------------------------------------------------------------------------------------------------------------
# A. the graph
# ----------------------------------------------------------------------------------------------------------------------
def _device_graph(pos, batch, rowptr, n_real=None, poison=False):
    from equihgnn_amd import ops
    de = _smearing().to(DEV)
    nr = None if n_real is None else torch.tensor([n_real], dtype=torch.int32, device=DEV)
    args = (pos.to(DEV), batch.to(DEV, torch.int32), rowptr.to(DEV, torch.int32), nr, de.means, de.betas, 5.0)
    with _poisoned(9) if poison else contextlib.nullcontext():
        return ops.radius_graph(*args)


@pytest.mark.parametrize("N,n_real", [(n, None) for n in CAP_SIZES] + [(GRID_CAP + 1, GRID_CAP - 90)])
def test_radius_graph_across_the_grid_cap(N, n_real):
    pos, batch, rowptr = lattice_batch(N, N, n_real)
    g = _device_graph(pos, batch, rowptr, n_real, poison=True)
    slot, cnt, src, dst, eid = _reference_graph(pos, batch, n_real)
    assert torch.equal(g.slot.cpu().long(), slot)
    assert torch.equal(g.cnt.cpu().long(), cnt)
    # the batch exercises what it claims to
    src_cnt = torch.bincount(src, minlength=N)
    assert int(cnt.max()) == K and int(cnt.min()) == 1 and int(src_cnt.max()) > K
    key = dst * N + src
    assert bool((~torch.isin(src * N + dst, key)).any()), "no edge kept one way only"
    p = pos.double()
    d2 = (p[src] - p[dst]).pow(2).sum(-1)
    assert float(d2.max()) < 25.0
    five = torch.tensor([3.0, 4.0, 0.0], dtype=torch.float64)
    two = torch.nonzero(rowptr[1:] - rowptr[:-1] == 2).reshape(-1)
    at5 = two[((p[rowptr[two] + 1] - p[rowptr[two]]) == five).all(-1)]
    assert at5.numel() > 0 and bool((cnt[rowptr[at5]] == 1).all())          # exactly 5 A: not an edge
    if n_real is not None:
        assert bool((cnt[n_real:] == 1).all()) and torch.equal(slot[n_real:, 0], torch.arange(n_real, N))
    # geometry, element by element (the bounds of test_radius_graph_and_geometry)
    w, cut, rbf, sh = _reference_geometry(pos, src, dst)
    r_d, cut_d, rbf_d, sh_d = g.r.cpu(), g.cut.cpu(), g.rbf.cpu(), g.sh.cpu()
    torch.testing.assert_close(r_d[eid].double(), w, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cut_d[eid].double(), cut, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rbf_d[eid].double(), rbf, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(sh_d[eid].double(), sh, rtol=1e-5, atol=1e-5)
    empty = torch.ones(N * K, dtype=torch.bool)
    empty[eid] = False
    assert int(empty.sum()) > 0
    for name, t in (("r", r_d), ("cut", cut_d), ("rbf", rbf_d), ("sh", sh_d)):
        assert bool(torch.isfinite(t).all()), name
        assert bool((t[empty] == 0).all()), name
    # by source: the edges of source j are src_eid[src_start[j] : src_start[j] + src_cnt[j]], ascending, every kept edge once
    starts, counts, lst = g.src_start.cpu().long(), g.src_cnt.cpu().long(), g.src_eid.cpu().long()
    assert torch.equal(counts, src_cnt)
    order = torch.argsort(starts, stable=True)
    assert int(starts.min()) >= 0 and int((starts + counts).max()) <= N * K
    assert bool((starts[order][1:] >= (starts + counts)[order][:-1]).all())         # disjoint ranges
    by_src = torch.argsort(src, stable=True)                                        # eid ascends within a source
    first = torch.cat([torch.zeros(1, dtype=torch.int64), src_cnt.cumsum(0)[:-1]])
    where = starts[src[by_src]] + (torch.arange(src.numel()) - first[src[by_src]])
    assert torch.equal(lst[where], eid[by_src])


# ----------------------------------------------------------------------------------------------------------------------
# B. the operators
# ----------------------------------------------------------------------------------------------------------------------
# name -> (op, reference, inputs, outputs, hidden outputs); a shape is (rows, trailing dims in units of C); an input also
# says whether it is the raw argument of an activation (not made non-negative for the magnitude run)
def _ops():
    from equihgnn_amd import ops
    n, e, n8, e2 = ("n", (1,)), ("e", (1,)), ("n", (8, 1)), ("e", (2,))
    return {"nbr": (ops.vis_neighbor_sum, visnet_ref.nbr_ref, [(n, 0), (e, 0)], [n], []),
            "eemb": (ops.vis_edge_embed, visnet_ref.eemb_ref, [(n, 0), (e, 0)], [e], []),
            "attn": (ops.vis_attn, visnet_ref.attn_ref, [(n, 0), (n, 0), (n, 0), (e, 1), (e, 1)], [e, n], [8]),
            "vec": (ops.vis_vec_msg, visnet_ref.vec_ref, [(n8, 0), (e2, 1)], [n8], []),
            "eupd": (ops.vis_edge_update, visnet_ref.eupd_ref, [(n8, 0), (n8, 0), (e, 1)], [e], [])}


def _shape(spec, N, C):
    rows, dims = spec
    return (N if rows == "n" else K * N, *[d * C if i == len(dims) - 1 else d for i, d in enumerate(dims)])


def _draw(shape, seed, exact):
    gen = torch.Generator().manual_seed(seed)
    if exact:
        return (torch.randint(0, 3, shape, generator=gen) - 1).double()
    return torch.randn(*shape, generator=gen, dtype=torch.float32).double()      # fp32 values: what the device is given


def _case_tensors(name, N, C, exact, seed=0):
    _, _, ins, outs, _ = _ops()[name]
    xs = [_draw(_shape(s, N, C), seed + 10 + i, exact) for i, (s, _) in enumerate(ins)]
    ups = [_draw(_shape(s, N, C), seed + 100 + i, exact) for i, s in enumerate(outs)]
    return xs, ups


def _reference(name, G, xs, ups, dtype=torch.float64, magnitude=False, chunk=4096, rowptr=None):
    """(outputs, input gradients) of the plain-torch reference in ``dtype``, molecule range by molecule range (no edge
    leaves a molecule) so that no [edges, 8, C] intermediate of the whole batch is held."""
    _, ref, ins, _, _ = _ops()[name]
    G = G.to(dtype)
    N = G.N
    cuts = [0, N] if rowptr is None else _chunks(rowptr, N, chunk)
    outs, grads = None, None
    for a0, a1 in zip(cuts[:-1], cuts[1:]):
        sub = G if (a0, a1) == (0, N) else G.rows(a0, a1)

        def part(t):
            return t[a0:a1] if t.shape[0] == N else t[K * a0:K * a1]

        leaves = []
        for t, (_, raw) in zip(xs, ins):
            t = part(t).to(dtype)
            leaves.append((t.abs() if magnitude and not raw else t).clone().requires_grad_(True))
        o = ref(sub, *leaves, magnitude=magnitude)
        o = o if isinstance(o, tuple) else (o,)
        up = [part(u).to(dtype) for u in ups]
        torch.autograd.backward(o, [u.abs() if magnitude else u for u in up])
        o = [t.detach() for t in o]
        gr = [t.grad for t in leaves]
        outs = [[t] for t in o] if outs is None else [a + [t] for a, t in zip(outs, o)]
        grads = [[t] for t in gr] if grads is None else [a + [t] for a, t in zip(grads, gr)]
    return [torch.cat(a) for a in outs], [torch.cat(a) for a in grads]


def _chunks(rowptr, N, chunk):
    cuts = [0]
    for b in rowptr.tolist()[1:]:
        if b - cuts[-1] >= chunk or b == N:
            cuts.append(b)
    return cuts


def _device(name, g, xs, ups, poison=True):
    """(outputs, input gradients) of the op on the GPU, every output and gradient the op allocates poisoned first."""
    op, _, ins, outs, hidden = _ops()[name]
    x32 = [t.float().to(DEV).requires_grad_(True) for t in xs]
    up32 = [t.float().to(DEV) for t in ups]
    with _poisoned(len(outs) + len(hidden)) if poison else contextlib.nullcontext():
        out = op(*x32, g)
    out = out if isinstance(out, tuple) else (out,)
    with _poisoned(len(ins) + len(hidden)) if poison else contextlib.nullcontext():
        torch.autograd.backward(out, up32)
    res = [t.detach().cpu() for t in out], [t.grad.cpu() for t in x32]
    del x32, up32, out
    return res


def _empty_rows(G):
    empty = torch.ones(G.E, dtype=torch.bool)
    empty[G.eid] = False
    return empty


def _finite_and_zero(name, G, got, what):
    """Every element finite; rows of empty slots (per-edge tensors) exactly 0."""
    empty = _empty_rows(G)
    for i, t in enumerate(got):
        assert bool(torch.isfinite(t).all()), (name, what, i)
        if t.shape[0] == G.E:
            assert bool((t[empty] == 0).all()), (name, what, i, "rows of empty slots")


def _edges_of(g):
    ei, eid = g.edge_index()
    return visnet_ref.EdgeList(g.N, ei[0].cpu(), ei[1].cpu(), eid.cpu(), g.cut.cpu().double(), g.sh.cpu().double())


def _lattice_graph(N, seed, n_real=None):
    pos, batch, rowptr = lattice_batch(N, seed, n_real)
    return _device_graph(pos, batch, rowptr, n_real), rowptr


def _dyadic_cut(g, seed):
    """The graph with cut replaced by multiples of 1/4 in (0, 1] on the kept slots (0 on the empty ones, as the header
    promises the kernels)."""
    from equihgnn_amd import ops
    gen = torch.Generator().manual_seed(seed)
    cut = torch.randint(1, 5, (K * g.N,), generator=gen).float() / 4
    cut = (cut * (g.slot.reshape(-1).cpu() >= 0)).to(DEV)
    return ops.RadiusGraph(**{**g.__dict__, "cut": cut})


EXACT_SHAPES = [(n, 64) for n in CAP_SIZES] + [(17000, 256)] + [(300, c) for c in WIDTHS]


@pytest.mark.parametrize("N,C", EXACT_SHAPES)
@pytest.mark.parametrize("name", ["nbr", "eemb"])
def test_exact_operators(name, N, C):
    """No transcendental: inputs in {-1, 0, 1} and a dyadic cutoff make every product and every sum exact in fp32."""
    g, rowptr = _lattice_graph(N, N + C)
    g = _dyadic_cut(g, N)
    G = _edges_of(g)
    xs, ups = _case_tensors(name, N, C, exact=True)
    got_o, got_g = _device(name, g, xs, ups)
    want_o, want_g = _reference(name, G, xs, ups, rowptr=rowptr)
    _finite_and_zero(name, G, got_o, "output")
    _finite_and_zero(name, G, got_g, "gradient")
    for i, (a, b) in enumerate(zip(got_o, want_o)):
        assert torch.equal(a.double(), b), (name, "output", i)
    for i, (a, b) in enumerate(zip(got_g, want_g)):
        assert float(b.abs().max()) > 0
        assert torch.equal(a.double(), b), (name, "gradient", i)


def _ratio(got, want, scale):
    """Largest |got - want| / (2^-24 A); an element with A = 0 must be met exactly (inf otherwise)."""
    err = (got.double() - want).abs()
    r = torch.where(scale > 0, err / (EPS * scale.clamp_min(1e-300)), torch.full_like(err, float("inf")))
    return float(torch.where((scale > 0) | (err > 0), r, torch.zeros_like(err)).max())


# C = 256 at 17000 atoms for vis_attn only: the float64 references of the two [N, 8, C] operators take most of a minute
# there, and their width-dependent paths are the 300-atom cases'
ROUNDED_SHAPES = ([(name, n, 64) for name in ("attn", "vec", "eupd") for n in CAP_SIZES] + [("attn", 17000, 256)]
                  + [(name, 300, c) for name in ("attn", "vec", "eupd") for c in WIDTHS])


@pytest.mark.parametrize("name,N,C", ROUNDED_SHAPES)
def test_rounded_operators(name, N, C):
    g, rowptr = _lattice_graph(N, N + C)
    G = _edges_of(g)
    xs, ups = _case_tensors(name, N, C, exact=False)
    got_o, got_g = _device(name, g, xs, ups)
    want_o, want_g = _reference(name, G, xs, ups, rowptr=rowptr)
    mag_o, mag_g = _reference(name, G, xs, ups, magnitude=True, rowptr=rowptr)
    _finite_and_zero(name, G, got_o, "output")
    _finite_and_zero(name, G, got_g, "gradient")
    k = ROUNDING_K[name]
    worst = {}
    for what, got, want, mag in (("output", got_o, want_o, mag_o), ("gradient", got_g, want_g, mag_g)):
        for i, (a, b, s) in enumerate(zip(got, want, mag)):
            assert a.shape == b.shape
            worst[what, i] = _ratio(a, b, s)
            if C % 64:                                       # the last channel sits in a partial lane round
                assert _ratio(a[..., -1], b[..., -1], s[..., -1]) <= k, (name, what, i, "last channel")
            # the max-norm check of test_operator_pairs_against_float64
            assert float((a.double() - b).abs().max()) <= 2e-5 * (float(b.abs().max()) + 1e-30) + 1e-7, (name, what, i)
    print(f"{name} N={N} C={C}: |got - want| / (2^-24 A) = " + ", ".join(f"{w}{i} {v:.2f}" for (w, i), v in worst.items()))
    assert max(worst.values()) <= k, (worst, k)


@pytest.mark.parametrize("name", ["nbr", "eemb", "attn", "vec", "eupd"])
def test_rows_do_not_depend_on_the_grid_pass(name):
    """The molecules at the end of a 40000-atom batch (rows of the third pass of the grid-stride loop) against the same
    molecules as a batch of their own (one pass): the summation order is per row and fixed, so every bit agrees."""
    N, C = 40000, 64
    pos, batch, rowptr = lattice_batch(N, N + C)
    a0 = int(rowptr[rowptr <= N - 1500].max())
    assert a0 > 2 * GRID_CAP and N - a0 < GRID_CAP
    xs, ups = _case_tensors(name, N, C, exact=False)
    big_o, big_g = _device(name, _device_graph(pos, batch, rowptr), xs, ups, poison=False)
    tail = rowptr[rowptr >= a0] - a0

    def part(t):
        return t[a0:] if t.shape[0] == N else t[K * a0:]

    small = _device_graph(pos[a0:], batch[a0:] - batch[a0], tail)
    small_o, small_g = _device(name, small, [part(t) for t in xs], [part(t) for t in ups], poison=False)
    for i, (a, b) in enumerate(zip(big_o + big_g, small_o + small_g)):
        assert torch.equal(part(a), b), (name, i)


# ----------------------------------------------------------------------------------------------------------------------
# D. symmetry of the whole front-end
# ----------------------------------------------------------------------------------------------------------------------
def _rotation():
    """A proper rotation (determinant +1) and a translation."""
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64))
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)


def _symmetry_batches(C):
    """A crafted batch (test_hip_visnet._batch) and its rotated, shifted copy (positions rounded to fp32 once), both
    with every candidate pair more than 1e-3 A^2 from the cutoff, so both give one and the same graph."""
    from test_hip_visnet import _batch, _margin
    R, t = _rotation()
    for seed in range(300 + C, 340 + C):
        b, _, _ = _batch(seed)
        b2, _, _ = _batch(seed)
        b2.pos64 = b.pos.double() @ R.t() + t               # (what the float64 guard of the test itself is given)
        b2.pos = b2.pos64.float()
        if _margin(b.pos, b.batch) > 1e-3 and _margin(b2.pos, b2.batch) > 1e-3:
            assert torch.equal(visnet_ref.radius_graph(b.pos, b.batch), visnet_ref.radius_graph(b2.pos, b2.batch))
            return b, b2, R
    raise AssertionError("no seed with a safe margin")


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _l2_products(vec):
    """Inner products of the l = 2 block between neighbouring channels of one atom: [N, C - 1]."""
    v = vec[:, 3:8, :]
    return (v[:, :, 1:] * v[:, :, :-1]).sum(1)


def _symmetry_figures(run, b, b2, R):
    """Rotated against unrotated, for ``run(batch) -> (out, x, vec, grads)``: x and out invariant, the l = 1 block (x, y,
    z as k_vis_geom orders them) turned by R, the l = 2 block's inner products invariant, every parameter gradient of
    one invariant loss invariant."""
    out, x, vec, grads = run(b)
    out2, x2, vec2, grads2 = run(b2)
    turned = torch.einsum("ab,nbc->nac", R.to(vec.dtype), vec[:, 0:3, :])
    return {"x": _rel(x2, x), "out": _rel(out2, out), "vec1": _rel(vec2[:, 0:3, :], turned),
            "vec2": _rel(_l2_products(vec2), _l2_products(vec)),
            "grad": max(_rel(grads2[n], grads[n]) for n in grads if float(grads[n].abs().max()) > 0)}


def _invariant_loss(out, x, vec):
    gen = torch.Generator().manual_seed(5)
    w_o = torch.randn(out.shape, generator=gen, dtype=torch.float64).to(out)
    w_x = torch.randn(x.shape, generator=gen, dtype=torch.float64).to(out)
    return (out * w_o).sum() + (x * w_x).sum() + vec[:, 0:3, :].pow(2).sum() + _l2_products(vec).sum()


def _reference_run(m, dtype):
    names = dict(m.named_parameters())

    def run(b):
        sd = {k: v.detach().to(dtype).clone().requires_grad_(k in names) if v.is_floating_point() else v
              for k, v in m.state_dict().items()}
        pos = getattr(b, "pos64", b.pos) if dtype == torch.float64 else b.pos
        out, x, vec = visnet_ref.visnet(sd, b.x, pos, b.batch, dtype=dtype, with_repr=True)
        _invariant_loss(out, x, vec).backward()
        return out.detach(), x.detach(), vec.detach(), {n: sd[n].grad for n in names}
    return run


def _device_run(m):
    from test_hip_visnet import _index

    def run(b):
        bd = b.to(DEV)
        m.zero_grad(set_to_none=True)
        idx = _index(bd)
        x, vec = m.representation_model(bd.x, bd.pos, idx)
        out = m.output_model.pre_reduce(x, vec) * m.std
        _invariant_loss(out, x, vec).backward()
        return out.detach().cpu(), x.detach().cpu(), vec.detach().cpu(), {n: p.grad.cpu() for n, p in m.named_parameters()}
    return run


@pytest.mark.parametrize("C", [64, 128])
def test_front_end_is_equivariant(C):
    from test_hip_visnet import _visnet
    b, b2, R = _symmetry_batches(C)
    m = _visnet(C, seed=C)
    exact = _symmetry_figures(_reference_run(m, torch.float64), b, b2, R)       # guards the test itself
    assert max(exact.values()) < 1e-10, exact
    got = _symmetry_figures(_device_run(m.to(DEV)), b, b2, R)
    print(f"C={C}: rotated against unrotated {got}")
    for key, bound in SYMMETRY_BOUND[C].items():
        assert got[key] <= bound, (key, got[key], bound)


def test_wrapper_is_invariant():
    """visnet_equihnns through the registry, as test_rigid_motion_invariance does for egnn_equihnns (its bound)."""
    import equihgnn_amd.models  # noqa: F401  (registers the classes)
    from common import fill_state_dict
    from equihgnn_amd.registry import default_args, registry
    b, b2, _ = _symmetry_batches(64)
    torch.manual_seed(0)
    m = registry.get_model_class("visnet_equihnns")(1, default_args(MLP_hidden=64, output_hidden=32))
    visnet_ref.fill_visnet_model(m, 5, fill_state_dict)
    m.to(DEV).eval()
    with torch.no_grad():
        a = m(b.to(DEV))
        c = m(b2.to(DEV))
    assert float(a.abs().max()) > 1e-3
    np.testing.assert_allclose(c.cpu().numpy(), a.cpu().numpy(), atol=2e-4)


# ----------------------------------------------------------------------------------------------------------------------
# E. the edge update end to end
# ----------------------------------------------------------------------------------------------------------------------
def _edge_update_model(C, num_layers):
    from equihgnn_amd.visnet import ViSNet
    torch.manual_seed(C + num_layers)
    m = ViSNet(hidden_channels=C, lmax=2, max_num_neighbors=16, num_layers=num_layers)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return m


@pytest.mark.parametrize("num_layers,layer,start", [(2, 0, "given"), (3, 1, "zero")])
def test_edge_update_reaches_the_gradients(num_layers, layer, start):
    """vec starts at zero, so the first layer's edge update has wt = ws = 0: df = 0 and the gradients of its w_src_proj,
    w_trg_proj and f_proj are exactly 0 at any depth.  Two cases where an edge update works on a non-zero vec and its
    df reaches the loss through the next layer's dk_proj / dv_proj: the representation model's own modules in the order
    of ViSNetBlock.forward with two layers, started from a given non-zero vec (layer 0's edge update), and the
    representation model as it is with three layers (layer 1's; layer 0's three gradients are then exactly 0)."""
    from test_hip_visnet import _batch, _index, _margin
    from equihgnn_amd import ops
    C = 64
    b, _, _ = _batch(66)
    assert _margin(b.pos, b.batch) > 1e-3
    N = b.x.shape[0]
    m = _edge_update_model(C, num_layers)
    gen = torch.Generator().manual_seed(9)
    vec0 = 0.5 * torch.randn(N, 8, C, generator=gen).double() if start == "given" else None
    w_x = torch.randn(N, C, generator=gen, dtype=torch.float64)
    w_v = torch.randn(N, 8, C, generator=gen, dtype=torch.float64)
    names = dict(m.named_parameters())
    sd = {k: v.detach().double().clone().requires_grad_(k in names) if v.is_floating_point() else v
          for k, v in m.state_dict().items()}
    _, x64, vec64 = visnet_ref.visnet(sd, b.x, b.pos, b.batch, num_layers=num_layers, with_repr=True, vec0=vec0)
    ((x64 * w_x).sum() + (vec64 * w_v).sum()).backward()

    m = m.to(DEV)
    bd = b.to(DEV)
    rm = m.representation_model
    if start == "given":
        g = _index(bd).radius(bd.pos, rm.cutoff, rm.max_num_neighbors, rm.distance_expansion.means,
                              rm.distance_expansion.betas)
        x = rm.neighbor_embedding(bd.x, rm.embedding(bd.x), g)
        vec = vec0.float().to(DEV)
        f = rm.edge_embedding(x, g)
        for lay in rm.vis_mp_layers:
            dx, dvec, df = lay(x, vec, f, g)
            x, vec = x + dx, vec + dvec
            f = f + df if df is not None else f
        x = ops.layer_norm_rows(x, rm.out_norm.weight, rm.out_norm.bias, rm.out_norm.eps)
    else:
        x, vec = rm(bd.x, bd.pos, _index(bd))
    ((x * w_x.float().to(DEV)).sum() + (vec * w_v.float().to(DEV)).sum()).backward()
    assert _rel(x.detach().cpu(), x64.detach()) < 1e-3 and _rel(vec.detach().cpu(), vec64.detach()) < 1e-3
    pre = "representation_model.vis_mp_layers."
    for n, p in m.named_parameters():
        if not n.startswith("representation_model."):
            continue
        want = sd[n].grad
        edge_update = any(n == f"{pre}{l}.{w}.{s}" for l in range(num_layers - 1)
                          for w, s in (("w_src_proj", "weight"), ("w_trg_proj", "weight"), ("f_proj", "weight"),
                                       ("f_proj", "bias")))
        if edge_update and (start == "given" or int(n[len(pre)]) >= 1):
            assert float(want.abs().max()) > 0 and float(p.grad.abs().max()) > 0, n
        if float(want.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, n
            continue
        assert _rel(p.grad.cpu(), want) < 5e-3, (n, _rel(p.grad.cpu(), want))      # test_front_end_matches_float64_reference's
    for w in ("w_src_proj.weight", "w_trg_proj.weight", "f_proj.weight"):
        assert float(names[f"{pre}{layer}.{w}"].grad.abs().max()) > 0, w


# ----------------------------------------------------------------------------------------------------------------------
# the measured figures (CPU)
# ----------------------------------------------------------------------------------------------------------------------
def _measure():
    import time
    worst = {}
    for name, N, C in ROUNDED_SHAPES:
        t0 = time.time()
        pos, batch, rowptr = lattice_batch(N, N + C)
        G = _cpu_edges(pos, batch)
        xs, ups = _case_tensors(name, N, C, exact=False)
        o64, g64 = _reference(name, G, xs, ups, rowptr=rowptr)
        oa, ga = _reference(name, G, xs, ups, magnitude=True, rowptr=rowptr)
        o32, g32 = _reference(name, G, xs, ups, dtype=torch.float32, rowptr=rowptr)
        each = [round(_ratio(a, b, s), 2) for a, b, s in zip(o32 + g32, o64 + g64, oa + ga)]
        r = max(each)
        print(each)
        worst[name] = max(worst.get(name, 0.0), r)
        print(f"{name} N={N} C={C}: fp32 reference |fp32 - fp64| / (2^-24 A) = {r:.3f}   ({time.time() - t0:.1f} s)", flush=True)
    print("ROUNDING_K measured:", {k: round(v, 3) for k, v in worst.items()}, " x4:", {k: round(4 * v, 2) for k, v in worst.items()})
    from test_hip_visnet import _visnet
    for C in (64, 128):
        b, b2, R = _symmetry_batches(C)
        m = _visnet(C, seed=C)
        f32 = _symmetry_figures(_reference_run(m, torch.float32), b, b2, R)
        f64 = _symmetry_figures(_reference_run(m, torch.float64), b, b2, R)
        print(f"SYMMETRY C={C}: fp32 reference {f32}\n   x4: { {k: float(f'{4 * v:.2g}') for k, v in f32.items()} }\n   float64 {f64}")


if __name__ == "__main__":
    _measure()
