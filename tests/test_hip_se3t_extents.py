"""GPU: the se3t_* kernels (csrc/se3t.hip) at training widths, on shaped sender tables, on poisoned outputs, and the whole
front-end against float64 and by symmetry.  The oracle is tests/se3t_ref.py in float64 (pinned to the reference's own float64
run by test_se3t_host.py); cases, bounds and helpers of test_hip_se3t.py unless said otherwise.  Every case counts the calls
of its native entry points (_count of test_hip_grid_trips.py).

What each section reaches in se3t.hip (file lines):

A  test_pair_at_every_kind_of_width: the 64-column loop of k_se3t_pair_fwd, ``for (cb = blockIdx.y; ...; cb += gridDim.y)``
   :133 with gridDim.y = min(cblocks, 4) :526.  O = 80: a full block next to one of 16 columns, whose lanes r_ >= 4 are
   inactive (act / col_ld :135-136, the store skipped :168); O = 256: four blocks = gridDim.y (the training width); O = 272 /
   320: a fifth block on the second trip, ragged / full; O = 1024: four trips (the cap of st_pair_check :501).  The backward
   kernels at the same widths: the O / 16 loop of k_se3t_pair_bwd_h :243 and the Q * 8 * (O / 16) tiles of k_se3t_pair_bwd_g
   :276 over gridDim.y = 8 :554.
B  test_shaped_sender_table: the 16-edge tiles per sender, ``g0 += 16`` :124 / :229 / :280 and st_entry :104, with in-degrees
   0, 1, 15, 16, 17, 31, 32, 33, 48 and 63; the padding lanes of a ragged tile (edge 0 read instead :131-132 / :234, zero
   selected in the inner dimension :291); the in-degree-0 sender (no trip of :280, zeros stored :296 and :309); masked slots
   (st_dsrc :204-214, k_se3t_pool :193).  Run again with perm shuffled inside each sender's segment: an edge's forward row
   and dh row are fixed-order sums over that edge alone, so they must not change by a bit.
C  test_*_on_poisoned_memory: every torch.empty / empty_like of ops/se3t.py and the _workspace it draws from filled with NaN
   where they are made; the B cases, one attention and one NormSE3 case.
D  test_attention_slot_counts: the ``s <= K`` guards of the 17-slot loops :340 / :355 / :360 / :397 / :413 at K = 1, 2, 15
   (and 4, 16), masked slots :346 in every row (ATTN_SEED: how a case's seed is chosen);
   test_attention_with_every_softmax_saturated: the seeds that rule passes over, dl = p (dp - dot) :414 as pure residue.
E  test_norm_widths_and_the_clamp: gridDim.y = ceil(C / 256) with the early return ``c >= C`` :437-438 / :455-456 at C = 1,
   255, 256, 257, 1024 (the feed-forward width at hidden 256), 1280; the clamp fmaxf(.., eps) :444 and ``open`` :468-475 on
   rows of norm 0, 1e-13, 1e-11 and 1e3, compared row by row.
F  test_edge_basis_on_a_lattice: ``ds <= radius`` :55 / :58 at exactly 5 A and just beyond, the count behind meanw :61, the
   zero vector :64-65, the axes, a padded batch's tail.
G  test_front_end_matches_float64: SE3Transformer(dim = C) at C = 64, 80, 256 and N = 2, 16, 17, 18, 40, its seven taps and
   every parameter gradient against se3t_ref.front_end in float64.
H  test_front_end_is_equivariant: three proper rotations with a translation, and a permutation of the atoms; degree-0 taps and
   every gradient invariant, degree-1 taps turned by the rotation itself; the permuted cloud's taps bit for bit.
J  test_pooled_forward_accumulates: ``accumulate`` of k_se3t_pool :194 through the C ABI.
(I, the refusals of the entry points :486-645, needs no GPU: tests/test_cabi.py::test_se3t_argument_validation_without_gpu.)

The bounds of A, B, D and J are TOL of test_hip_se3t.py or bit equality.  The bounds of E (NORM_BOUND), G (FRONT_BOUND), H
(SYMMETRY_BOUND, ILL_CONDITIONED) and of D's saturated cases (SATURATED_K) are MEASURED figures: 4 x the error of the
restatement itself evaluated in fp32 on the CPU on the same inputs, written into those tables below with the measured value
in brackets.
``PYTHONPATH=. python tests/test_hip_se3t_extents.py`` measures them again (CPU only)."""
import contextlib

import pytest
import torch

import se3t_ref
import test_hip_se3t as S
from test_hip_grid_trips import _count, _rel, _summed_limit
from test_hip_se3t import DEV, OFF, TOL, _rand
from test_hip_visnet_extents import _PoisonedTorch

pytestmark = pytest.mark.gpu

TAPS = ("conv_in0", "conv_in1", "block0_0", "block0_1", "block1_0", "block1_1", "front_end")

# E.  Per row: |got - float64| <= bound x the row's largest float64 entry, for ``out`` and ``dx``.  The bound of a class of rows
# is TOL where the restatement in fp32 on the CPU stays within TOL / 4 by the same rule, else 4 x its error ([measured], the
# larger of out and dx over every C and m of the test; 4: the device's erff / sqrtf differ by a few ulp, another summation order).
NORM_BOUND = {"ordinary": TOL,     # [2.7e-07]
              "lone": 3.6e-4,      # [8.92e-05]  the ordinary rows at C = 1: the one scale is negative and nothing larger shares
                                   #             the row, so GELU's tail, 1 + erf(a) by cancellation, is the row's largest entry
              "zero": TOL,         # [9.2e-08]   (out: met exactly)
              "closed": TOL,       # [1.1e-07]   norm 1e-13 < eps
              "open": TOL,         # [1.5e-07]   norm 1e-11 >= eps
              "large": TOL}        # [1.5e-07]   norm 1e3
NORM_ROWS = {"zero": 5, "closed": 9, "open": 13, "large": 21}

# G.  (C, N) -> tap -> bound on max |got - float64| / max |float64|, and "grad": the same for the worst parameter gradient:
# max(1e-5, 4 x the error of se3t_ref.front_end in fp32 on the CPU on the same input) [measured].  At (256, 18) one parameter's
# gradient is what cancellation leaves (ILL_CONDITIONED below) and would set a bound of 9 % for all 130; it has a bound of its
# own, "grad_ill", and "grad" is the worst of the others.
def _front_bound(grad, grad_ill=0.0, **taps):
    return {**{k: 1e-5 for k in TAPS}, **taps, "grad": grad, "grad_ill": grad_ill}


# [measured: the seven taps in the order of TAPS, then the worst gradient]
FRONT_BOUND = {
    (64, 40): _front_bound(1.7e-4),                       # [2.27e-07, 4.01e-07, 5.29e-07, 7.49e-07, 2.08e-06, 7.05e-07, 1.36e-06, 4.17e-05]
    (80, 40): _front_bound(3.4e-5, block1_0=1.1e-5),      # [3.41e-07, 4.04e-07, 6.71e-07, 5.39e-07, 2.74e-06, 8.20e-07, 2.15e-06, 8.51e-06]
    (256, 18): _front_bound(4.1e-3, 9.0e-2),              # [5.85e-07, 4.19e-07, 2.55e-06, 1.84e-06, 1.57e-06, 8.97e-07, 1.70e-06, 1.02e-03;
                                                          #  2.25e-02: the parameter of ILL_CONDITIONED, held to its own figure]
    (64, 2): _front_bound(8.5e-5),                        # [3.55e-07, 2.88e-07, 3.89e-07, 7.96e-07, 7.60e-07, 1.03e-06, 8.07e-07, 2.13e-05]
    (64, 16): _front_bound(3.9e-5, block1_1=1.4e-5),      # [2.10e-07, 4.75e-07, 4.25e-07, 1.19e-06, 1.09e-06, 3.46e-06, 7.26e-07, 9.67e-06]
    (64, 17): _front_bound(5.0e-5)}                       # [3.13e-07, 2.30e-07, 5.76e-07, 4.77e-07, 2.47e-06, 7.61e-07, 1.98e-06, 1.24e-05]

# H.  C -> bound on max |moved - expected| / max |expected| over the three rotations: 4 x what se3t_ref.front_end in fp32 on the
# CPU shows between the same clouds [measured]; "deg0": the degree-0 taps and the output, "deg1": the degree-1 taps,
# "grad": the worst parameter gradient.  The permuted cloud: its taps are the base cloud's, permuted, bit for bit (the
# restatement's are [0]: a row of every product is a fixed-order sum over that atom or edge alone); "perm_grad": every parameter
# gradient, max(1e-5, 4 x [measured]) with G's floor ("perm_ill": the same rule for the parameter of ILL_CONDITIONED, whose
# figure is read apart).  A permutation changes nothing but the order of the sums over atoms and edges: dG sums a sender's
# edges in perm order, the weight gradients sum rows in atom order.
SYMMETRY_BOUND = {                                                # [deg0, deg1, grad, perm_grad, perm_ill]
    64: {"deg0": 1.4e-5, "deg1": 3.6e-6, "grad": 9.0e-5, "perm_grad": 1.8e-5, "perm_ill": 0.0},        # [3.47e-06, 9.05e-07, 2.24e-05, 4.54e-06, -]
    256: {"deg0": 1.6e-5, "deg1": 5.9e-6, "grad": 3.6e-3, "perm_grad": 1.6e-5, "perm_ill": 2.2e-5}}    # [3.92e-06, 1.47e-06, 8.94e-04, 4.08e-06, 5.42e-06]
# The parameter whose gradient the fp32 restatement misses by more than 1e-2 of its largest entry against float64 [2.25e-02]:
# that gradient, 3e-3 at most next to 30 for its neighbours, is what cancellation leaves.  G and H read its figures apart.
ILL_CONDITIONED = {64: (), 256: ("net.blocks.1.0.attn.to_self_k.weights.0",)}
# (The bracketed figures move with torch's thread count; each is the largest seen over several runs of __main__ with different
# counts.  Seen: grad at (64, 40) 3.95e-05 and 4.17e-05; H's grad at C = 64 1.86e-05, 1.98e-05, 2.24e-05; perm_grad at C = 64
# 1.3e-06, 1.9e-06, 4.54e-06 and at C = 256 2.1e-06, 3.22e-06, 4.08e-06; perm_ill 3.85e-06, 5.42e-06; E's ordinary rows 2.7e-07
# and 3.5e-07.)


# ----------------------------------------------------------------------------------------------------------------------
# A. the pair kernels at every kind of width
# ----------------------------------------------------------------------------------------------------------------------
WIDE = [(o, pair) for o in (80, 256, 272, 320) for pair in OFF] + [(1024, (0, 0)), (1024, (1, 1))]


@pytest.mark.parametrize("o,pair", WIDE)
def test_pair_at_every_kind_of_width(o, pair, monkeypatch):
    """I = 32 (the kernels never see I), 37 atoms x 16 slots = 592 edges with a ragged last tile; at O = 1024 21 atoms (the
    float64 per-edge weights of (1, 1) stay under 1 GB).  Edge-level and pooled, forward and the gradients of x, h, W3, b3."""
    calls = _count(monkeypatch, "se3t_pair_fwd", "se3t_pair_bwd")
    worst = S._pair_case(pair, 32, o, 21 if o == 1024 else 37, 16, 61)
    assert calls == {"se3t_pair_fwd": 2, "se3t_pair_bwd": 2}, calls
    print(f"A O={o} pair={pair}: largest error / TOL = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# B. shaped sender tables, C. poisoned outputs
# ----------------------------------------------------------------------------------------------------------------------
SHAPED_DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 48, 63)
ALL_MASKED, ONE_SLOT, ALL_SLOTS = 5, 6, 7


def shaped_table():
    """nbr [64, 16], rows distinct and self-excluded, in which atom i < 10 is the neighbour of SHAPED_DEGREES[i] atoms and
    the other 54 share the remaining 768 entries (15 or 14 each): every receiver, last first, takes the 16 senders with the
    most entries left."""
    n, k = 64, 16
    left = torch.tensor(list(SHAPED_DEGREES) + [15] * 12 + [14] * 42)
    assert int(left.sum()) == n * k
    nbr = torch.empty(n, k, dtype=torch.int64)
    for i in range(n - 1, -1, -1):
        cap = left.clone()
        cap[i] = -1
        pick = torch.argsort(cap, descending=True, stable=True)[:k]
        assert int(left[pick].min()) > 0, i
        left[pick] -= 1
        nbr[i] = pick.roll(i)
    assert int(left.abs().max()) == 0
    return nbr


def shaped_mask():
    mask = torch.rand(64, 16, generator=torch.Generator().manual_seed(81)) < 0.7
    mask[ALL_MASKED] = False
    mask[ONE_SLOT] = False
    mask[ONE_SLOT, 9] = True
    mask[ALL_SLOTS] = True
    return mask


def _shaped_graph():
    """(nbr, mask, rowptr, [perm, perm shuffled inside each sender's segment]) with what the table claims asserted."""
    from equihgnn_amd import ops
    n, k = 64, 16
    nbr, mask = shaped_table(), shaped_mask()
    deg = torch.bincount(nbr.reshape(-1), minlength=n)
    assert deg[:10].tolist() == list(SHAPED_DEGREES) and int(deg.sum()) == n * k
    assert all(len(set(r.tolist())) == k and i not in r.tolist() for i, r in enumerate(nbr))
    cnt = mask.sum(1)
    assert int(cnt[ALL_MASKED]) == 0 and int(cnt[ONE_SLOT]) == 1 and int(cnt[ALL_SLOTS]) == k
    csr = ops.csr_build(nbr.reshape(-1).to(torch.int32).to(DEV), None, n)
    rowptr, perm = csr.rowptr.cpu().long(), csr.perm.cpu().long()
    assert torch.equal(rowptr[1:] - rowptr[:-1], deg) and torch.equal(perm.sort().values, torch.arange(n * k))
    assert torch.equal(nbr.reshape(-1)[perm], torch.repeat_interleave(torch.arange(n), deg))
    g = torch.Generator().manual_seed(82)
    mixed = perm.clone()
    for j in range(n):
        a, b = int(rowptr[j]), int(rowptr[j + 1])
        mixed[a:b] = perm[a:b][torch.randperm(b - a, generator=g)]
    assert not torch.equal(mixed, perm) and torch.equal(nbr.reshape(-1)[mixed], nbr.reshape(-1)[perm])
    return nbr, mask, csr.rowptr, [csr.perm, mixed.to(csr.perm.dtype).to(DEV)]


@contextlib.contextmanager
def _poisoned(allocations):
    """Inside: every torch.empty / empty_like of ops.se3t and every _workspace it draws is filled with NaN where it is made
    (the mechanism of test_hip_visnet_extents); ``allocations`` of them must happen."""
    from equihgnn_amd.ops import se3t as T
    fake = _PoisonedTorch()

    def workspace(nbytes, device, _inner=T._workspace):
        fake.made += 1
        return _inner(nbytes, device).fill_(255)         # 0xFFFFFFFF: a NaN in every float
    keep = (T.torch, T._workspace)
    T.torch, T._workspace = fake, workspace
    try:
        yield
        assert fake.made == allocations, (fake.made, allocations)
    finally:
        T.torch, T._workspace = keep


def _shaped_case(pair, o, poison, monkeypatch):
    from equihgnn_amd import ops
    calls = _count(monkeypatch, "se3t_pair_fwd", "se3t_pair_bwd")
    worst = 0.0
    off, mo, mi, f = OFF[pair]
    n, k, i, seed = 64, 16, 32, 83
    nbr, mask, rowptr, perms = _shaped_graph()
    x = _rand(n, i, mi, seed=seed + 1)
    h = _rand(n, k, 128, seed=seed + 2)
    w3 = (_rand(o * i * f, 128, seed=seed + 3) / 128 ** 0.5).float().double()
    b3 = (_rand(o * i * f, seed=seed + 4) * 0.1).float().double()
    rows = _rand(n, k, 34, seed=seed + 5)
    bas = rows[..., off:off + mo * mi * f].reshape(n, k, mo, mi, f)
    leaves64 = [t.clone().requires_grad_(True) for t in (x, h, w3, b3)]
    edge64 = se3t_ref.pair_kernel_apply(leaves64[1], leaves64[2], leaves64[3], bas, leaves64[0][nbr])
    pool64 = se3t_ref.masked_mean(edge64, mask)
    meanw = (mask.double() / mask.sum(1, keepdim=True).clamp(min=1)).float().to(DEV)
    rows32 = rows.float().to(DEV).reshape(n * k, 34)
    for pooled, ref in ((False, edge64.reshape(n * k, o, mo)), (True, pool64)):
        up = _rand(*ref.shape, seed=seed + 6)
        g64 = torch.autograd.grad((ref * up).sum(), leaves64, retain_graph=True)
        runs = []
        for perm in perms:
            leaves = [t.float().to(DEV).requires_grad_(True) for t in (x, h, w3, b3)]
            xg, hg, wg, bg = leaves
            w, b = S._node_weights(wg, bg, o, i, f)
            xc = xg.transpose(1, 2).reshape(n * mi, i)
            G, GB = xc @ w, xc @ b
            with _poisoned(5) if poison else contextlib.nullcontext():       # out + workspace; dh, dG, dGB
                out = ops.se3t_pair(hg.reshape(n * k, 128), G, GB, rows32, pair, o, rowptr, perm, meanw if pooled else None)
                grads = torch.autograd.grad((out.transpose(1, 2) * up.float().to(DEV)).sum(), leaves + [G, GB])
            out = out.detach().transpose(1, 2)
            worst = max(worst, S._close(out, ref, ("fwd", pooled)))
            for name, a, c in zip("x h w3 b3".split(), g64, grads):
                worst = max(worst, S._close(c, a, ("bwd", name, pooled)))
            for name, t in zip("out x h w3 b3 G GB".split(), (out, *grads)):
                assert bool(torch.isfinite(t).all()), (name, pooled)
            dh, dG, dGB = grads[1].view(n, k, 128), grads[4].view(n, -1), grads[5].view(n, -1)
            assert float(dG[0].abs().max()) == 0 and float(dGB[0].abs().max()) == 0       # nobody's neighbour
            assert float(dG[9].abs().max()) > 0 and float(dGB[9].abs().max()) > 0       # the hub
            if pooled:
                assert float(out[ALL_MASKED].abs().max()) == 0
                assert float(dh[~mask.to(DEV)].abs().max()) == 0
                assert float(dh[mask.to(DEV)].abs().max()) > 0
            runs.append((out, grads[1]))
        # the same edges in another place of their sender's tiles
        if not pooled:
            assert torch.equal(runs[0][0], runs[1][0]), "an edge's forward row depends on its place in the tile"
        assert torch.equal(runs[0][1], runs[1][1]), ("an edge's dh row depends on its place in the tile", pooled)
    assert calls == {"se3t_pair_fwd": 4, "se3t_pair_bwd": 4}, calls
    print(f"B/C O={o} pair={pair} poison={poison}: largest error / TOL = {worst:.3f}")


SHAPED = [(pair, o) for pair in ((0, 1), (1, 1)) for o in (64, 80)]


@pytest.mark.parametrize("pair,o", SHAPED)
def test_shaped_sender_table(pair, o, monkeypatch):
    _shaped_case(pair, o, False, monkeypatch)


@pytest.mark.parametrize("pair,o", SHAPED)
def test_shaped_sender_table_on_poisoned_memory(pair, o, monkeypatch):
    _shaped_case(pair, o, True, monkeypatch)


def test_attention_on_poisoned_memory(monkeypatch):
    calls = _count(monkeypatch, "se3t_attn_fwd", "se3t_attn_bwd")
    with _poisoned(7):                                       # out, logits; five gradients
        mask, g32, _ = S._attn_case(37, 15, 3, False, 21)
    assert calls == {"se3t_attn_fwd": 1, "se3t_attn_bwd": 1}, calls
    _masked_slots_are_zero(mask, g32)


# ----------------------------------------------------------------------------------------------------------------------
# D. attention slot counts
# ----------------------------------------------------------------------------------------------------------------------
def _masked_slots_are_zero(mask, g32):
    for t in g32:
        assert bool(torch.isfinite(t).all())
    dke, dve = g32[2].detach().cpu(), g32[4].detach().cpu()          # [N, K, 64, m]
    assert int((~mask).sum()) > 0 and int(mask.sum()) > 0
    assert float(dke[~mask].abs().max()) == 0 and float(dve[~mask].abs().max()) == 0
    assert float(dke[mask].abs().max()) > 0 and float(dve[mask].abs().max()) > 0


ATTN_SIZES = [(2, 1), (3, 2), (16, 15), (5, 4), (37, 16)]
# The seed of each case: the first from 21 on at which the float64 oracle can judge every tensor by _attn_case's max-norm rule,
# that is, at which the restatement in fp32 on the CPU is within a quarter of _attn_case's bound on the output and on all five
# gradients (_attn_oracle_margin; found by this file's __main__, asserted by the test).  With |logit| ~ 80 and one or two
# rows that have a neighbour at all, most seeds saturate every softmax; dq and dk are then nothing but the rounding residue of
# p (dp - sum p dp), 1e-6 and less of the other gradients, and torch's own fp32 backward is 0.2 to 0.6 of their largest entry
# from float64 (as the kernel is; below 1e-16 float64 loses them as well).  Such a seed says nothing about the kernel.
ATTN_SEED = {**{(nk, m, big): 21 for nk in ATTN_SIZES for m in (1, 3) for big in (False, True)},
             ((2, 1), 1, True): 23, ((3, 2), 1, True): 26, ((16, 15), 3, True): 22}


def _attn_oracle_margin(n, k, m, big, seed):
    """The largest, over the output and the five gradients, of (error of the fp32 restatement on the CPU) / (_attn_case's
    bound); inf if ``big`` does not bring a logit past _attn_case's own 60."""
    mask, ts = S._attn_inputs(n, k, m, big, seed)
    res = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).requires_grad_(True) for t in ts]
        out, sim = se3t_ref.attention_core(*leaves, mask)
        up = _rand(*out.shape, seed=seed + 6).to(dtype)
        res[dtype] = [out.detach(), *torch.autograd.grad((out * up).sum(), leaves)], sim.detach()
    sim = res[torch.float64][1]
    lmax = float(sim[sim > -1e30].abs().max())
    if big and lmax <= 60:
        return float("inf")
    tol = TOL + 4 * lmax * 2.0 ** -24
    return max(float((a.double() - b).abs().max()) / (tol * float(b.abs().max()) + 1e-30)
               for a, b in zip(res[torch.float32][0], res[torch.float64][0]))


def _attn_seed(n, k, m, big):
    return next(seed for seed in range(21, 2000) if _attn_oracle_margin(n, k, m, big, seed) <= 0.25)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("nk", ATTN_SIZES)
def test_attention_slot_counts(nk, m, big, monkeypatch):
    calls = _count(monkeypatch, "se3t_attn_fwd", "se3t_attn_bwd")
    seed = ATTN_SEED[nk, m, big]
    assert _attn_oracle_margin(nk[0], nk[1], m, big, seed) <= 0.25
    mask, g32, worst = S._attn_case(nk[0], nk[1], m, big, seed)
    assert calls == {"se3t_attn_fwd": 1, "se3t_attn_bwd": 1}, calls
    _masked_slots_are_zero(mask, g32)
    print(f"D nk={nk} m={m} big={big}: largest error / bound = {worst:.3f}")


SATURATED = [((2, 1), 1), ((3, 2), 1), ((16, 15), 3)]          # with ``big`` and seed 21: what ATTN_SEED passes over
# |error| <= SATURATED_K x bound x A element by element: 4 x the largest such ratio of the restatement in fp32 on the CPU over
# the three cases [measured: 0.70, dkedge at (16, 15); the bound's 4 |logit| 2^-24 is nearly what a logit's rounding costs]
SATURATED_K = 2.8


def _saturated_reference(n, k, m):
    """(mask, inputs, upstream, bound, float64 output, float64 gradients, [A(dq), A(dkself), A(dkedge)]) of a SATURATED case."""
    scale = 32 ** -0.5
    mask, ts = S._attn_inputs(n, k, m, True, 21)
    l64 = [t.clone().requires_grad_(True) for t in ts]
    ref, sim = se3t_ref.attention_core(*l64, mask)
    sim = sim.detach()
    tol = TOL + 4 * float(sim[sim > -1e30].abs().max()) * 2.0 ** -24
    up = _rand(*ref.shape, seed=27)
    g64 = torch.autograd.grad((ref * up).sum(), l64)
    assert min(float(g.abs().max()) for g in g64[:3]) < 1e-5
    prob = sim.softmax(-1)                                                         # [N, 2, K + 1]
    heads = lambda t: t.reshape(*t.shape[:-2], 2, 32, m)
    keys, vals = (heads(torch.cat((a[:, None], b), 1)) for a, b in ((ts[1], ts[2]), (ts[3], ts[4])))      # [N, K + 1, 2, 32, m]
    dp = torch.einsum("nhdm,njhdm->nhj", heads(up), vals).abs()
    w = scale * prob * (dp + (prob * dp).sum(-1, keepdim=True))
    a_q = torch.einsum("nhj,njhdm->nhdm", w, keys.abs()).reshape(n, 64, m)
    a_k = (w.transpose(1, 2)[..., None, None] * heads(ts[0]).abs()[:, None]).reshape(n, k + 1, 64, m)
    return mask, ts, up, tol, ref.detach(), g64, [a_q, a_k[:, 0], a_k[:, 1:]]


def _saturated_ratios(g32, g64, sizes, tol):
    """The largest |error| / (bound x A) of dq, dkself, dkedge."""
    return {name: float(((got.detach().cpu().double() - want).abs() / (tol * size + 1e-30)).max())
            for name, got, want, size in zip(("q", "kself", "kedge"), g32, g64, sizes)}


@pytest.mark.parametrize("nk,m", SATURATED)
def test_attention_with_every_softmax_saturated(nk, m, monkeypatch):
    """The seeds ATTN_SEED passes over: the softmax of (nearly) every row is one slot to 1e-6 or less, and one or all of dq,
    dkself, dkedge are what p_s (dp_s - sum_t p_t dp_t) leaves, too small for a max-norm rule.  The output and the gradients
    of the values by _attn_case's rule; those three element by element against the size of their terms in float64,
        |error| <= SATURATED_K x bound x A,   A(dq) = scale sum_s p_s (|dp_s| + sum_t p_t |dp_t|) |k_s|,   A(dk_s) = the s-th
    term with |q|,   bound = _attn_case's TOL + 4 |logit| 2^-24   (a masked slot has A = 0: met exactly)."""
    from equihgnn_amd import ops
    n, k = nk
    calls = _count(monkeypatch, "se3t_attn_fwd", "se3t_attn_bwd")
    assert _attn_oracle_margin(n, k, m, True, 21) > 1.0
    mask, ts, up, tol, ref, g64, sizes = _saturated_reference(n, k, m)
    l32 = [t.float().to(DEV).requires_grad_(True) for t in ts]
    cm = lambda t: t.transpose(-1, -2).reshape(-1, m, 64)
    out = ops.se3t_attn(*(cm(t) for t in l32), mask.float().to(DEV), 32 ** -0.5).transpose(1, 2)
    g32 = torch.autograd.grad((out * up.float().to(DEV)).sum(), l32)
    assert calls == {"se3t_attn_fwd": 1, "se3t_attn_bwd": 1}, calls
    S._close(out, ref, "fwd", tol)
    S._close(g32[3], g64[3], "vself", tol)
    S._close(g32[4], g64[4], "vedge", tol)
    _masked_slots_are_zero(mask, g32)
    ratios = _saturated_ratios(g32, g64, sizes, tol)
    print(f"D saturated nk={nk} m={m}: largest error / (bound x A): {ratios} ({SATURATED_K})")
    assert max(ratios.values()) <= SATURATED_K, ratios


# ----------------------------------------------------------------------------------------------------------------------
# E. NormSE3 widths and the clamp
# ----------------------------------------------------------------------------------------------------------------------
NORM_WIDTHS = (1, 255, 256, 257, 1024, 1280)


def _norm_tensors(c, m):
    """x [37, C, m] with the planted rows (each channel's norm over m is the planted one), scale [1, 1, C] with every third
    entry negative, the upstream gradient; float32-representable."""
    x = _rand(37, c, m, seed=71)
    x[NORM_ROWS["zero"]] = 0.0
    for name, size in (("closed", 1e-13), ("open", 1e-11), ("large", 1e3)):
        r = NORM_ROWS[name]
        x[r] = x[r] / x[r].norm(dim=-1, keepdim=True) * size
    s = 1.0 + 0.1 * _rand(1, 1, c, seed=72)
    s[..., ::3] = -s[..., ::3]
    return x.float().double(), s.float().double(), _rand(37, c, m, seed=73)


def _norm_reference(x, s, up, dtype=torch.float64):
    xr, sr = x.to(dtype).requires_grad_(True), s.to(dtype).requires_grad_(True)
    out = se3t_ref.norm_se3(xr, sr)
    dx, ds = torch.autograd.grad((out * up.to(dtype)).sum(), (xr, sr))
    return out.detach(), dx, ds


def _row_classes(got, ref):
    """class -> largest over its rows of max |got - ref| / max |ref| of the row (a row that is zero in ``ref`` must be met
    exactly: inf otherwise)."""
    err = (got.double() - ref).abs().flatten(1).max(1).values
    top = ref.abs().flatten(1).max(1).values
    ratio = torch.where(top > 0, err / top.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    planted = torch.zeros(ref.shape[0], dtype=torch.bool)
    res = {}
    for name, r in NORM_ROWS.items():
        planted[r] = True
        res[name] = float(ratio[r])
    res["lone" if ref.shape[1] == 1 else "ordinary"] = float(ratio[~planted].max())
    return res


def _norm_case(c, m, poison, monkeypatch):
    from equihgnn_amd import ops
    calls = _count(monkeypatch, "se3t_norm_fwd", "se3t_norm_bwd")
    x, s, up = _norm_tensors(c, m)
    out64, dx64, ds64 = _norm_reference(x, s, up)
    assert float(out64[NORM_ROWS["zero"]].abs().max()) == 0 and float(out64[NORM_ROWS["closed"]].abs().max()) > 0
    x32, s32 = x.float().to(DEV).requires_grad_(True), s.float().to(DEV).requires_grad_(True)
    with _poisoned(4) if poison else contextlib.nullcontext():           # out; dx, dscale, the slab workspace
        out = ops.se3t_norm(x32.transpose(1, 2).contiguous(), s32).transpose(1, 2)
        dx, ds = torch.autograd.grad((out * up.float().to(DEV)).sum(), (x32, s32))
    assert calls == {"se3t_norm_fwd": 1, "se3t_norm_bwd": 1}, calls
    xt, st = x.float().to(DEV).requires_grad_(True), s.float().to(DEV).requires_grad_(True)
    gt = torch.autograd.grad((se3t_ref.norm_se3(xt, st) * up.float().to(DEV)).sum(), (xt, st))
    for name, t in (("out", out), ("dx", dx), ("dscale", ds)):
        assert bool(torch.isfinite(t).all()), name
    assert float(out[NORM_ROWS["zero"]].abs().max()) == 0
    figs = {}
    for what, got, ref in (("out", out, out64), ("dx", dx, dx64)):
        for name, v in _row_classes(got.detach().cpu(), ref).items():
            figs[what, name] = v
    print(f"E C={c} m={m}: per-row error / row maximum " + ", ".join(f"{w} {n} {v:.2e}" for (w, n), v in figs.items()))
    for (what, name), v in figs.items():
        assert v <= NORM_BOUND[name], (what, name, v, NORM_BOUND[name])
    lim = _summed_limit(f"se3t_norm C={c} m={m} dscale", TOL, gt[1], ds64)
    err = _rel(ds, ds64)
    print(f"E C={c} m={m} dscale: {err:.2e} (limit {lim:.2e})")
    assert err <= lim, (err, lim)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("c", NORM_WIDTHS)
def test_norm_widths_and_the_clamp(c, m, monkeypatch):
    _norm_case(c, m, False, monkeypatch)


def test_norm_on_poisoned_memory(monkeypatch):
    _norm_case(257, 3, True, monkeypatch)


# ----------------------------------------------------------------------------------------------------------------------
# F. the edge basis on decidable geometry
# ----------------------------------------------------------------------------------------------------------------------
def lattice_cloud():
    """pos float64 [23, 3] on a lattice of 1/4 A (every squared distance of interest is exact in fp32): a pair at exactly
    5 A, a pair at 5.00625 A, a centre with a neighbour along each of +-x, +-y, +-z, two atoms on one point, six scattered
    atoms, and a padded batch's tail (four dummy atoms 10 A apart on a line 1e4 A away)."""
    c = (8.0, 28.0, 8.0)
    pts = [(0.0, 0.0, 0.0), (3.0, 4.0, 0.0),
           (20.0, 0.0, 0.0), (25.0, 0.25, 0.0),
           c, (c[0] + 1.5, c[1], c[2]), (c[0] - 1.25, c[1], c[2]), (c[0], c[1] + 2.0, c[2]), (c[0], c[1] - 2.25, c[2]),
           (c[0], c[1], c[2] + 0.75), (c[0], c[1], c[2] - 1.0),
           (28.0, 28.0, 8.0), (28.0, 28.0, 8.0)]
    g = torch.Generator().manual_seed(91)
    extra = set()
    while len(extra) < 6:
        extra.add(tuple((torch.randint(160, 200, (3,), generator=g).double() * 0.25).tolist()))       # 40 .. 50 A
    pts += sorted(extra)
    pts += [(1.0e4 + 10.0 * i, 0.0, 0.0) for i in range(4)]
    pos = torch.tensor(pts, dtype=torch.float64)
    assert torch.equal(pos.float().double(), pos) and float(pos[:-4].max()) < 64
    return pos


def test_edge_basis_on_a_lattice(monkeypatch):
    from equihgnn_amd import ops
    calls = _count(monkeypatch, "se3t_edge_basis")
    pos = lattice_cloud()
    n = pos.shape[0]
    nbr, dist, mask, rel = se3t_ref.edge_graph(pos)
    k = nbr.shape[1]
    assert k == 16
    # the cloud holds what it claims to
    d2 = rel.pow(2).sum(-1)
    assert bool(((d2 == 25.0) & mask).any()) and bool(((d2 == 25.0625) & ~mask).any())
    for axis in range(3):
        other = [a for a in range(3) if a != axis]
        on_axis = (rel[..., other] == 0).all(-1) & mask
        assert bool((on_axis & (rel[..., axis] > 0)).any()) and bool((on_axis & (rel[..., axis] < 0)).any())
    assert int(((d2 == 0) & mask).sum()) == 2
    assert not bool(mask[-4:].any()) and bool((~mask[:-4]).any())
    with _poisoned(4):                                       # dist, maskf, meanw, basis
        d, maskf, meanw, basis = ops.se3t_edge_basis(pos.float().to(DEV), nbr.to(torch.int32).to(DEV), 5.0, S._qtab())
    assert calls == {"se3t_edge_basis": 1}
    d, maskf, meanw, basis = d.cpu().double().view(n, k), maskf.cpu(), meanw.cpu().double(), basis.cpu().double().view(n, k, 34)
    for name, t in (("dist", d), ("maskf", maskf), ("meanw", meanw), ("basis", basis)):
        assert bool(torch.isfinite(t).all()), name
    assert torch.equal(maskf > 0, mask)                              # every slot: nothing is "near the radius" here
    want_w = mask.double() / mask.sum(1, keepdim=True).clamp(min=1)
    assert float((meanw - want_w).abs().max()) <= 1e-6
    assert float(meanw[-4:].abs().max()) == 0
    err = (basis - S._basis_rows(rel)).abs()
    assert float(err.max()) <= 1e-6, float(err.max())
    near = dist <= 16.0
    assert float((d - dist)[near].abs().max()) <= 1e-5
    assert float(((d - dist).abs() / dist)[~near].max()) <= 1e-6
    assert bool((d[d2 == 25.0] == 5.0).all()) and bool((d[d2 == 0] == 0.0).all())
    print(f"F: basis {float(err.max()):.2e}, dist {float((d - dist)[near].abs().max()):.2e} / "
          f"{float(((d - dist).abs() / dist)[~near].max()):.2e} rel, meanw {float((meanw - want_w).abs().max()):.2e}")


# ----------------------------------------------------------------------------------------------------------------------
# G. the whole front-end at other widths, H. its symmetry
# ----------------------------------------------------------------------------------------------------------------------
FRONT_SHAPES = [(64, 40), (80, 40), (256, 18), (64, 2), (64, 16), (64, 17)]


def rotations():
    """Three proper rotations (QR of seeded matrices, determinant +1), each with a translation."""
    out = []
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        if torch.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        assert abs(float(torch.linalg.det(q)) - 1.0) < 1e-12
        out.append((q, torch.randn(3, generator=g, dtype=torch.float64)))
    return out


def _moved(pos, q, t):
    return (pos @ q.T + t).float().double()                  # (rounded to fp32 again: what the device is given)


def _decidable(pos):
    """In every row the sorted distances differ by more than 1e-4 and none lies within 1e-3 of the radius."""
    n = pos.shape[0]
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    off = ~torch.eye(n, dtype=torch.bool)
    s = d.masked_fill(~off, float("inf")).sort(-1).values[:, :n - 1]
    return (n < 3 or float((s[:, 1:] - s[:, :-1]).min()) > 1e-4) and float((d[off] - 5.0).abs().min()) > 1e-3


def front_cloud(n):
    """The first seeded cloud of n atoms (fp32 values) that is decidable, and stays so with the same neighbour table under
    the three rigid motions; some pairs lie beyond the radius (two atoms: within it)."""
    for seed in range(200):
        pos = (_rand(n, 3, seed=1000 * n + seed) * 2.4).float().double()
        d = (pos[:, None] - pos[None]).norm(dim=-1)
        if (n == 2 and float(d.max()) > 4.0) or (n > 2 and float(d.max()) < 6.0):
            continue
        moved = [_moved(pos, q, t) for q, t in rotations()]
        if not all(_decidable(p) for p in [pos] + moved):
            continue
        nbr, _, mask, _ = se3t_ref.edge_graph(pos)
        assert all(torch.equal(se3t_ref.edge_graph(p)[0], nbr) and torch.equal(se3t_ref.edge_graph(p)[2], mask) for p in moved)
        assert n == 2 or bool((~mask).any())
        return pos
    raise AssertionError("no seed with decidable distances")


def _layer(c):
    from common import fill_state_dict
    from equihgnn_amd.se3_transformer import SE3Transformer
    torch.manual_seed(0)
    m = SE3Transformer(dim=c)
    fill_state_dict(m, 100 + c)
    return m


def _front_inputs(c, n):
    return _rand(n, c, seed=7 * c + n), front_cloud(n), _rand(n, c, seed=7 * c + n + 1)


def _reference_run(m, feats, pos, up, dtype=torch.float64):
    """(taps in the reference's layout [N, C, m] with the output as "front_end", parameter gradients of (out * up).sum())
    of se3t_ref.front_end in ``dtype``."""
    names = [k for k, _ in m.named_parameters()]
    sd = {k: v.detach().to(dtype).clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    taps = {}
    out = se3t_ref.front_end(sd, feats.to(dtype), pos.to(dtype), prefix="", taps=taps)
    (out * up.to(dtype)).sum().backward()
    return {k: v.detach() for k, v in taps.items()}, {k: sd[k].grad for k in names}


class _Spy:
    """Keeps the EdgeBasis objects the layer builds (the neighbour table it really used)."""

    def __init__(self, monkeypatch):
        from equihgnn_amd import se3_transformer as M
        self.seen = seen = []

        class Kept(M.EdgeBasis):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                seen.append(self)
        monkeypatch.setattr(M, "EdgeBasis", Kept)


def _device_run(m, feats, pos, up):
    m.zero_grad(set_to_none=True)
    taps = {}
    out = m(feats.float().to(DEV), pos.float().to(DEV), taps=taps)
    (out * up.float().to(DEV)).sum().backward()
    res = {k: v.detach().transpose(1, 2).cpu() for k, v in taps.items()}
    res["front_end"] = out.detach().cpu()
    return res, {k: p.grad.cpu() for k, p in m.named_parameters()}


def _relerr(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-300))


def _front_figures(got, want, ill=()):
    """tap -> error, "grad": the worst parameter gradient's but for those named in ``ill``, "grad_ill": theirs."""
    (taps, grads), (taps64, grads64) = got, want
    figs = {k: _relerr(taps[k], taps64[k]) for k in TAPS}
    assert sorted(grads) == sorted(grads64) and all(float(g.abs().max()) > 0 for g in grads64.values())
    figs["grad"] = max(_relerr(grads[k], grads64[k]) for k in grads64 if k not in ill)
    figs["grad_ill"] = max((_relerr(grads[k], grads64[k]) for k in ill), default=0.0)
    return figs


FRONT_CALLS = {"se3t_edge_basis": 1, "se3t_pair_fwd": 20, "se3t_pair_bwd": 20, "se3t_attn_fwd": 4, "se3t_attn_bwd": 4,
               "se3t_norm_fwd": 12, "se3t_norm_bwd": 12}


@pytest.mark.parametrize("c,n", FRONT_SHAPES)
def test_front_end_matches_float64(c, n, monkeypatch):
    calls = _count(monkeypatch, *FRONT_CALLS)
    spy = _Spy(monkeypatch)
    feats, pos, up = _front_inputs(c, n)
    m = _layer(c)
    want = _reference_run(m, feats, pos, up)
    got = _device_run(m.to(DEV), feats, pos, up)
    assert calls == FRONT_CALLS, calls
    nbr, _, mask, _ = se3t_ref.edge_graph(pos)
    (geo,) = spy.seen
    assert geo.K == min(16, n - 1) and torch.equal(geo.nbr.cpu().long(), nbr) and torch.equal(geo.maskf.cpu() > 0, mask)
    figs = _front_figures(got, want, ILL_CONDITIONED[c] if (c, n) == (256, 18) else ())
    print(f"G C={c} N={n}: " + ", ".join(f"{k} {v:.2e} ({FRONT_BOUND[c, n][k]:.1e})" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= FRONT_BOUND[c, n][k], (k, v, FRONT_BOUND[c, n][k])


def _symmetry_figures(run, feats, pos, up, ill=()):
    """{"deg0", "deg1", "grad"}: the largest over the three rigid motions of moved against expected (degree-0 taps and the
    output unchanged, degree-1 taps turned by q, every gradient unchanged), and for the permuted cloud "perm": its taps
    (permuted with the atoms), "perm_grad": its gradients (unchanged) but those named in ``ill``, "perm_ill": those."""
    base_t, base_g = run(feats, pos, up)
    figs = {"deg0": 0.0, "deg1": 0.0, "grad": 0.0, "perm": 0.0, "perm_grad": 0.0, "perm_ill": 0.0}

    def fold(moved, perm, expect0, expect1):
        taps, grads = moved
        for k in TAPS:
            key = "perm" if perm else ("deg1" if k.endswith("1") else "deg0")
            want = expect1(base_t[k]) if k.endswith("1") else expect0(base_t[k])
            figs[key] = max(figs[key], _relerr(taps[k], want))
        for k in base_g:
            key = ("perm_ill" if k in ill else "perm_grad") if perm else "grad"
            figs[key] = max(figs[key], _relerr(grads[k], base_g[k]))

    for q, t in rotations():
        fold(run(feats, _moved(pos, q, t), up), False, lambda a: a, lambda a: torch.einsum("ab,ncb->nca", q.to(a.dtype), a))
    p = torch.randperm(pos.shape[0], generator=torch.Generator().manual_seed(4))
    fold(run(feats[p], pos[p], up[p]), True, lambda a: a[p], lambda a: a[p])
    return figs


@pytest.mark.parametrize("c,n", [(64, 40), (256, 18)])
def test_front_end_is_equivariant(c, n, monkeypatch):
    calls = _count(monkeypatch, *FRONT_CALLS)
    spy = _Spy(monkeypatch)
    feats, pos, up = _front_inputs(c, n)
    m = _layer(c)
    if c == 64:                                              # guards the test itself: float64, forward, the first motion
        q, t = rotations()[0]
        sd = {k: v.double() for k, v in m.state_dict().items()}
        a, b = {}, {}
        with torch.no_grad():
            se3t_ref.front_end(sd, feats, pos, prefix="", taps=a)
            se3t_ref.front_end(sd, feats, _moved(pos, q, t), prefix="", taps=b)
        assert _relerr(b["front_end"], a["front_end"]) < 1e-6
        assert _relerr(b["block1_1"], torch.einsum("ab,ncb->nca", q, a["block1_1"])) < 1e-6
    m = m.to(DEV)
    assert set(ILL_CONDITIONED[c]) <= {k for k, _ in m.named_parameters()}
    figs = _symmetry_figures(lambda f, p, u: _device_run(m, f, p, u), feats, pos, up, ILL_CONDITIONED[c])
    assert calls == {k: 5 * v for k, v in FRONT_CALLS.items()}, calls     # the base cloud, three motions, the permuted one
    assert len(spy.seen) == 5
    for g in spy.seen[1:4]:                                  # the same neighbour table and mask under every motion
        assert torch.equal(g.nbr, spy.seen[0].nbr) and torch.equal(g.maskf, spy.seen[0].maskf)
    bound = dict(SYMMETRY_BOUND[c], perm=0.0)
    print(f"H C={c}: " + ", ".join(f"{k} {v:.2e} ({bound[k]:.1e})" for k, v in figs.items()))
    over = {k: (v, bound[k]) for k, v in figs.items() if not v <= bound[k]}
    assert not over, over


# ----------------------------------------------------------------------------------------------------------------------
# J. accumulate = 1
# ----------------------------------------------------------------------------------------------------------------------
def test_pooled_forward_accumulates(monkeypatch):
    """se3t_pair_fwd through the C ABI: the pooled forward added into a filled ``out`` is, bit for bit, that ``out`` plus
    the pooled forward on its own (one fp32 addition per element either way); the latter is what ops.se3t_pair returns."""
    from equihgnn_amd import hip, ops
    from equihgnn_amd.ops._base import _c_void_p, _ptr, _stream
    from equihgnn_amd.ops.se3t import SE3T_PAIRS
    calls = _count(monkeypatch, "se3t_pair_fwd")
    pair, o, n, k = (1, 1), 80, 37, 16
    off, mo, q = SE3T_PAIRS[pair]
    _, mask, csr = S._graph(n, k, 95)
    e = n * k
    h = _rand(e, 128, seed=96).float().to(DEV)
    G = (_rand(n, q * 128 * o, seed=97) * 0.1).float().to(DEV)
    GB = _rand(n, q * o, seed=98).float().to(DEV)
    rows = _rand(e, 34, seed=99).float().to(DEV)
    meanw = (mask.double() / mask.sum(1, keepdim=True).clamp(min=1)).float().to(DEV)
    out0 = _rand(n, mo, o, seed=100).float().to(DEV)
    L = hip.lib()
    need = L.se3t_pair_fwd_workspace_bytes(e, mo, o, 1)
    assert need == e * mo * o * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    res = []
    for accumulate in (0, 1):
        out = out0.clone() if accumulate else torch.full_like(out0, float("nan"))
        ws.fill_(255)
        hip.check(L.se3t_pair_fwd(_ptr(h), _ptr(G), _ptr(GB), _c_void_p(rows.data_ptr() + 4 * off), 34, _ptr(csr.rowptr),
                                  _ptr(csr.perm), n, e, mo, q, o, _ptr(meanw), k, _ptr(out), accumulate, _ptr(ws), need,
                                  _stream(h.device)), "se3t_pair_fwd")
        res.append(out)
    torch.cuda.synchronize()
    pooled, added = res
    assert bool(torch.isfinite(pooled).all()) and float(pooled.abs().max()) > 0 and float(pooled[3].abs().max()) == 0
    assert torch.equal(added, out0 + pooled)
    assert torch.equal(pooled, ops.se3t_pair(h, G, GB, rows, pair, o, csr.rowptr, csr.perm, meanw))
    assert calls == {"se3t_pair_fwd": 3}, calls


# ----------------------------------------------------------------------------------------------------------------------
# the measured figures (CPU)
# ----------------------------------------------------------------------------------------------------------------------
def _measure():
    import time
    worst = {}
    for c in NORM_WIDTHS:
        for m in (1, 3):
            x, s, up = _norm_tensors(c, m)
            o64, dx64, _ = _norm_reference(x, s, up)
            o32, dx32, _ = _norm_reference(x, s, up, torch.float32)
            for got, ref in ((o32, o64), (dx32, dx64)):
                for name, v in _row_classes(got, ref).items():
                    worst[name] = max(worst.get(name, 0.0), v)
    print("NORM_BOUND: fp32 restatement, per-row error / row maximum:", {k: f"{v:.2e}" for k, v in worst.items()},
          " TOL / 4 =", TOL / 4)
    for (n, k), m in SATURATED:
        mask, ts, up, tol, _, g64, sizes = _saturated_reference(n, k, m)
        l32 = [t.float().requires_grad_(True) for t in ts]
        g32 = torch.autograd.grad((se3t_ref.attention_core(*l32, mask)[0] * up.float()).sum(), l32)
        print(f"SATURATED_K ({n}, {k}) m={m}: fp32 restatement, |error| / (bound x A):", _saturated_ratios(g32, g64, sizes, tol))
    print("ATTN_SEED:", {(nk, m, big): _attn_seed(nk[0], nk[1], m, big) for nk in ATTN_SIZES for m in (1, 3) for big in (False, True)})
    for c, n in FRONT_SHAPES:
        t0 = time.time()
        feats, pos, up = _front_inputs(c, n)
        m = _layer(c)
        want = _reference_run(m, feats, pos, up)
        t1 = time.time()
        ill = ILL_CONDITIONED[c] if (c, n) == (256, 18) else ()
        figs = _front_figures(_reference_run(m, feats, pos, up, torch.float32), want, ill)
        top = max(float(want[0][k].abs().max()) for k in TAPS)
        print(f"FRONT_BOUND ({c}, {n}): fp32 restatement " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
              + f"   largest tap entry {top:.1f}; float64 {t1 - t0:.1f} s")
        print(f"    ({c}, {n}): {{" + ", ".join(f'"{k}": {max(1e-5, float(f"{4 * v:.2g}")):.1e}' for k, v in figs.items()) + "},")
    for c, n in ((64, 40), (256, 18)):
        feats, pos, up = _front_inputs(c, n)
        m = _layer(c)
        for dtype in (torch.float32, torch.float64):
            figs = _symmetry_figures(lambda f, p, u: _reference_run(m, f, p, u, dtype), feats, pos, up, ILL_CONDITIONED[c])
            print(f"SYMMETRY_BOUND {c} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))      # common (as conftest.py adds it)
    _measure()
