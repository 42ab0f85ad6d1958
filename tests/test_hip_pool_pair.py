"""GPU: the paired pool hg_pool_pair_fwd / hg_pool_pair_bwd (csrc/pool_pair.hip) and ops.pool_pair against float64 torch,
on its special cases, on poisoned outputs, on both sides of its grid caps, and against the read-out it replaces.

Tolerance against float64: atol = rtol = 1e-5, the bound tests/test_hip_kernels.py:105,112 holds hg_segment_reduce_f32's
sums (and their backward gather) to on randn rows.  That test's segments average 4 rows; the segments here are molecules
of up to 64 rows, so the absolute part is scaled by sqrt(rows / 4), the growth of a float32 running sum's rounding error
with its length.  The grid-cap tests use rows of small integers, whose sums are exact in float32: they compare bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = RTOL = 1e-5          # tests/test_hip_kernels.py:105,112
REF_SEGMENT = 4             # ... at 1500 entries over 380 non-empty rows


def _ops():
    from equihgnn_amd import ops
    return ops


def _index(batch, n_e):
    """What ops.pool_pair reads of a HyperIndex, from ``batch`` [N] and ``n_e`` [B] alone (int64, on the device)."""
    ops = _ops()
    B = n_e.shape[0]
    e_mol = torch.repeat_interleave(torch.arange(B, device=n_e.device), n_e)
    pool, he = ops.csr_build(batch, None, B), ops.csr_build(e_mol, None, B)
    return SimpleNamespace(pool=pool, batch32=batch.to(torch.int32), N=int(batch.shape[0]),
                           hyperedge_pool=lambda _n_e: (he, e_mol.to(torch.int32))), e_mol


def _case(seed, B, C, max_atoms=40, p_high=0.3, no_edges=()):
    """Random molecules: 1..max_atoms atoms, 0..max_atoms hyperedges of which a share ``p_high`` has order 3..8 (the
    molecules ``no_edges`` none at all), randn rows."""
    g = torch.Generator().manual_seed(seed)
    n_atoms = torch.randint(1, max_atoms + 1, (B,), generator=g)
    n_e = torch.randint(0, max_atoms + 1, (B,), generator=g)
    for b in no_edges:
        n_e[b] = 0
    N, M = int(n_atoms.sum()), int(n_e.sum())
    batch = torch.repeat_interleave(torch.arange(B), n_atoms)
    order = torch.where(torch.rand(M, generator=g) < p_high, torch.randint(3, 9, (M,), generator=g), torch.full((M,), 2))
    return batch, n_e, order, torch.randn(N, C, generator=g), torch.randn(M, C, generator=g), torch.randn(B, 2 * C, generator=g)


def _ref(x, e, batch, e_mol, order, B):
    """float64: [sum of x rows per molecule | sum of e rows of order > 2 per molecule]"""
    C = x.shape[1]
    keep = order > 2
    left = torch.zeros(B, C, dtype=torch.float64).index_add(0, batch, x)
    right = torch.zeros(B, C, dtype=torch.float64).index_add(0, e_mol[keep], e[keep])
    return torch.cat((left, right), -1)


def _check(batch, n_e, order, x, e, w, longest):
    ops = _ops()
    B = n_e.shape[0]
    index, e_mol = _index(batch.to(DEV), n_e.to(DEV))
    xd, ed = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    out = ops.pool_pair(xd, ed, index, n_e.to(DEV), order.to(DEV))
    (out * w.to(DEV)).sum().backward()
    x64, e64 = x.double().requires_grad_(True), e.double().requires_grad_(True)
    ref = _ref(x64, e64, batch, e_mol.cpu(), order, B)
    (ref * w.double()).sum().backward()
    atol = ATOL * max(1.0, longest / REF_SEGMENT) ** 0.5
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"pool_pair B={B} C={x.shape[1]} N={x.shape[0]} M={e.shape[0]}: max |out - float64| = {err:.2e} (atol {atol:.1e})")
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=atol, rtol=RTOL)
    # the backward is a copy of float32 values: the float64 gradient of these float32 weights is the same number
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.numpy(), atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(ed.grad.cpu().numpy(), e64.grad.numpy(), atol=ATOL, rtol=RTOL)
    assert float(ed.grad[(order <= 2).to(DEV)].abs().max() if bool((order <= 2).any()) else 0.0) == 0.0
    return out.detach(), ref.detach()


@pytest.mark.parametrize("C", [64, 256, 300, 4, 1024])
def test_pool_pair_matches_float64(C):
    _check(*_case(C, 97, C), longest=40)


def test_molecules_without_high_order_hyperedges_and_without_any():
    """Molecules 3 and 96 (the last) have no hyperedge at all; with p_high = 0.02 most of the others have none of order > 2:
    their right halves are exactly zero."""
    batch, n_e, order, x, e, w = _case(5, 97, 64, p_high=0.02, no_edges=(3, 96))
    out, ref = _check(batch, n_e, order, x, e, w, longest=40)
    empty = (ref[:, 64:].abs().max(1).values == 0)
    assert bool(empty[3]) and bool(empty[96]) and int(empty.sum()) > 20
    assert float(out[empty.to(DEV), 64:].abs().max()) == 0.0


def test_empty_hyperedge_pool():
    """No hyperedge in the whole batch: e is [0, C]; the right half is zero and de is an empty tensor."""
    batch, n_e, order, x, e, w = _case(6, 33, 256, no_edges=range(33))
    assert e.shape[0] == 0
    out, _ = _check(batch, n_e, order, x, e, w, longest=40)
    assert float(out[:, 256:].abs().max()) == 0.0


def test_long_segments_take_the_64_entry_rounds():
    """Molecules of up to 200 rows: several rounds of 64 entries per wavefront, the last one partial."""
    _check(*_case(7, 19, 64, max_atoms=200, p_high=0.5), longest=200)


def _raw_fwd(x, pool_rowptr, pool_perm, e, he_rowptr, he_perm, order, out, B, C):
    from equihgnn_amd import hip
    from equihgnn_amd.ops import _ptr, _stream
    return hip.lib().hg_pool_pair_fwd(_ptr(x), _ptr(pool_rowptr), _ptr(pool_perm), x.shape[0], _ptr(e), _ptr(he_rowptr),
                                      _ptr(he_perm), _ptr(order), e.shape[0], _ptr(out), B, C, _stream(x.device))


def _raw_bwd(dout, x_mol, e_mol, order, dx, de, B, C):
    from equihgnn_amd import hip
    from equihgnn_amd.ops import _ptr, _stream
    return hip.lib().hg_pool_pair_bwd(_ptr(dout), _ptr(x_mol), dx.shape[0], _ptr(e_mol), _ptr(order), de.shape[0], _ptr(dx),
                                      _ptr(de), B, C, _stream(dout.device))


def test_null_entries_and_poisoned_outputs():
    """Hand-made CSRs with null entries (-1) and entries past the row count, molecule ids that are negative or >= B in the
    backward: they count as zero rows, and every entry of NaN-filled outputs is written."""
    C, B, N, M = 64, 5, 23, 17
    g = torch.Generator().manual_seed(8)
    x, e = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    order = torch.tensor([2, 3, 5, 2, 2, 4, 2, 8, 3, 2, 2, 2, 6, 2, 3, 2, 7])
    # molecule 1 is empty on both sides; entries -1 and N + 3 / M + 1 are null
    x_perm = torch.tensor([0, 1, -1, 2, 3, 4, N + 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, -1])
    x_rowptr = torch.tensor([0, 6, 6, 12, 20, 26])
    e_perm = torch.tensor([0, 1, 2, -1, 3, 4, 5, 6, 7, M + 1, 8, 9, 10, 11, 12, 13, 14, 15, 16])
    e_rowptr = torch.tensor([0, 5, 5, 9, 10, 19])
    d = lambda t, dt=None: (t if dt is None else t.to(dt)).to(DEV)
    out = torch.full((B, 2 * C), float("nan"), device=DEV)
    assert _raw_fwd(d(x), d(x_rowptr, torch.int32), d(x_perm, torch.int32), d(e), d(e_rowptr, torch.int32),
                    d(e_perm, torch.int32), d(order), out, B, C) == 0
    ref = torch.zeros(B, 2 * C, dtype=torch.float64)
    for b in range(B):
        for q in range(int(x_rowptr[b]), int(x_rowptr[b + 1])):
            j = int(x_perm[q])
            if 0 <= j < N:
                ref[b, :C] += x[j].double()
        for q in range(int(e_rowptr[b]), int(e_rowptr[b + 1])):
            j = int(e_perm[q])
            if 0 <= j < M and int(order[j]) > 2:
                ref[b, C:] += e[j].double()
    assert not bool(torch.isnan(out).any())
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=ATOL * 2 ** 0.5, rtol=RTOL)
    assert float(out[1].abs().max()) == 0.0
    # identity perm (NULL) = the entries themselves
    out2 = torch.full((B, 2 * C), float("nan"), device=DEV)
    rp = torch.tensor([0, 6, 6, 12, 20, N]), torch.tensor([0, 5, 5, 9, 10, M])
    assert _raw_fwd(d(x), d(rp[0], torch.int32), None, d(e), d(rp[1], torch.int32), None, d(order), out2, B, C) == 0
    xm = torch.repeat_interleave(torch.arange(B), rp[0].diff())
    em = torch.repeat_interleave(torch.arange(B), rp[1].diff())
    np.testing.assert_allclose(out2.cpu().numpy(), _ref(x.double(), e.double(), xm, em, order, B).numpy(),
                               atol=ATOL * 2 ** 0.5, rtol=RTOL)
    # backward
    dout = torch.randn(B, 2 * C, generator=g)
    x_mol, e_mol = xm.clone(), em.clone()
    x_mol[2], x_mol[7], e_mol[1], e_mol[8] = -1, B, -3, B + 2
    dx, de = torch.full((N, C), float("nan"), device=DEV), torch.full((M, C), float("nan"), device=DEV)
    assert _raw_bwd(d(dout), d(x_mol, torch.int32), d(e_mol, torch.int32), d(order), dx, de, B, C) == 0
    want_x = torch.where(((x_mol >= 0) & (x_mol < B))[:, None], dout[x_mol.clamp(0, B - 1), :C], torch.zeros(()))
    want_e = torch.where(((e_mol >= 0) & (e_mol < B) & (order > 2))[:, None], dout[e_mol.clamp(0, B - 1), C:], torch.zeros(()))
    assert torch.equal(dx.cpu(), want_x) and torch.equal(de.cpu(), want_e)


def test_padded_batch_matches_the_unpadded_one_and_the_read_out_it_replaces():
    """A pad_batch-padded batch through HyperIndex (the pad molecule owns the padded atoms and hyperedges, whose e_order is
    0): the real molecules' rows equal the unpadded batch's bit for bit; and ops.pool_pair equals the mask-multiply / two
    reduces / cat path of the other paired models on the same inputs, values and both input gradients."""
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import pool_sum
    ops = _ops()
    C = 256
    b = synth_batch(24, 4321, "pcqm")
    p = pad_batch(b, *bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz, 128))
    g = torch.Generator().manual_seed(9)
    outs = {}
    for tag, data in (("plain", b), ("padded", p)):
        data = data.to(DEV)
        index = HyperIndex.from_batch(data)
        N, M, B = data.x.shape[0], data.edge_attr.shape[0], data.y.shape[0]
        g.manual_seed(9)
        x, e, w = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g), torch.randn(B, 2 * C, generator=g)
        if tag == "padded":       # the same rows for the real atoms / hyperedges
            x[:b.num_nodes], e[:b.num_hyperedges], w[:24] = outs["plain"][3], outs["plain"][4], outs["plain"][5]
        xd, ed = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
        out = ops.pool_pair(xd, ed, index, data.n_e, data.e_order)
        (out * w.to(DEV)).sum().backward()
        # the path it replaces (models._PairedBase._pool with fused_pool False)
        x2, e2 = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
        he_csr, he_key = index.hyperedge_pool(data.n_e)
        keep = (data.e_order > 2).to(e2.dtype).unsqueeze(-1)
        old = torch.cat((pool_sum(x2, index), ops.reduce_entries(e2 * keep, he_csr, he_key, "sum")), -1)
        (old * w.to(DEV)).sum().backward()
        print(f"pool_pair vs the replaced path ({tag}): max |d out| = {float((out - old).abs().max()):.2e}, "
              f"max |d dx| = {float((xd.grad - x2.grad).abs().max()):.2e}, max |d de| = {float((ed.grad - e2.grad).abs().max()):.2e}")
        atol = ATOL * (60 / REF_SEGMENT) ** 0.5           # PCQM-like molecules: up to 60 atoms
        np.testing.assert_allclose(out.detach().cpu().numpy(), old.detach().cpu().numpy(), atol=atol, rtol=RTOL)
        np.testing.assert_allclose(xd.grad.cpu().numpy(), x2.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)
        np.testing.assert_allclose(ed.grad.cpu().numpy(), e2.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)
        ref = _ref(x.double(), e.double(), data.batch.cpu(), he_key.cpu().long(), data.e_order.cpu(), B)
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref.numpy(), atol=atol, rtol=RTOL)
        outs[tag] = (out.detach().cpu(), xd.grad.cpu(), ed.grad.cpu(), x, e, w)
    assert torch.equal(outs["padded"][0][:24], outs["plain"][0])
    assert float(outs["padded"][0][24, C:].abs().max()) == 0.0          # the pad molecule's hyperedges have order 0
    assert torch.equal(outs["padded"][1][:b.num_nodes], outs["plain"][1])
    assert torch.equal(outs["padded"][2][:b.num_hyperedges], outs["plain"][2])
    assert float(outs["padded"][2][b.num_hyperedges:].abs().max()) == 0.0


def test_pool_pair_is_deterministic():
    batch, n_e, order, x, e, _ = _case(10, 300, 256)
    index, _ = _index(batch.to(DEV), n_e.to(DEV))
    a = _ops().pool_pair(x.to(DEV), e.to(DEV), index, n_e.to(DEV), order.to(DEV))
    for _ in range(3):
        assert torch.equal(a, _ops().pool_pair(x.to(DEV), e.to(DEV), index, n_e.to(DEV), order.to(DEV)))


# The forward launches one wavefront per (molecule, half), four per workgroup, at most 4096 workgroups (grid-stride beyond):
# 8192 molecules fill that grid exactly; 131 070 molecules would be workgroup 65 535 of an uncapped grid.  The backward
# launches 256 >> log2(lanes per row) rows per workgroup (16 at C = 64), at most 4096 workgroups: 65 536 rows fill it,
# 16 x 65 535 rows would be the last workgroup of an uncapped grid.
@pytest.mark.parametrize("B", [8192, 8193, 131070, 131073], ids=["fills_grid", "past_grid", "block_65535", "past_65535"])
def test_forward_around_its_grid_caps(B):
    C = 64
    g = torch.Generator().manual_seed(B)
    n_atoms = torch.randint(1, 4, (B,), generator=g)
    n_e = torch.randint(0, 3, (B,), generator=g)
    n_atoms[-1], n_e[-1] = 3, 2                           # the last molecule (the last wavefront of each half) has rows
    N, M = int(n_atoms.sum()), int(n_e.sum())
    x = torch.randint(-8, 9, (N, C), generator=g).float()
    e = torch.randint(-8, 9, (M, C), generator=g).float()
    order = torch.randint(2, 5, (M,), generator=g)
    order[-1] = 3
    batch = torch.repeat_interleave(torch.arange(B), n_atoms)
    index, e_mol = _index(batch.to(DEV), n_e.to(DEV))
    he, _ = index.hyperedge_pool(None)
    out = torch.full((B, 2 * C), float("nan"), device=DEV)
    assert _raw_fwd(x.to(DEV), index.pool.rowptr, index.pool.perm, e.to(DEV), he.rowptr, he.perm, order.to(DEV), out, B, C) == 0
    ref = _ref(x.double(), e.double(), batch, e_mol.cpu(), order, B)
    assert torch.equal(out.cpu().double(), ref)           # small integers: exact
    assert float(out[-1, C:].abs().max()) > 0


@pytest.mark.parametrize("rows", [65536, 65537, 16 * 65535, 16 * 65535 + 17],
                         ids=["fills_grid", "past_grid", "block_65535", "past_65535"])
def test_backward_around_its_grid_caps(rows):
    C, B = 64, 1000
    g = torch.Generator().manual_seed(rows)
    N = rows // 2
    M = rows - N
    x_mol, e_mol = torch.randint(0, B, (N,), generator=g), torch.randint(0, B, (M,), generator=g)
    order = torch.randint(2, 5, (M,), generator=g)
    order[-1] = 4
    dout = torch.randn(B, 2 * C, generator=g)
    dx, de = torch.full((N, C), float("nan"), device=DEV), torch.full((M, C), float("nan"), device=DEV)
    assert _raw_bwd(dout.to(DEV), x_mol.int().to(DEV), e_mol.int().to(DEV), order.to(DEV), dx, de, B, C) == 0
    assert torch.equal(dx.cpu(), dout[x_mol, :C])
    assert torch.equal(de.cpu(), dout[e_mol, C:] * (order > 2)[:, None])
    assert float(de[-1].abs().max()) > 0


def test_bad_arguments_return_the_error_code():
    from equihgnn_amd import hip
    C, B = 64, 4
    x, e = torch.zeros(16, C, device=DEV), torch.zeros(8, C, device=DEV)
    rp = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    order = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.full((B, 2 * C), 7.0, device=DEV)
    assert _raw_fwd(x, rp, None, e, rp, None, order, out, B, 66) == hip.EQH_ERR_ALIGN
    assert _raw_fwd(x, rp, None, e, rp, None, order, out, B, 1028) == hip.EQH_ERR_RANGE
    assert _raw_fwd(x, rp, None, e, rp, None, order, out, -1, C) == hip.EQH_ERR_ARG
    assert _raw_fwd(x, None, None, e, rp, None, order, out, B, C) == hip.EQH_ERR_ARG
    assert _raw_fwd(x, rp, None, e, rp, None, None, out, B, C) == hip.EQH_ERR_ARG
    assert _raw_fwd(x.view(-1)[1:1 + 8 * C].view(8, C), rp, None, e, rp, None, order, out, B, C) == hip.EQH_ERR_ALIGN
    assert _raw_bwd(out, rp, rp, order, x, e, B, 2) == hip.EQH_ERR_ALIGN
    assert _raw_bwd(out, None, rp, order, x, e, B, C) == hip.EQH_ERR_ARG
    assert _raw_bwd(out, rp, rp, order, x, e, 1 << 30, C) == hip.EQH_ERR_RANGE
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 7.0 and float(x.abs().max()) == 0.0      # nothing was launched
    with pytest.raises(ValueError, match="one width"):
        _ops().pool_pair(x, torch.zeros(8, 2 * C, device=DEV), None, None, order)
