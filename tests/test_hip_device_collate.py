"""GPU: batch.DeviceMolStore / DeviceGraphStore.collate (csrc/collate_dev.hip: a scan launch and a fill launch) against the host
MolStore.collate / GraphStore.collate (csrc/collate.hip) on the same store, idx and pad_to -- every comparison bit for bit and
field by field (never ``_flat``: its alignment gaps are uninitialised on both sides)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H_FIELDS = ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e", "e_order", "batch", "y")
G_FIELDS = ("x", "edge_index", "edge_attr", "batch", "y")
SENTINEL = 0x5A


class Form:
    """One of the two batch forms: its host store, the device copy, its fields and extent rules."""

    def __init__(self, host, fields, sizes, spare):
        self.host, self.fields, self.sizes = host, fields, sizes
        self.dev = host.to_device(DEV)
        self.spare = spare          # what a padded extent needs beyond the batch: (1, 1, 0) / (1, 0)

    def pad_to(self, idx, mode):
        from equihgnn_amd.batch import bucket_sizes, graph_bucket_sizes
        ext = self.host.extents(np.asarray(idx, dtype=np.int64))
        if mode is None:
            return None
        if mode == "min":               # hypergraph (N + 1, M + 1, Z); graph (N + 1, E): pn = 1 and pe = 0
            return tuple(e + s for e, s in zip(ext, self.spare))
        if mode == "bucket":
            return bucket_sizes(*ext, 128) if len(ext) == 3 else graph_bucket_sizes(*ext, 128)
        if mode == "spare300":          # 300 padded atoms (the pos line / a long ring), a few padded incidences / edges
            return (ext[0] + 300, ext[1] + 1, ext[2] + 7) if len(ext) == 3 else (ext[0] + 300, ext[1] + 77)
        if mode == "selfloops":         # graph only: ONE padded atom, nine padded edges
            return ext[0] + 1, ext[1] + 9
        raise KeyError(mode)

    def same(self, got, want, what=""):
        for f in self.fields:
            g, w = getattr(got, f), getattr(want, f)
            assert g.is_cuda and g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, f)
            g = g.cpu()
            if w.dtype == torch.float32:        # bits, not values: -0.0 / NaN payloads would pass torch.equal or fail it
                g, w = g.view(torch.int32), w.view(torch.int32)
            assert torch.equal(g, w), (what, f)
        for s in self.sizes + ("num_graphs",):
            assert getattr(got, s) == getattr(want, s), (what, s)
        assert getattr(got, "num_real_graphs", None) == getattr(want, "num_real_graphs", None), what


@pytest.fixture(scope="module")
def hyper():
    """400 synthetic molecules (half qm9, half pcqm) and three hand-made ones: 400 a single atom without hyperedge or
    incidence, 401 a molecule whose only hyperedge is a conjugated group of order 5, 402 a 60-atom molecule."""
    from equihgnn_amd.batch import ATOM_FEATURE_DIMS, HMol, MolStore, synth_molecule
    rng = np.random.default_rng(5)
    mols = [synth_molecule(rng, "qm9") for _ in range(200)] + [synth_molecule(rng, "pcqm") for _ in range(200)]
    feats = lambda n: np.stack([rng.integers(0, d, size=n) for d in ATOM_FEATURE_DIMS], 1).astype(np.int64)
    e0 = np.zeros(0, np.int64)
    mols.append(HMol(feats(1), rng.normal(size=(1, 3)).astype(np.float32), e0, e0, np.zeros((0, 1), np.int64), e0, 0.25))
    mols.append(HMol(feats(5), rng.normal(size=(5, 3)).astype(np.float32), np.arange(5, dtype=np.int64),
                     np.zeros(5, np.int64), np.full((1, 1), 5, np.int64), np.array([5], np.int64), -1.5))
    mols.append(synth_molecule(rng, "pcqm", n_atoms=60))
    return Form(MolStore(mols), H_FIELDS, ("num_nodes", "num_hyperedges"), (1, 1, 0))


def _graph_form(flavour, seed):
    from equihgnn_amd.batch import ATOM_FEATURE_DIMS, GMol, GraphStore, synth_graph
    rng = np.random.default_rng(seed)
    mols = [synth_graph(rng, flavour) for _ in range(400)]
    F = mols[0].edge_attr.shape[1]
    x1 = np.stack([rng.integers(0, d, size=1) for d in ATOM_FEATURE_DIMS], 1).astype(np.int64)
    mols.append(GMol(x1, np.zeros((2, 0), np.int64), np.zeros((0, F), np.int64), 0.5))       # 400: one atom, no edge
    return Form(GraphStore(mols), G_FIELDS, ("num_nodes", "num_edges"), (1, 0))


@pytest.fixture(scope="module")
def graph1():
    f = _graph_form("qm9", 6)
    assert f.host.F == 1
    return f


@pytest.fixture(scope="module")
def graph3():
    f = _graph_form("pcqm", 7)
    assert f.host.F == 3
    return f


def _indices(name, n_mols):
    """The index sets of the cases.  B = 300 is more than one scan chunk (256 molecules) and holds every hand-made molecule."""
    rng = np.random.default_rng(11)
    if name == "B1":
        return np.array([7], np.int64)
    if name == "B3":                    # the same molecule twice around the one without hyperedges / edges
        return np.array([5, 400, 5], np.int64)
    if name == "B70":                   # pcqm only in the hypergraph store (200..399); any 70 of a graph store
        return np.arange(200, 270, dtype=np.int64)
    if name == "B300":
        return np.concatenate((rng.permutation(400)[:300 - (n_mols - 400)], np.arange(400, n_mols))).astype(np.int64)
    if name == "B0":
        return np.zeros(0, np.int64)
    raise KeyError(name)


H_MODES = (None, "min", "bucket", "spare300")
G_MODES = (None, "min", "selfloops", "bucket", "spare300")
CASES = lambda modes: [(b, m) for b in ("B1", "B3", "B70", "B300") for m in modes] + [("B0", m) for m in modes if m]


@pytest.mark.parametrize("which,mode", CASES(H_MODES))
def test_hypergraph_collate_writes_the_host_collates_bytes(hyper, which, mode):
    idx = _indices(which, len(hyper.host))
    tgt = hyper.pad_to(idx, mode)
    want = hyper.host.collate(idx, pad_to=tgt)
    got = hyper.dev.collate(idx, pad_to=tgt)
    hyper.same(got, want, (which, mode))
    N, M, Z = hyper.host.extents(idx)
    assert got._counts.tolist() == [N, M, Z, 0]
    if mode == "spare300":              # the padded atoms' line, against the host's bits and the formula's
        line = got.pos[N:, 0].cpu()
        assert line.shape[0] == 300 and torch.equal(line.view(torch.int32), want.pos[N:, 0].view(torch.int32))
        assert torch.equal(line, torch.tensor(1.0e4, dtype=torch.float32) + 10.0 * torch.arange(300, dtype=torch.float32))
        assert not got.pos[N:, 1:].any()


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("which,mode", CASES(G_MODES))
def test_graph_collate_writes_the_host_collates_bytes(graph1, graph3, F, which, mode):
    form = graph1 if F == 1 else graph3
    idx = _indices(which, len(form.host))
    tgt = form.pad_to(idx, mode)
    want = form.host.collate(idx, pad_to=tgt)
    got = form.dev.collate(idx, pad_to=tgt)
    form.same(got, want, (F, which, mode))
    N, E = form.host.extents(idx)
    assert got._counts.tolist() == [N, E, 0, 0]
    if mode == "selfloops":
        assert (got.edge_index[:, E:] == N).all() and got.edge_index.shape[1] == E + 9


@pytest.mark.parametrize("form_name", ["hyper", "graph3"])
def test_index_as_a_slice_of_a_larger_device_tensor_and_into_packed_staging(request, form_name):
    """What the loader does: idx is a slice at a non-zero offset of the epoch's permutation, out a packed device batch."""
    form = request.getfixturevalue(form_name)
    idx = _indices("B300", len(form.host))
    perm = torch.from_numpy(np.concatenate((np.full(5, -7, np.int64), idx, np.full(9, 10 ** 9, np.int64)))).to(DEV)
    tgt = form.pad_to(idx, "bucket")
    out = form.dev.empty_staging(tgt, len(idx) + 1)
    assert out._flat.is_cuda and out._flat.data_ptr() % 256 == 0
    got = form.dev.collate(perm[5:5 + len(idx)], pad_to=tgt, out=out)
    assert got is out
    form.same(got, form.host.collate(idx, pad_to=tgt))
    ref = form.host.empty_staging(tgt, len(idx) + 1)
    assert out._layout == ref._layout and out._flat.numel() == ref._flat.numel()
    # an out that does not fit: another shape, a CPU batch
    with pytest.raises(ValueError, match="collate: out"):
        form.dev.collate(idx[:10], pad_to=tgt, out=out)
    with pytest.raises(ValueError, match="collate: out"):
        form.dev.collate(idx, pad_to=tgt, out=ref)
    # host-side checks before any launch
    with pytest.raises(IndexError):
        form.dev.collate(np.array([0, len(form.host)], np.int64))
    with pytest.raises(ValueError, match="collate: pad_to must exceed the batch"):
        form.dev.collate(idx, pad_to=form.host.extents(idx))
    # a device index without pad_to (read back once) gives the unpadded batch
    form.same(form.dev.collate(perm[5:5 + len(idx)]), form.host.collate(idx))


@pytest.mark.parametrize("form_name", ["hyper", "graph1"])
def test_an_index_outside_the_store_counts_as_an_empty_molecule_and_sets_status_bit_0(request, form_name):
    form = request.getfixturevalue(form_name)
    idx = _indices("B70", len(form.host))
    bad = idx.copy()
    bad[3], bad[40] = len(form.host), -1
    tgt = form.pad_to(idx, "bucket")
    got = form.dev.collate(torch.from_numpy(bad).to(DEV), pad_to=tgt)          # (a device index is trusted: no host check)
    keep = np.delete(idx, [3, 40])
    ext = form.host.extents(keep)
    counts = got._counts.tolist()
    assert counts[:len(ext)] == list(ext) and counts[len(ext)] == 1
    want = form.host.collate(keep, pad_to=tgt)
    for f in form.fields:               # everything but the per-molecule fields is the batch of the 68 valid molecules
        if f in ("y", "n_e", "batch"):
            continue
        assert torch.equal(getattr(got, f).cpu(), getattr(want, f)), f
    y = got.y.cpu()
    assert y[3] == 0 and y[40] == 0 and torch.equal(torch.from_numpy(np.delete(y.numpy(), [3, 40])), want.y)
    assert not ((got.batch == 3) | (got.batch == 40)).any()


def _guarded(n_elems, dtype):
    """[n_elems] of dtype with a 64-element guard behind it, everything filled with the sentinel byte"""
    buf = torch.full(((n_elems + 64) * torch.empty(0, dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf.view(dtype)


def _guard_intact(buf, n_elems):
    return bool((buf[n_elems:].view(torch.uint8) == SENTINEL).all())


def test_extents_that_do_not_fit_set_status_bit_1_and_nothing_is_written_past_them_hypergraph(hyper):
    from equihgnn_amd import hip
    L, d = hip.lib(), hyper.dev
    idx = _indices("B70", len(hyper.host))
    N, M, Z = hyper.host.extents(idx)
    B, PN, PM, PZ = len(idx), N - 3, M, Z - 5           # every extent too small (PM == M: no room for the padding hyperedge)
    dev_idx = torch.from_numpy(idx).to(DEV)
    spec = dict(x=(PN * 9, torch.int64), pos=(PN * 3, torch.float32), batch=(PN, torch.int64), edge_index0=(PZ, torch.int64),
                edge_index1=(PZ, torch.int64), edge_attr=(PM, torch.int64), e_order=(PM, torch.int64),
                n_e=(B + 1, torch.int64), y=(B + 1, torch.float32))
    bufs = {k: _guarded(n, dt) for k, (n, dt) in spec.items()}
    ws = torch.empty(L.hb_collate_dev_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    a = hip.HbCollateDev()
    a.B, a.n_mols, a.idx = B, len(d), dev_idx.data_ptr()
    a.node_off, a.he_off, a.inc_off = (d._offsets[k].data_ptr() for k in range(3))
    for name in ("x", "pos", "v", "e", "edge_attr", "e_order", "y"):
        setattr(a, name, getattr(d, name).data_ptr())
    a.PN, a.PM, a.PZ, a.padded = PN, PM, PZ, 1
    for k, b in bufs.items():
        setattr(a, "out_" + k, b.data_ptr())
    a.out_counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel()
    rc = L.hb_collate_dev(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == hip.EQH_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [N, M, Z, 2]
    for k, (n, _) in spec.items():
        assert _guard_intact(bufs[k], n), k
    want = hyper.host.collate(idx)                       # what fits is the head of the batch
    assert torch.equal(bufs["x"][:PN * 9].cpu(), want.x.reshape(-1)[:PN * 9])
    assert torch.equal(bufs["edge_index1"][:PZ].cpu(), want.edge_index1[:PZ])
    assert torch.equal(bufs["e_order"][:PM].cpu(), want.e_order[:PM])


def test_extents_that_do_not_fit_set_status_bit_1_and_nothing_is_written_past_them_graph(graph3):
    from equihgnn_amd import hip
    L, d = hip.lib(), graph3.dev
    idx = _indices("B70", len(graph3.host))
    N, E = graph3.host.extents(idx)
    B, F, PN, PE = len(idx), 3, N, E - 6                 # PN == N: no room for the padding atom
    dev_idx = torch.from_numpy(idx).to(DEV)
    spec = dict(x=(PN * 9, torch.int64), batch=(PN, torch.int64), edge_index=(2 * PE, torch.int64),
                edge_attr=(PE * F, torch.int64), y=(B + 1, torch.float32))
    bufs = {k: _guarded(n, dt) for k, (n, dt) in spec.items()}
    ws = torch.empty(L.gb_collate_dev_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    a = hip.GbCollateDev()
    a.B, a.n_mols, a.idx, a.F = B, len(d), dev_idx.data_ptr(), F
    a.node_off, a.edge_off = (d._offsets[k].data_ptr() for k in range(2))
    for name in ("x", "src", "dst", "edge_attr", "y"):
        setattr(a, name, getattr(d, name).data_ptr())
    a.PN, a.PE, a.padded = PN, PE, 1
    for k, b in bufs.items():
        setattr(a, "out_" + k, b.data_ptr())
    a.out_counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel()
    rc = L.gb_collate_dev(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == hip.EQH_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [N, E, 2, 0]
    for k, (n, _) in spec.items():
        assert _guard_intact(bufs[k], n), k
    want = graph3.host.collate(idx)
    assert torch.equal(bufs["edge_index"][:2 * PE].view(2, PE).cpu(), want.edge_index[:, :PE])
    assert torch.equal(bufs["edge_attr"][:PE * F].cpu(), want.edge_attr.reshape(-1)[:PE * F])


@pytest.mark.parametrize("form_name", ["hyper", "graph3"])
def test_the_same_call_twice_into_different_buffers_gives_equal_bytes(request, form_name):
    form = request.getfixturevalue(form_name)
    idx = _indices("B300", len(form.host))
    tgt = form.pad_to(idx, "spare300")
    one, two = form.dev.collate(idx, pad_to=tgt), form.dev.collate(idx, pad_to=tgt)
    for f in form.fields:
        a, b = getattr(one, f), getattr(two, f)
        assert a.data_ptr() != b.data_ptr() or a.numel() == 0
        assert torch.equal(a.view(torch.uint8) if a.numel() else a, b.view(torch.uint8) if b.numel() else b), f


@pytest.mark.parametrize("form_name", ["hyper", "graph1"])
def test_the_two_launches_replay_in_a_captured_graph_on_an_index_overwritten_in_place(request, form_name):
    form = request.getfixturevalue(form_name)
    rng = np.random.default_rng(3)
    first, second = rng.permutation(len(form.host))[:64].astype(np.int64), rng.permutation(len(form.host))[:64].astype(np.int64)
    tgt = tuple(max(a, b) for a, b in zip(form.pad_to(first, "bucket"), form.pad_to(second, "bucket")))
    idx = torch.from_numpy(first).to(DEV)
    out = form.dev.empty_staging(tgt, 65)
    form.dev.collate(idx, pad_to=tgt, out=out)             # (outside the capture once: the library is loaded, scratch exists)
    torch.cuda.synchronize()
    out._flat.fill_(SENTINEL)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        form.dev.collate(idx, pad_to=tgt, out=out)
    g.replay()
    form.same(out, form.host.collate(first, pad_to=tgt), "first")
    idx.copy_(torch.from_numpy(second).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    form.same(out, form.host.collate(second, pad_to=tgt), "second")
    assert not np.array_equal(first, second)


def test_subset_matches_the_host_stores_subset(hyper, graph3):
    ids = np.random.default_rng(9).permutation(401)[:50]
    sub_h, sub_d = graph3.host.subset(ids), graph3.dev.subset(ids)
    assert len(sub_d) == len(sub_h) == 50 and sub_d.F == 3
    for a, b in zip(sub_d.count_columns(), sub_h.count_columns()):
        assert np.array_equal(a, b)
    pick = np.array([3, 49, 0, 17], np.int64)
    graph3.same(sub_d.collate(pick), sub_h.collate(pick))
    # DeviceMolStore.subset: the molecules ids of the parent store, in that order
    sub = hyper.dev.subset(ids)
    assert len(sub) == 50
    hyper.same(sub.collate(pick, pad_to=None), hyper.host.collate(ids[pick]))
    with pytest.raises(IndexError):
        hyper.dev.subset([len(hyper.host)])
