"""The 2-D data path on the host (no GPU): batch.GraphStore as a structure of arrays, its native collate gb_collate against
the restatement collate_graphs + pad_graph_batch, the GbCollate layout, fit.BucketedLoader over a GraphStore, and
reader.read_processed_graph building the array store without per-molecule objects."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from equihgnn_amd.batch import (GBatch, GMol, GraphStore, collate_graphs, graph_bucket_sizes, pad_graph_batch, synth_graph)

FIELDS = ("x", "edge_index", "edge_attr", "batch", "y")
SIZES = ("num_nodes", "num_edges", "num_graphs")


def _mols(flavour, n=12, seed=3, holes=True):
    """n synth_graph molecules; with `holes`, one without bonds and one with an isolated atom (make_golden_2d.case_mols)."""
    rng = np.random.default_rng(seed)
    mols = [synth_graph(rng, flavour) for _ in range(n)]
    F = mols[0].edge_attr.shape[1]
    if holes:
        m = mols[2]
        mols[2] = GMol(x=m.x, edge_index=np.zeros((2, 0), np.int64), edge_attr=np.zeros((0, F), np.int64), y=m.y)
        m = mols[5]
        mols[5] = GMol(x=np.concatenate([m.x, m.x[:1]], 0), edge_index=m.edge_index, edge_attr=m.edge_attr, y=m.y)
    for i, m in enumerate(mols):
        m.y = float(i)
    return mols


def _same(got, want, what=""):
    for f in FIELDS:
        assert getattr(got, f).dtype == getattr(want, f).dtype and torch.equal(getattr(got, f), getattr(want, f)), (what, f)
    for s in SIZES:
        assert getattr(got, s) == getattr(want, s), (what, s)
    assert getattr(got, "num_real_graphs", None) == getattr(want, "num_real_graphs", None), what


IDX = [5, 0, 11, 3, 2, 5, 7]          # permuted, molecule 5 twice, the bond-less molecule 2 in the middle


@pytest.mark.parametrize("flavour,F", [("qm9", 1), ("pcqm", 3)])
def test_native_graph_collate_equals_the_restatement_bit_for_bit(flavour, F):
    mols = _mols(flavour)
    store = GraphStore(mols)
    assert store.F == F and len(store) == 12
    ref = collate_graphs([mols[i] for i in IDX])
    N, E = ref.num_nodes, ref.num_edges
    assert store.extents(IDX) == (N, E)
    _same(store.collate(IDX), ref, "unpadded")
    _same(store.collate(np.array(IDX)[::-1]), collate_graphs([mols[i] for i in IDX[::-1]]), "strided idx")
    for tgt in (graph_bucket_sizes(N, E, 64), (N + 1, E), (N + 1, E + 3), (N + 5, E + 12)):
        _same(store.collate(IDX, pad_to=tgt), pad_graph_batch(ref, *tgt), tgt)
    # out=: a packed staging buffer, filled with garbage first (the collate must write every element)
    tgt = graph_bucket_sizes(N, E, 64)
    out = GBatch.empty_packed(tgt[0], tgt[1], F, len(IDX) + 1)
    out._flat.fill_(0xA5)
    got = store.collate(IDX, pad_to=tgt, out=out)
    assert got is out and out._flat is not None
    _same(out, pad_graph_batch(ref, *tgt), "out=")
    for f in FIELDS:                                           # every field a 256-byte aligned view of the one buffer
        off = getattr(out, f).data_ptr() - out._flat.data_ptr()
        assert 0 <= off < out._flat.numel() and off % 256 == 0
    # an empty batch
    e = store.collate([])
    assert (e.num_nodes, e.num_edges, e.num_graphs) == (0, 0, 0)
    assert e.x.shape == (0, 9) and e.edge_index.shape == (2, 0) and e.edge_attr.shape == (0, F) and e.y.shape == (0,)


@pytest.mark.parametrize("flavour", ["qm9", "pcqm"])
def test_native_graph_collate_of_a_batch_without_edges(flavour):
    mols = [GMol(x=m.x, edge_index=np.zeros((2, 0), np.int64), edge_attr=np.zeros((0, m.edge_attr.shape[1]), np.int64), y=m.y)
            for m in _mols(flavour, holes=False)]
    store = GraphStore(mols)
    ref = collate_graphs([mols[i] for i in IDX])
    assert ref.num_edges == 0
    _same(store.collate(IDX), ref, "unpadded")
    for PE in (0, 64):
        tgt = (graph_bucket_sizes(ref.num_nodes, 0, 64)[0], PE)
        _same(store.collate(IDX, pad_to=tgt), pad_graph_batch(ref, *tgt), tgt)
    # ... and a store in which only SOME molecules have edges, indexed so that the batch has none
    mixed = GraphStore(_mols(flavour))
    _same(mixed.collate([2, 2]), collate_graphs([_mols(flavour)[2]] * 2), "bond-less twice")


def test_native_graph_collate_errors():
    mols = _mols("pcqm")
    store = GraphStore(mols)
    N, E = store.extents(IDX)
    for bad in ([0, 12], [-1], [3, 10 ** 12]):
        with pytest.raises(IndexError):
            store.collate(bad)
        with pytest.raises(IndexError):
            store.collate(bad, pad_to=(4096, 8192))
    with pytest.raises(ValueError, match="pad_to must exceed"):
        store.collate(IDX, pad_to=(N, E + 64))
    with pytest.raises(ValueError, match="pad_to must exceed"):
        store.collate(IDX, pad_to=(N + 64, E - 1))
    with pytest.raises(ValueError):
        pad_graph_batch(collate_graphs([mols[i] for i in IDX]), N, E + 64)          # (the restatement refuses the same)
    tgt, B1 = (N + 9, E + 4), len(IDX) + 1
    ok = lambda: GBatch.empty_packed(tgt[0], tgt[1], 3, B1)
    store.collate(IDX, pad_to=tgt, out=ok())
    for field, wrong in (("x", torch.empty((tgt[0], 9), dtype=torch.int32)), ("y", torch.empty(B1, dtype=torch.float64)),
                         ("edge_index", torch.empty((tgt[1], 2), dtype=torch.int64)),
                         ("edge_attr", torch.empty((tgt[1], 1), dtype=torch.int64)),
                         ("batch", torch.empty(tgt[0] + 1, dtype=torch.int64)),
                         ("edge_index", torch.empty((tgt[1], 2), dtype=torch.int64).t())):          # right shape, strided
        out = ok()
        setattr(out, field, wrong)
        with pytest.raises(ValueError, match=f"out.{field} must be"):
            store.collate(IDX, pad_to=tgt, out=out)
    with pytest.raises(ValueError, match="bond features"):
        GraphStore(_mols("qm9")[:3] + mols[:3])
    # a store re-seated by hand with arrays the C side must not read by address
    store.src = store.src.astype(np.int32)
    with pytest.raises(ValueError, match="GraphStore.src must be"):
        store.collate(IDX)
    with pytest.raises(ValueError):
        GraphStore.from_arrays(store.n_nodes, store.n_edges, store.x[:-1], store.dst, store.dst, store.edge_attr, store.y)


def test_graph_store_from_arrays_is_the_store_of_the_molecules():
    mols = _mols("pcqm")
    a = GraphStore(mols)
    b = GraphStore.from_arrays(a.n_nodes, a.n_edges, a.x, a.src, a.dst, a.edge_attr, a.y)
    assert b.x is a.x and b.edge_attr is a.edge_attr                          # right dtype and layout: kept, not copied
    for name in ("node_off", "edge_off"):
        assert np.array_equal(getattr(a, name), getattr(b, name)) and getattr(b, name).shape == (13,)
    _same(b.collate(IDX, pad_to=(400, 900)), a.collate(IDX, pad_to=(400, 900)))


def test_graph_store_subset_is_the_store_of_those_molecules():
    mols = _mols("pcqm")
    sub = GraphStore(mols).subset(IDX)
    assert len(sub) == len(IDX) and sub.F == 3
    _same(sub.collate(range(len(IDX)), pad_to=(400, 900)), GraphStore([mols[i] for i in IDX]).collate(range(len(IDX)), pad_to=(400, 900)))
    assert len(GraphStore(mols).subset([])) == 0
    with pytest.raises(IndexError):
        GraphStore(mols).subset([12])


def test_packed_graph_batch_is_a_view_of_one_buffer_and_survives_to():
    b = pad_graph_batch(collate_graphs(_mols("pcqm")), 512, 1024)
    p = b.packed()
    _same(p, b)
    assert p._flat.dtype == torch.uint8 and p._flat.numel() % 256 == 0
    q = p.to("cpu")
    _same(q, b)
    assert q._layout == p._layout and q.x.data_ptr() == q._flat.data_ptr()
    e = GBatch.empty_packed(512, 1024, 3, b.num_graphs)
    assert e._layout == p._layout                                # a loader's staging batch refreshes a trainer's static by ONE copy
    assert not hasattr(b, "_flat") and b.to("cpu").x.shape == b.x.shape       # the unpacked form is unchanged


def test_gb_collate_struct_layout_matches_the_compiler(tmp_path):
    """sizeof(GbCollate) and offsetof / sizeof of every field as the host compiler lays them out, against the
    ctypes.Structure derived from the header (tests/test_cabi.py's method on this one struct)."""
    from equihgnn_amd import build, hip

    cls, s = hip.GbCollate, "GbCollate"
    assert [f for f, _ in cls._fields_] == ["B", "n_mols", "idx", "node_off", "edge_off", "x", "src", "dst", "edge_attr", "F", "y",
                                            "PN", "PE", "padded", "out_x", "out_edge_index", "out_edge_attr", "out_batch",
                                            "out_y", "out_counts"]
    assert hip.SIGNATURES["gb_collate"] == (ctypes.c_int32, [ctypes.POINTER(cls)])
    lines, want = [f'std::printf("{s} %zu\\n", sizeof({s}));'], {s: str(ctypes.sizeof(cls))}
    for f, _ in cls._fields_:
        lines.append(f'std::printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)nullptr)->{f}));')
        want[f"{s}.{f}"] = f"{getattr(cls, f).offset} {getattr(cls, f).size}"
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "equihgnn_hip.h"\nint main() {\n' + "\n".join(lines)
                   + "\nreturn 0;\n}\n")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-I", build.INCLUDE, str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got == want


def test_gb_collate_argument_validation():
    from equihgnn_amd import hip
    L = hip.lib()
    assert L.gb_collate(None) == hip.EQH_ERR_ARG
    a = hip.GbCollate()
    assert L.gb_collate(ctypes.byref(a)) == hip.EQH_ERR_ARG                   # no out_counts
    counts = np.full(2, -7, dtype=np.int64)
    a.out_counts = counts.ctypes.data
    assert L.gb_collate(ctypes.byref(a)) == hip.EQH_OK and counts.tolist() == [0, 0]      # B = 0, unpadded: nothing to write
    a.B = 1
    assert L.gb_collate(ctypes.byref(a)) == hip.EQH_ERR_ARG                   # idx missing
    a.B, a.padded, a.PN, a.PE = 0, 1, 0, 0
    assert L.gb_collate(ctypes.byref(a)) == hip.EQH_ERR_RANGE                 # PN must exceed N
    a.PN = 1
    assert L.gb_collate(ctypes.byref(a)) == hip.EQH_ERR_ARG                   # out_x missing for one padded atom


def test_bucketed_loader_over_a_graph_store_static_shapes_and_coverage():
    """tests/test_fit.py::test_bucketed_loader_static_shapes_and_coverage for a GraphStore: a few static buckets per run,
    every molecule once per epoch, packed staging buffers, two ranks, and padded edges among padded atoms only."""
    from equihgnn_amd.fit import BucketedLoader
    mols = _mols("pcqm", n=230, seed=4)
    store = GraphStore(mols)
    seen = []
    for rank in range(2):
        ld = BucketedLoader(store, 32, True, seed=5, device=None, rank=rank, world=2, prefetch=2, levels=1 + 2 * rank)
        ld.lookahead = False
        shapes = set()
        for b in ld:
            nb = b.num_real_graphs
            assert isinstance(b, GBatch) and b.edge_attr.shape[1] == 3
            seen.extend(int(v) for v in b.y[:nb].tolist())
            shapes.add((b.x.shape[0], b.edge_index.shape[1], b.y.shape[0]))
            assert (b.num_nodes, b.num_edges, b.num_graphs) == (b.x.shape[0], b.edge_index.shape[1], nb + 1)
            assert getattr(b, "_flat", None) is not None and int(b.batch[-1]) == nb
            assert torch.equal(b.batch[b.edge_index[0]], b.batch[b.edge_index[1]])      # no real atom reads a padded one
            n_real = int((b.batch < nb).sum())
            _same(b, pad_graph_batch(collate_graphs([mols[int(i)] for i in b.y[:nb].tolist()]), b.x.shape[0],
                                     b.edge_index.shape[1]), "loader batch")
            assert n_real < b.x.shape[0]
        buckets = sorted({s[:2] for s in shapes})
        assert 1 <= len(buckets) <= ld.levels
        for lo, hi in zip(buckets, buckets[1:]):              # neighbouring ladder rungs: (q, 2 q) apart
            assert (hi[0] - lo[0]) % ld.quantum == 0 and hi[0] > lo[0] and hi[1] - lo[1] == 2 * (hi[0] - lo[0])
        assert all(s[0] % ld.quantum == 0 and s[1] % ld.quantum == 0 for s in buckets)
        assert ld.collated == 115 and ld.collate_seconds > 0
    assert sorted(seen) == list(range(230))
    # a ladder deep enough that this epoch's batches land on several rungs: the rung check really compares rungs
    ld = BucketedLoader(store, 32, True, seed=5, device=None, rank=1, world=2, levels=6)
    batches, tgts = ld.plan()
    rungs = sorted(set(tgts))
    assert 2 <= len(rungs) <= 6 and all(len(t) == 2 for t in rungs)
    for lo, hi in zip(rungs, rungs[1:]):
        assert (hi[0] - lo[0]) % 64 == 0 and hi[0] > lo[0] and hi[1] - lo[1] == 2 * (hi[0] - lo[0])
    for b, t in zip(batches, tgts):                           # one spare atom, no spare edge
        assert store.n_nodes[b].sum() + 1 <= t[0] and store.n_edges[b].sum() <= t[1]


def test_bucketed_loader_pads_every_rank_of_a_graph_store_to_the_same_extents():
    from equihgnn_amd.fit import BucketedLoader
    store = GraphStore(_mols("qm9", n=400, seed=11))
    world = 4
    for levels in (1, 3):
        plans = []
        for r in range(world):
            ld = BucketedLoader(store, 32, shuffle=True, seed=5, rank=r, world=world, levels=levels)
            ld.lookahead = False
            plans.append([ld.plan() for _ in range(3)])
            ld.close()
        for e in range(3):
            t0 = plans[0][e][1]
            assert all(len(t) == 2 for t in t0)
            for r in range(1, world):
                assert plans[r][e][1] == t0, (levels, e, r)
            nat = [[int(store.n_nodes[b].sum()) for b in plans[r][e][0]] for r in range(world)]
            assert len({tuple(n) for n in nat}) == world
            for r in range(world):
                for b, t in zip(plans[r][e][0], plans[r][e][1]):
                    assert store.n_nodes[b].sum() < t[0] and store.n_edges[b].sum() <= t[1]


def test_bucketed_loader_reused_graph_buffers_do_not_carry_a_stale_index():
    from equihgnn_amd.fit import BucketedLoader, _drop_index
    store = GraphStore(_mols("qm9", n=16 * 12, seed=8, holes=False))
    ld = BucketedLoader(store, 16, False, device=None, prefetch=2)
    seen = {}
    for epoch in range(2):
        for i, b in enumerate(ld):
            assert getattr(b, "_graph_index", None) is None, (epoch, i)
            b._graph_index = ("index of", epoch, i)              # what a cached GraphIndex would be
            seen[id(b)] = seen.get(id(b), 0) + 1
    ld.close()
    assert max(seen.values()) > 1                                # buffers really were reused
    _drop_index(b)
    assert b._graph_index is None and b._hyper_index is None


def test_read_processed_graph_builds_no_per_molecule_object(tmp_path, monkeypatch):
    from test_gnn2d_host import _write_graph_file

    from equihgnn_amd import reader

    class Refuses:
        def __init__(self, *a, **k):
            raise AssertionError("read_processed_graph built a GMol")

    for flavour in ("qm9", "pcqm"):
        mols = _mols(flavour, n=9, seed=9)
        path = str(tmp_path / f"g_{flavour}.pt")
        _write_graph_file(path, mols)
        monkeypatch.setattr(reader, "GMol", Refuses)
        st = reader.read_processed_graph(path)
        monkeypatch.undo()
        assert isinstance(st, GraphStore) and len(st) == 9 and st.F == mols[0].edge_attr.shape[1]
        _same(st.collate(range(9)), collate_graphs(mols), flavour)
        assert np.array_equal(reader.read_processed_graph(path, target=1).y, np.full(9, 7.0, np.float32))
    # an edge that names an atom of the NEXT molecule: refused by the per-molecule maximum
    mols = _mols("pcqm", n=4, seed=2, holes=False)
    ei = mols[1].edge_index.copy()
    ei[1, 0] = mols[1].x.shape[0]
    mols[1] = GMol(x=mols[1].x, edge_index=ei, edge_attr=mols[1].edge_attr, y=mols[1].y)
    path = str(tmp_path / "g_bad.pt")
    _write_graph_file(path, mols)
    with pytest.raises(ValueError, match="not local"):
        reader.read_processed_graph(path)
