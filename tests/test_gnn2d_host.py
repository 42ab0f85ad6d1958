"""Host-side checks of the 2-D baselines gin / gcn: registry, state_dict layout against the reference's, the 2-D collate and
padding, read_processed_graph, the generator's stand-ins and its bit-for-bit regeneration.  No GPU needed."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from common import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF  # noqa: E402  (the reference checkout the generators read)

HAVE_REF = os.path.isfile(os.path.join(REF, "equihgnn", "models", "baseline_2d.py"))


def test_registry_maps_gin_and_gcn_to_gnn_2d():
    import equihgnn_amd.models as M
    from equihgnn_amd.registry import create_model, registry

    for name in ("gin", "gcn"):
        klass = registry.get_model_class(name)
        assert klass is not None and klass.__name__ == "GNN_2D" and M.MODELS[name] is klass
        assert create_model(name) is klass
    for name in ("gat", "gatv2"):
        assert registry.get_model_class(name) is None


def test_unbuilt_variants_raise_with_a_reason():
    from equihgnn_amd.baseline_2d import GNN_2D

    for kw in (dict(gnn_type="gat"), dict(gnn_type="gatv2"), dict(graph_pooling="max"), dict(graph_pooling="attention"),
               dict(graph_pooling="set2set")):
        with pytest.raises(NotImplementedError, match="not|torch_geometric"):
            GNN_2D(1, emb_dim=32, **kw)
    with pytest.raises(ValueError):
        GNN_2D(1, num_layer=1)


@pytest.mark.parametrize("gnn_type", ["gin", "gcn"])
def test_state_dict_layout_matches_the_reference(gnn_type):
    """main.py:28-31 constructs model_cls(1, gnn_type=method, drop_ratio=dropout): same signature, same keys and shapes
    as the reference's GNN_2D (tests/golden/reference_state_dicts_2d.json, written by make_golden_2d.py).  The layout does
    not depend on the bond width of the data: all three bond tables exist either way."""
    from equihgnn_amd.baseline_2d import GNN_2D

    with open(os.path.join(GOLDEN_DIR, "reference_state_dicts_2d.json")) as f:
        ref = json.load(f)[gnn_type]
    sd = GNN_2D(1, num_layer=5, emb_dim=32, gnn_type=gnn_type, drop_ratio=0.0).state_dict()
    assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()} == ref
    m = GNN_2D(1, gnn_type=gnn_type, drop_ratio=0.1)        # main.py's call: 5 layers, width 300
    assert m.num_layer == 5 and m.emb_dim == 300 and m.graph_pred_linear.in_features == 300


def _pyg_batch(mols):
    """Plain numpy restatement of PyG Batch.from_data_list for Data(x, edge_index, edge_attr, y)."""
    xs, eis, eas, bs, ys, off = [], [], [], [], [], 0
    for i, m in enumerate(mols):
        xs.append(m.x)
        eis.append(m.edge_index + off)
        eas.append(m.edge_attr)
        bs.append(np.full(m.x.shape[0], i, dtype=np.int64))
        ys.append(m.y)
        off += m.x.shape[0]
    return np.concatenate(xs), np.concatenate(eis, 1), np.concatenate(eas), np.concatenate(bs), np.array(ys, np.float32)


@pytest.mark.parametrize("flavour,F", [("qm9", 1), ("pcqm", 3)])
def test_graph_store_collate_is_pyg_batch(flavour, F):
    from equihgnn_amd.batch import GraphStore, synth_graph

    rng = np.random.default_rng(3)
    mols = [synth_graph(rng, flavour) for _ in range(12)]
    st = GraphStore(mols)
    idx = [5, 0, 11, 3]
    b = st.collate(idx)
    x, ei, ea, batch, y = _pyg_batch([mols[i] for i in idx])
    assert b.edge_attr.shape[1] == F
    for got, want in ((b.x, x), (b.edge_index, ei), (b.edge_attr, ea), (b.batch, batch), (b.y, y)):
        assert np.array_equal(got.numpy(), want)
    assert (b.num_nodes, b.num_edges, b.num_graphs) == (x.shape[0], ei.shape[1], 4)
    # ogb mol2graph: every bond in both directions, (i, j) then (j, i)
    assert np.array_equal(ei[:, 0::2], ei[::-1, 1::2])


def test_pad_graph_batch_masks():
    from equihgnn_amd.batch import graph_bucket_sizes, pad_graph_batch, synth_graph_batch
    from equihgnn_amd.layers import real_row_mask

    b = synth_graph_batch(6, 4, "pcqm")
    n, e = graph_bucket_sizes(b.num_nodes, b.num_edges)
    p = pad_graph_batch(b, n, e)
    N, E, B = b.num_nodes, b.num_edges, b.num_graphs
    assert p.x.shape[0] == n and p.edge_index.shape[1] == e and p.y.shape[0] == B + 1 and p.num_real_graphs == B
    assert torch.equal(p.x[:N], b.x) and torch.equal(p.edge_index[:, :E], b.edge_index)
    assert (p.batch[N:] == B).all() and (p.edge_index[:, E:] >= N).all() and (p.edge_index[:, E:] < n).all()
    mask = real_row_mask(p, torch.zeros(1))
    assert mask.shape == (n, 1) and float(mask.sum()) == N and float(mask[:N].min()) == 1.0
    assert real_row_mask(b, torch.zeros(1)) is None
    with pytest.raises(ValueError):
        pad_graph_batch(b, N, e)


def _write_graph_file(path, mols):
    """torch.save((data, slices)) of a PyG InMemoryDataset of Data(x, edge_index, edge_attr, y, pos, z, smile, idx), the
    containers being instances of classes named like PyG's (cf. tests/test_reader.py)."""
    mods = {n: types.ModuleType(n) for n in ("torch_geometric", "torch_geometric.data", "torch_geometric.data.data",
                                             "torch_geometric.data.storage")}

    class GlobalStorage:
        pass

    class Data:
        pass

    GlobalStorage.__module__, GlobalStorage.__qualname__ = "torch_geometric.data.storage", "GlobalStorage"
    Data.__module__, Data.__qualname__ = "torch_geometric.data.data", "Data"
    mods["torch_geometric.data.storage"].GlobalStorage = GlobalStorage
    mods["torch_geometric.data.data"].Data = Data
    off = lambda c: torch.from_numpy(np.concatenate(([0], np.cumsum(c))).astype(np.int64))
    n = [m.x.shape[0] for m in mols]
    e = [m.edge_index.shape[1] for m in mols]
    fields = {"x": torch.from_numpy(np.concatenate([m.x for m in mols])),
              "edge_index": torch.from_numpy(np.concatenate([m.edge_index for m in mols], 1)),
              "edge_attr": torch.from_numpy(np.concatenate([m.edge_attr for m in mols])),
              "y": torch.tensor([[m.y, 7.0] for m in mols], dtype=torch.float32),
              "pos": torch.zeros((sum(n), 3)), "z": torch.zeros(sum(n), dtype=torch.int64),
              "smile": ["C"] * len(mols), "idx": torch.arange(len(mols))}
    one = off(np.ones(len(mols), dtype=np.int64))
    slices = {"x": off(n), "edge_index": off(e), "edge_attr": off(e), "y": one, "pos": off(n), "z": off(n), "idx": one}
    store, data = GlobalStorage(), Data()
    store.__dict__["_mapping"] = fields
    data.__dict__["_store"] = store
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        torch.save((data, slices), path)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.mark.parametrize("flavour", ["qm9", "pcqm"])
def test_read_processed_graph_roundtrip(tmp_path, flavour):
    from equihgnn_amd.batch import GraphStore, synth_graph
    from equihgnn_amd.reader import read_processed_graph

    rng = np.random.default_rng(9)
    mols = [synth_graph(rng, flavour) for _ in range(7)]
    path = str(tmp_path / "g_data.pt")
    _write_graph_file(path, mols)
    assert "torch_geometric" not in sys.modules or not hasattr(sys.modules["torch_geometric"], "data")
    st = read_processed_graph(path)
    assert len(st) == 7
    a, b = st.collate(range(7)), GraphStore(mols).collate(range(7))
    for k in ("x", "edge_index", "edge_attr", "batch", "y"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------------------------------------
# the generator's stand-ins
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standins():
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_2d
    return make_golden_2d


def test_standin_message_passing_is_gather_message_scatter_add(standins):
    class Conv(standins.MessagePassing):
        def message(self, x_j, w):
            return w.unsqueeze(-1) * x_j

    g = torch.Generator().manual_seed(0)
    N, E = 9, 30
    ei = torch.randint(0, N, (2, E), generator=g)
    x = torch.randn(N, 5, generator=g, dtype=torch.float64)
    w = torch.randn(E, generator=g, dtype=torch.float64)
    out = Conv().propagate(ei, x=x, w=w)
    want = torch.zeros_like(x)
    for e in range(E):                   # flow source_to_target: message from edge_index[0] to edge_index[1]
        want[ei[1, e]] += w[e] * x[ei[0, e]]
    assert torch.allclose(out, want)


def test_standin_degree_and_pools(standins):
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 6, (40,), generator=g)
    assert torch.equal(standins.degree(idx, 8, dtype=torch.float32), torch.bincount(idx, minlength=8).float())
    batch = torch.tensor([0, 0, 0, 1, 3, 3])
    x = torch.randn(6, 4, generator=g)
    mean = standins.global_mean_pool(x, batch)
    mx = standins.global_max_pool(x, batch)
    assert mean.shape == (4, 4) and torch.allclose(mean[0], x[:3].mean(0)) and torch.equal(mean[2], torch.zeros(4))
    assert torch.allclose(mean[3], x[4:].mean(0)) and torch.equal(mx[3], x[4:].max(0).values)


def test_standin_bond_encoder_sums_present_columns(standins):
    enc = standins.BondEncoder(8)
    assert [e.weight.shape[0] for e in enc.bond_embedding_list] == [5, 6, 2]
    a3 = torch.tensor([[1, 2, 0], [4, 5, 1]])
    out = enc(a3)
    want = sum(enc.bond_embedding_list[i].weight[a3[:, i]] for i in range(3))
    assert torch.allclose(out, want)
    out1 = enc(a3[:, :1])
    out1.sum().backward()
    assert enc.bond_embedding_list[1].weight.grad is None and enc.bond_embedding_list[2].weight.grad is None
    with pytest.raises(RuntimeError):
        standins._placeholder("GATConv")(8, 8)


@pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is not on this machine")
def test_make_golden_2d_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(GOLDEN_DIR, "make_golden_2d.py"), "--check"], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("identical to the committed file") == len(
        [f for f in os.listdir(os.path.join(GOLDEN_DIR, "gnn2d")) if f.endswith(".npz")])


def test_read_processed_graph_refuses_out_of_table_bonds(tmp_path):
    """The kernels clamp a bond feature outside its ogb table (the reference's nn.Embedding would raise): the reader
    refuses such a file instead of letting it train on quietly altered inputs."""
    from equihgnn_amd.batch import GMol, synth_graph
    from equihgnn_amd.reader import read_processed_graph

    rng = np.random.default_rng(2)
    mols = [synth_graph(rng, "pcqm") for _ in range(3)]
    bad = mols[1].edge_attr.copy()
    bad[0, 1] = 6                                   # the stereo table has 6 rows
    mols[1] = GMol(x=mols[1].x, edge_index=mols[1].edge_index, edge_attr=bad, y=mols[1].y)
    path = str(tmp_path / "g_data.pt")
    _write_graph_file(path, mols)
    with pytest.raises(ValueError, match="bond tables"):
        read_processed_graph(path)
