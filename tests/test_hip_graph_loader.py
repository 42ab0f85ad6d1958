"""GPU: gin / gcn fitted from a dataset -- batch.GraphStore -> fit.BucketedLoader -> trainer.GraphedTrainStep / fit.Fitter --
against the same steps fed hand-built batches (collate_graphs + pad_graph_batch + .to)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict  # noqa: E402

DEV = "cuda:0"
FIELDS = ("x", "edge_index", "edge_attr", "batch", "y")


@pytest.fixture(scope="module")
def mols():
    """96 PCQM-like molecules with a learnable, standardised target (the number of atoms)."""
    from equihgnn_amd.batch import synth_graph
    rng = np.random.default_rng(21)
    out = [synth_graph(rng, "pcqm") for _ in range(96)]
    n = np.array([m.x.shape[0] for m in out], dtype=np.float64)
    for m, v in zip(out, (n - n.mean()) / n.std()):
        m.y = float(np.float32(v))
    return out


def _model(gnn_type, seed):
    from equihgnn_amd.baseline_2d import GNN_2D
    m = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type=gnn_type)
    fill_state_dict(m, seed)
    return m.to(DEV)


@pytest.mark.parametrize("gnn_type", ["gin", "gcn"])
def test_fitting_from_the_loader_is_fitting_from_hand_built_batches(mols, gnn_type):
    """Two epochs of GraphedTrainStep on a model fed by BucketedLoader(GraphStore, device=cuda) and on its deep copy fed the
    same batches built by collate_graphs + pad_graph_batch + .to: identical inputs, then identical losses and parameters
    (torch.equal: the same captured kernels on the same inputs in one process, and the 2-D kernels have no float atomics).
    The loader's batches are packed (one flat copy into the trainer's packed static batch), the hand-built ones are not
    (one copy per field): the two refresh branches of GraphedTrainStep.step must leave the same static inputs."""
    from equihgnn_amd.batch import GraphStore, collate_graphs, pad_graph_batch
    from equihgnn_amd.fit import BucketedLoader
    from equihgnn_amd.trainer import GraphedTrainStep, with_next

    store = GraphStore(mols)
    m1 = _model(gnn_type, 3).train()
    m2 = copy.deepcopy(m1)
    tr1, tr2 = GraphedTrainStep(m1, lr=1e-3), GraphedTrainStep(m2, lr=1e-3)
    loader = BucketedLoader(store, 16, True, 7, device=DEV)
    twin = BucketedLoader(store, 16, True, 7, device=None)
    losses1, losses2, shapes = [], [], set()
    try:
        for epoch in range(2):
            batches, tgts = twin.plan()
            assert len(batches) == 6
            for step, (data, nxt) in enumerate(with_next(loader)):
                idx, tgt = batches[step], tgts[step]
                hand = pad_graph_batch(collate_graphs([mols[int(i)] for i in idx]), *tgt).to(DEV)
                assert getattr(data, "_flat", None) is not None and data.x.is_cuda and not hasattr(hand, "_flat")
                back = data.to("cpu")
                for f in FIELDS:                                 # first the inputs, bit for bit
                    assert torch.equal(getattr(back, f), getattr(hand, f).cpu()), (epoch, step, f)
                assert (data.num_nodes, data.num_edges, data.num_graphs, data.num_real_graphs) == \
                       (hand.num_nodes, hand.num_edges, hand.num_graphs, hand.num_real_graphs) == (*tgt, 17, 16)
                shapes.add(tgt)
                losses1.append(float(tr1.step(data, nxt)))
                losses2.append(float(tr2.step(hand)))
            assert step == 5
    finally:
        loader.close()
        twin.close()
    torch.cuda.synchronize()
    print(f"{gnn_type}: buckets {sorted(shapes)}, losses {losses1[0]:.6f} -> {losses1[-1]:.6f}, "
          f"max |loss difference| {max(abs(a - b) for a, b in zip(losses1, losses2)):.3e}")
    assert len(shapes) == 1 and len(tr1.slots) == len(tr2.slots) == 1
    assert getattr(next(iter(tr1.slots.values()))["static"], "_flat", None) is not None       # the static batch is packed
    assert all(np.isfinite(losses1)) and len(set(losses1)) == 12
    assert losses1 == losses2
    s1, s2 = m1.state_dict(), m2.state_dict()
    assert list(s1) == list(s2)
    differ = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    assert not differ, f"first tensor that differs: {differ[0]}"
    moved = _model(gnn_type, 3).state_dict()
    assert any(not torch.equal(s1[k], moved[k]) for k in s1 if s1[k].is_floating_point())      # (the steps did train)


def test_fit_a_2d_model_from_graph_stores_end_to_end(mols):
    """Fitter.fit with GraphedTrainStep over train / valid BucketedLoaders of GraphStores, then Fitter.test."""
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import GraphStore
    from equihgnn_amd.fit import BucketedLoader, Fitter, split_80_10_10
    from equihgnn_amd.trainer import GraphedTrainStep

    torch.manual_seed(0)
    tr, va, te = split_80_10_10(len(mols), seed=1)
    pick = lambda ids: GraphStore([mols[i] for i in ids])
    model = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type="gin").to(DEV)
    fitter = Fitter(model, lr=3e-3, std=1.0, patience_lr=0, patience_stop=5, step_factory=GraphedTrainStep)
    train = BucketedLoader(pick(tr), 16, True, seed=0, device=DEV)
    res = fitter.fit(train, BucketedLoader(pick(va), 16, False, device=DEV), epochs=3)
    h = res.history
    print("train loss per epoch", [round(e["train_loss"], 5) for e in h], "val mae", [round(e["val_mae_mean"], 5) for e in h])
    assert len(h) == 3 and h[-1]["train_loss"] < h[0]["train_loss"] and np.isfinite(h[-1]["val_mae_mean"])
    assert len(fitter.step.slots) <= 4
    assert train.collated >= 3 * len(tr)
    test_store = pick(te)
    metrics, table = fitter.test(BucketedLoader(test_store, 16, False, device=DEV), res.best_state)
    assert table.shape == (len(te), 2) and np.isfinite(metrics["test_mae_mean"]) and np.isfinite(table).all()
    assert np.array_equal(np.sort(table[:, 1]), np.sort(test_store.y))


def test_evaluation_on_reused_graph_loader_buffers_matches_fresh_batches(mols):
    """tests/test_fit.py::test_evaluation_on_reused_loader_buffers_matches_fresh_batches for a GBatch: 8 equal-shape
    batches through a ring of prefetch + 4 = 5 buffers, two passes; per molecule the predictions are those of eager
    model(data) on freshly collated, unpadded batches (1e-5: the padded / unpadded eval bound of tests/test_hip_gnn2d.py)."""
    from equihgnn_amd.batch import GraphStore, collate_graphs
    from equihgnn_amd.fit import BucketedLoader, Fitter

    model = _model("gcn", 4).eval()
    with torch.no_grad():
        want = torch.cat([model(collate_graphs(mols[i:i + 12]).to(DEV)) for i in range(0, 96, 12)]).cpu().numpy()
    assert float(np.abs(want).std()) > 1e-3                    # (predictions differ between molecules: the check bites)
    fitter = Fitter(model, lr=0.0)
    ld = BucketedLoader(GraphStore(mols), 12, False, device=DEV, prefetch=1)
    for _ in range(2):
        _, table = fitter.test(ld)
        assert table.shape == (96, 2)
        np.testing.assert_allclose(table[:, 0], want, rtol=1e-5, atol=1e-5)
        assert np.array_equal(table[:, 1], np.array([m.y for m in mols], dtype=np.float32))
    assert {len(s["bufs"]) for s in ld._ring.values()} == {5}  # one shape, 8 batches per pass through 5 buffers
