"""GPU: fit.BucketedLoader over a device-resident store (batch.DeviceMolStore / DeviceGraphStore) -- no producer thread, no
pinned staging, collate kernels on the loader's side stream -- against the same loader over the host store: the same batches,
the same training, the same fit."""
import copy
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict  # noqa: E402

DEV = "cuda:0"
H_FIELDS = ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e", "e_order", "batch", "y")
G_FIELDS = ("x", "edge_index", "edge_attr", "batch", "y")
SIZES = ("num_nodes", "num_hyperedges", "num_graphs", "num_real_graphs")


@pytest.fixture(scope="module")
def stores():
    """203 molecules of both flavours (batches of 16 leave a smaller last one, also per rank of two) on host and device"""
    from equihgnn_amd.batch import MolStore, synth_molecule
    rng = np.random.default_rng(31)
    host = MolStore([synth_molecule(rng, "qm9" if i % 3 else "pcqm") for i in range(203)])
    return host, host.to_device(DEV)


@pytest.fixture(scope="module")
def graph_mols():
    from equihgnn_amd.batch import synth_graph
    rng = np.random.default_rng(21)
    out = [synth_graph(rng, "pcqm") for _ in range(96)]
    n = np.array([m.x.shape[0] for m in out], dtype=np.float64)
    for m, v in zip(out, (n - n.mean()) / n.std()):
        m.y = float(np.float32(v))
    return out


def _snapshot(b, fields=H_FIELDS, sizes=SIZES):
    """a batch's fields on the host (the ring hands the same object out again later) and its host-side sizes"""
    return {f: getattr(b, f).cpu() for f in fields}, tuple(getattr(b, s) for s in sizes)


def _same(a, b, where):
    assert a[1] == b[1], where
    for f in a[0]:
        x, y = a[0][f], b[0][f]
        assert x.dtype == y.dtype and x.shape == y.shape, (where, f)
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (where, f)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_device_and_host_store_loaders_yield_the_same_batches(stores, levels, rank, world):
    from equihgnn_amd.fit import BucketedLoader
    host, dev = stores
    kw = dict(seed=5, rank=rank, world=world, levels=levels, quantum=32)
    a = BucketedLoader(dev, 16, True, **kw)                      # device: the store's
    b = BucketedLoader(host, 16, True, device=DEV, **kw)
    assert a.device == torch.device(DEV)
    try:
        for epoch in range(2):
            got = [_snapshot(x) for x in a]
            want = [_snapshot(x) for x in b]
            per_rank = -(-203 // world)
            assert len(got) == len(want) == -(-per_rank // 16)
            for i, (g, w) in enumerate(zip(got, want)):
                _same(g, w, (epoch, i))
            assert got[-1][1][3] == per_rank % 16 != 0           # the smaller last batch
            assert all(g[1][3] == 16 for g in got[:-1])
    finally:
        a.close()
        b.close()
    # (the host loader has also collated into the epoch it started ahead; the device loader enqueues nothing it does not yield)
    assert a.collated == 2 * (-(-203 // world)) <= b.collated and a.collate_seconds > 0
    assert {len(s["bufs"]) <= a.prefetch + 4 for s in a._ring.values()} == {True}


def test_yielded_batches_are_packed_device_batches_with_fresh_index_slots(stores):
    from equihgnn_amd.fit import BucketedLoader
    _, dev = stores
    ld = BucketedLoader(dev, 16, False, prefetch=1)
    seen = {}
    for _ in range(2):
        for b in ld:
            assert b._flat.is_cuda and b._hyper_index is None and b._graph_index is None
            key = id(b)
            assert b._generation == seen.get(key, 0) + 1          # bumped at every hand-out of the same object
            seen[key] = b._generation
            b._hyper_index = "stale"                              # (what HyperIndex.from_batch would cache on it)
    assert len(seen) <= 2 * (1 + 4) and max(seen.values()) > 1    # two shapes, a ring of prefetch + 4 each, reused


def test_a_loader_on_another_device_than_its_store_is_refused(stores):
    from equihgnn_amd.fit import BucketedLoader
    with pytest.raises(ValueError, match="the store lives on"):
        BucketedLoader(stores[1], 16, True, device="cpu")


def test_an_abandoned_epoch_does_not_disturb_the_next(stores):
    from equihgnn_amd.fit import BucketedLoader
    host, dev = stores
    a = BucketedLoader(dev, 16, True, seed=9)
    b = BucketedLoader(host, 16, True, seed=9, device=DEV)
    try:
        for ld in (a, b):
            for i, _ in enumerate(ld):
                if i == 1:
                    break
        got = [_snapshot(x) for x in a]
        want = [_snapshot(x) for x in b]
        assert len(got) == len(want) == 13
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, i)
    finally:
        a.close()
        b.close()


def test_no_thread_is_alive_while_the_device_loader_iterates(stores):
    from equihgnn_amd.fit import BucketedLoader
    before = threading.active_count()
    ld = BucketedLoader(stores[1], 16, True, seed=1)
    for _ in range(2):
        for _b in ld:
            assert threading.active_count() == before
    assert threading.active_count() == before
    ld.close()


def test_three_graphed_training_steps_give_the_same_losses_from_either_loader(stores):
    from equihgnn_amd import models
    from equihgnn_amd.fit import BucketedLoader
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep, with_next
    host, dev = stores
    args = default_args(method="egnn_equihnns", MLP_hidden=64, output_hidden=32)
    m1 = models.MODELS["egnn_equihnns"](1, args)
    fill_state_dict(m1, 3)
    m1 = m1.to(DEV).train()
    m2 = copy.deepcopy(m1)
    losses = []
    for model, store in ((m1, dev), (m2, host)):
        step = GraphedTrainStep(model, lr=1e-3)
        ld = BucketedLoader(store, 16, True, seed=2, device=DEV)
        out = []
        try:
            for data, nxt in with_next(ld):
                out.append(float(step.step(data, nxt)))
                if len(out) == 3:
                    break
        finally:
            ld.close()
        losses.append(out)
    torch.cuda.synchronize()
    print("losses from the device store", losses[0], "from the host store", losses[1])
    assert all(np.isfinite(losses[0])) and len(set(losses[0])) == 3
    assert losses[0] == losses[1]
    s1, s2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(s1[k], s2[k]) for k in s1)


def test_one_fit_epoch_of_gin_from_device_graph_store_subsets_is_the_fit_from_host_stores(graph_mols):
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import GraphStore
    from equihgnn_amd.fit import BucketedLoader, Fitter, split_80_10_10
    from equihgnn_amd.trainer import GraphedTrainStep
    tr, va, _ = split_80_10_10(len(graph_mols), seed=1)
    whole = GraphStore(graph_mols)
    on_dev = whole.to_device(DEV)
    base = GNN_2D(1, num_layer=2, emb_dim=64, gnn_type="gin")
    fill_state_dict(base, 8)
    rows = []
    for pick in (on_dev.subset, whole.subset):
        model = copy.deepcopy(base).to(DEV)
        fitter = Fitter(model, lr=3e-3, std=1.0, step_factory=GraphedTrainStep)
        train = BucketedLoader(pick(tr), 16, True, seed=0, device=DEV)
        res = fitter.fit(train, BucketedLoader(pick(va), 16, False, device=DEV), epochs=1)
        assert len(res.history) == 1 and train.collated >= len(tr)      # (a host loader has collated ahead as well)
        rows.append(res.history[0])
    print("history row from device stores", rows[0])
    assert np.isfinite(rows[0]["train_loss"]) and rows[0] == rows[1]
