"""GPU: an epoch's loss and bootstrap metrics kept on the device -- ops.bootstrap_update against float64 numpy over the host
twin of its weights, ops.loss_accumulate against Python's sequential double sum, GraphedTrainStep(loss_readout=True) over
bootstrap / capture / calibration / replay steps, and Fitter(device_metrics=True): the same train_loss and test table as
the per-batch reads give, bootstrap metrics equal to numpy's over the host weights, and a count of device-to-host reads
that does not grow with the number of batches."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict  # noqa: E402

DEV = "cuda:0"
SLOTS = 64


def _expected(pred, target, scale, seed, position0, copies, skip=()):
    """[3, copies] float64: the sums one update adds, from the host weights and the fp32-multiply-first error."""
    from equihgnn_amd import ops
    w = ops.bootstrap_weights_host(seed, position0, len(pred), copies).astype(np.float64)
    for j in skip:
        w[:, j] = 0.0
    e = (pred * np.float32(scale)).astype(np.float64) - (target * np.float32(scale)).astype(np.float64)
    e[list(skip)] = 0.0
    return np.stack((w @ np.abs(e), w @ (e * e), w.sum(1)))


@pytest.mark.parametrize("copies", [1, 50, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_bootstrap_update_equals_float64_numpy_over_the_host_weights(n, copies):
    from equihgnn_amd import ops
    rng = np.random.default_rng(1000 * n + copies)
    seed = 17
    for position0 in (0, 2 ** 26 - 2):
        for scale in (1.0, 7.25):
            batches = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32))
                       for _ in range(2)]
            runs = []
            for _ in range(2):
                acc = torch.zeros(3, SLOTS, dtype=torch.float64, device=DEV)
                for k, (p, t) in enumerate(batches):     # two successive updates into one accumulator
                    ops.bootstrap_update(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), scale, copies, seed,
                                         position0 + k * n, acc)
                runs.append(acc.cpu())
            assert torch.equal(runs[0], runs[1])         # one writer per slot, fixed order: bitwise reproducible
            got = runs[0].numpy()
            want = sum(_expected(p, t, scale, seed, position0 + k * n, copies) for k, (p, t) in enumerate(batches))
            if n:
                rel = np.abs(got[:, :copies] - want) / np.maximum(np.abs(want), 1e-300)
                print(f"n {n} copies {copies} position0 {position0} scale {scale}: max relative difference {rel.max():.2e}")
            np.testing.assert_allclose(got[:, :copies], want, rtol=1e-12, atol=0.0)
            assert np.array_equal(got[2, :copies], want[2])          # (integers: exact)
            assert not got[:, copies:].any()                         # slots at or past `copies` stay zero


def test_bootstrap_update_on_inputs_that_are_not_unit_normal_and_one_nan():
    """Predictions around 1e3 whose errors are around 1e-3 (the difference is taken in double, after the fp32 products), and
    one NaN prediction: it reaches exactly the copies that drew its element, and only their |e| and e^2 sums."""
    from equihgnn_amd import ops
    n, copies, seed, p0, j = 300, 50, 4, 77, 123
    rng = np.random.default_rng(8)
    target = (1e3 + 10.0 * rng.standard_normal(n)).astype(np.float32)
    pred = (target.astype(np.float64) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    pred[j] = np.nan
    acc = torch.zeros(3, SLOTS, dtype=torch.float64, device=DEV)
    ops.bootstrap_update(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), 1.0, copies, seed, p0, acc)
    got = acc.cpu().numpy()[:, :copies]
    w = ops.bootstrap_weights_host(seed, p0, n, copies)
    hit = w[:, j] != 0
    assert 0 < hit.sum() < copies                                    # (both kinds of copy occur)
    assert np.array_equal(np.isnan(got[0]), hit) and np.array_equal(np.isnan(got[1]), hit)
    assert np.array_equal(got[2], w.sum(1).astype(np.float64))       # the counts carry no NaN
    want = _expected(pred, target, 1.0, seed, p0, copies, skip=(j,))
    np.testing.assert_allclose(got[:2, ~hit], want[:2, ~hit], rtol=1e-12, atol=0.0)
    assert 1e-4 < want[0, 0] / want[2, 0] < 1e-2                     # errors of the size meant, not of fp32(1e3)'s spacing


def test_loss_accumulate_is_the_sequential_double_sum():
    from equihgnn_amd import ops
    g = torch.Generator().manual_seed(3)
    losses = (torch.randn(1000, generator=g).abs() * torch.logspace(-4, 3, 1000)).to(torch.float32)
    dev = losses.to(DEV)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    for i in range(1000):
        ops.loss_accumulate(dev[i], acc)
    want = 0.0
    for v in losses.tolist():
        want += v
    total, count = acc.tolist()
    assert total == want and count == 1000.0


def test_the_device_operators_refuse_a_capturing_stream_and_host_tensors(monkeypatch):
    from equihgnn_amd import hip, ops
    acc = torch.zeros(3, SLOTS, dtype=torch.float64, device=DEV)
    x = torch.zeros(4, device=DEV)
    with pytest.raises(hip.HipLibraryError):
        ops.bootstrap_update(x.cpu(), x, 1.0, 50, 0, 0, acc)
    with pytest.raises(TypeError):
        ops.bootstrap_update(x, x, 1.0, 50, 0, 0, acc.float())
    with pytest.raises(hip.HipLibraryError, match="eqh_bootstrap_update"):
        ops.bootstrap_update(x, x, 1.0, 65, 0, 0, acc)
    # position0 travels by value: a replay would repeat it (the check is asked, not a capture started)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        ops.bootstrap_update(x, x, 1.0, 50, 0, 0, acc)
    with pytest.raises(RuntimeError, match="capturing"):
        ops.loss_accumulate(x[0], torch.zeros(2, dtype=torch.float64, device=DEV))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert not acc.any()


# ---- trainer and Fitter on a small gin ----------------------------------------------------------------------------------------
def _mols(n, seed=21):
    """PCQM-like molecules with a learnable, standardised target (the number of atoms)."""
    from equihgnn_amd.batch import synth_graph
    rng = np.random.default_rng(seed)
    out = [synth_graph(rng, "pcqm") for _ in range(n)]
    k = np.array([m.x.shape[0] for m in out], dtype=np.float64)
    for m, v in zip(out, (k - k.mean()) / k.std()):
        m.y = float(np.float32(v))
    return out


@pytest.fixture(scope="module")
def mols():
    return _mols(192)


def _gin(seed):
    from equihgnn_amd.baseline_2d import GNN_2D
    m = GNN_2D(1, num_layer=2, emb_dim=64, gnn_type="gin")
    fill_state_dict(m, seed)
    return m.to(DEV)


def test_graphed_step_keeps_the_sum_of_its_losses_on_the_device(mols):
    """20 steps: the eager bootstrap step, the capture of bucket A, its calibration windows (the second form's capture among
    them), replays, then two steps of a larger bucket B (another capture, a replay).  The device sum is the double sum of the
    losses step() returned, in order; the option changes nothing else."""
    from equihgnn_amd.batch import collate_graphs, graph_bucket_sizes, pad_graph_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    groups = [collate_graphs(mols[i:i + 16]) for i in range(0, 96, 16)]
    a = graph_bucket_sizes(max(b.x.shape[0] for b in groups), max(b.edge_index.shape[1] for b in groups), 64)
    bkt = (a[0] + 64, a[1] + 64)
    batches = [pad_graph_batch(groups[t % 6], *(a if t < 18 else bkt)).to(DEV) for t in range(20)]
    on, off = _gin(5).train(), _gin(5).train()
    tr_on, tr_off = GraphedTrainStep(on, lr=1e-3, loss_readout=True), GraphedTrainStep(off, lr=1e-3)
    want = 0.0
    for data in batches:
        want += float(tr_on.step(data))
        tr_off.step(data)
    total, count = tr_on.loss_sum.tolist()
    assert count == 20.0 and total == want and want > 0.0
    assert len(tr_on.slots) == 2                                          # both buckets captured
    if tr_on.prefetch_policy == "auto":       # 17 graphed steps of bucket A: the first window timed, the second form captured
        assert tr_on.calibrating and tr_on.form_calibration.aside and tr_on.form_calibration.form == "in_step"
    assert tr_off.loss_sum is None and not tr_off.loss_readout
    for (k, p), q in zip(on.state_dict().items(), off.state_dict().values()):
        assert torch.equal(p, q), k


def _fit(mols, n_train, n_valid, device_metrics, epochs=2):
    """(fitter, result, what metrics.update saw): gin fitted from stores of the first n_train / n_valid molecules, batch 32."""
    from equihgnn_amd.batch import GraphStore
    from equihgnn_amd.fit import BucketedLoader, Fitter
    from equihgnn_amd.trainer import GraphedTrainStep
    fitter = Fitter(_gin(9), lr=3e-3, std=2.5, step_factory=GraphedTrainStep, metric_seed=6, device_metrics=device_metrics)
    seen = []
    if device_metrics:
        real = fitter.metrics.update

        def update(pred, target, scale=1.0):           # device clones: no read, the counter under test is not touched
            seen.append((fitter.metrics.position, pred.clone(), target.clone(), scale))
            real(pred, target, scale)
        fitter.metrics.update = update
    train = BucketedLoader(GraphStore(mols[:n_train]), 32, True, seed=0, device=DEV)
    valid = BucketedLoader(GraphStore(mols[:n_valid]), 32, False, device=DEV)
    res = fitter.fit(train, valid, epochs=epochs)
    return fitter, res, seen


@pytest.fixture(scope="module")
def fit_on(mols):
    return _fit(mols, 96, 40, True)


@pytest.fixture(scope="module")
def fit_off(mols):
    return _fit(mols, 96, 40, False)


def test_fitter_train_loss_is_bitwise_that_of_the_per_batch_reads(fit_on, fit_off):
    from equihgnn_amd.fit import BootstrapMetrics, DeviceBootstrapMetrics
    (f_on, r_on, _), (f_off, r_off, _) = fit_on, fit_off
    assert isinstance(f_on.metrics, DeviceBootstrapMetrics) and isinstance(f_off.metrics, BootstrapMetrics)
    assert f_on.step.loss_readout and not f_off.step.loss_readout and f_off.step.loss_sum is None
    assert [list(row) for row in r_on.history] == [list(row) for row in r_off.history]
    assert len(r_on.history) == 2
    for a, b in zip(r_on.history, r_off.history):
        assert a["train_loss"] == b["train_loss"] and np.isfinite(a["train_loss"])
        assert a["lr"] == b["lr"]
    assert r_on.history[0]["train_loss"] != r_on.history[1]["train_loss"]
    assert f_on.step.loss_sum.tolist() == [0.0, 0.0]                  # read once per epoch, then zeroed


def test_fitter_bootstrap_metrics_equal_numpy_over_the_host_weights(fit_on):
    from equihgnn_amd import ops
    fitter, res, seen = fit_on
    assert len(seen) == 2 * 2 and [s[0] for s in seen] == [0, 32, 0, 32]      # 40 molecules: 32 + 8, positions in loader order
    for epoch, row in enumerate(res.history):
        sums = np.zeros((3, 50))
        for pos, pred, target, scale in seen[2 * epoch:2 * epoch + 2]:
            assert scale == 2.5
            p, t = pred.cpu().numpy().reshape(-1), target.cpu().numpy().reshape(-1)
            assert len(p) == (32 if pos == 0 else 8)
            sums += _expected(p, t, scale, 6, pos, 50)
        mae, mse = sums[0] / np.maximum(sums[2], 1.0), sums[1] / np.maximum(sums[2], 1.0)
        want = {"val_mae_mean": mae.mean(), "val_mae_std": mae.std(ddof=1), "val_mse_mean": mse.mean(),
                "val_mse_std": mse.std(ddof=1)}
        for k, v in want.items():
            print(f"epoch {epoch} {k}: {row[k]!r} against numpy {v!r}")
            assert abs(row[k] - v) <= 1e-9 * abs(v) and v > 0.0, (epoch, k)


def test_fitter_reads_do_not_grow_with_the_number_of_batches(mols, fit_on, fit_off):
    reads_on, reads_off = fit_on[0].host_reads, fit_off[0].host_reads
    twice_on, twice_off = _fit(mols, 192, 80, True)[0].host_reads, _fit(mols, 192, 80, False)[0].host_reads
    print(f"host reads, 2 epochs: on {reads_on} / {twice_on}, off {reads_off} / {twice_off} (96 / 192 molecules)")
    assert reads_on == twice_on == 2 * 2                              # per epoch: the loss pair, the 3 x 64 sums
    assert reads_off == 2 * (3 + 2 * 2) and twice_off == 2 * (6 + 2 * 3)      # per batch: the loss; predictions and targets
    assert twice_off > reads_off


def test_fitter_test_table_is_bitwise_that_of_the_per_batch_copies(mols, fit_on, fit_off):
    from equihgnn_amd.batch import GraphStore
    from equihgnn_amd.fit import BucketedLoader
    tables, reads = [], []
    for fitter, _, _ in (fit_on, fit_off):
        before = fitter.host_reads
        metrics, table = fitter.test(BucketedLoader(GraphStore(mols[90:160]), 32, False, device=DEV))
        reads.append(fitter.host_reads - before)
        assert all(np.isfinite(v) for v in metrics.values()) and list(metrics) == [
            "test_mae_mean", "test_mae_std", "test_mse_mean", "test_mse_std"]
        tables.append(table)
    assert tables[0].shape == (70, 2) and tables[0].dtype == tables[1].dtype
    assert np.array_equal(tables[0], tables[1])
    assert np.array_equal(tables[0][:, 1], np.array([m.y for m in mols[90:160]], dtype=np.float32))
    assert reads == [2, 3 * 4]                                        # the table and the sums; four reads for each of 3 batches
