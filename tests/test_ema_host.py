"""The exponential moving average (EMA) of the weights, host side (no GPU): the argument checks of the three native entry
points (eqh_adam_step_ema, eqh_adam_step_clip_ema, eqh_swap_f32), which return before anything is launched; the decay checks
of ``FlatAdam`` / ``TrainStep`` / ``Fitter``; ``TrainStep(ema_decay=..)`` on the CPU oracle against
``torch.optim.swa_utils.AveragedModel`` and against a float64 restatement of the recurrence; ``averaged()``; and a
``Fitter(ema_decay=..)`` fit whose checkpoint holds averaged parameters with live BatchNorm buffers.

The bound of the comparisons (T updates, per parameter tensor): elementwise ``|e - e_ref| <= 4 T 2^-24 max_t |p_t|`` -- three
fp32 roundings per update (subtract, scale, add) on magnitudes of at most 2 max |p|; the contraction by the decay is ignored."""
import contextlib
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle  # noqa: F401
from equihgnn_amd.batch import synth_molecule
from equihgnn_amd.trainer import TrainStep, ema_decay_at
from golden.common import fill_state_dict, golden_args, trajectory_batches
from oracle import ref_models as O

NAME = "trajectory_egnn_equihnns_c64_b"
STEPS = 5
BAD_DECAYS = (1.0, -0.1, float("nan"))


def _bound(T, peak):
    return 4.0 * T * 2.0 ** -24 * peak


def _oracle(method="mhnns", hidden=32, seed=107, **kw):
    model = O.MODELS[method](1, golden_args(method, hidden, **kw))
    fill_state_dict(model, seed)
    return model.train()


# ---- header, library, argument checks --------------------------------------------------------------------------------------
def test_native_entry_points_are_bound_and_check_their_arguments():
    from equihgnn_amd import hip
    L = hip.lib()
    for name in ("eqh_adam_step_ema", "eqh_adam_step_clip_ema", "eqh_swap_f32"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    assert len(hip.SIGNATURES["eqh_adam_step_ema"][1]) == len(hip.SIGNATURES["eqh_adam_step"][1]) + 3
    assert len(hip.SIGNATURES["eqh_adam_step_clip_ema"][1]) == len(hip.SIGNATURES["eqh_adam_step_clip"][1]) + 3
    held = ctypes.create_string_buffer(512)          # addresses that are never read: no call below gets as far as a launch
    ok = (ctypes.addressof(held) + 15) // 16 * 16
    other = ok + 256

    def plain(ema=ok, decay=0.9, warmup=0, n=4, grad=ok, lr=ok):
        return L.eqh_adam_step_ema(ok, grad, ok, ok, n, lr, 0.9, 0.999, 1e-8, 0.0, 1.0, ok, 0, None, 0,
                                   ema, decay, warmup, None)

    def clip(ema=ok, decay=0.9, warmup=0, n=4, grad=ok, partials=ok, max_norm=5.0, readout=ok):
        return L.eqh_adam_step_clip_ema(ok, grad, ok, ok, n, ok, 0.9, 0.999, 1e-8, 0.0, 1.0, ok, 0, None, 0,
                                        partials, max_norm, readout, ema, decay, warmup, None)
    for entry in (plain, clip):
        assert entry(ema=None) == hip.EQH_ERR_ARG
        for bad in BAD_DECAYS + (1.5, float("inf")):
            assert entry(decay=bad) == hip.EQH_ERR_ARG, bad
            assert entry(decay=bad, n=0) == hip.EQH_ERR_ARG, bad      # (checked ahead of the empty-tensor return)
        assert entry(ema=ok + 4) == hip.EQH_ERR_ALIGN
        assert entry(n=0) == hip.EQH_OK and entry(n=0, ema=None) == hip.EQH_OK      # nothing to update, nothing launched
        assert entry(n=0, decay=0.0, warmup=1) == hip.EQH_OK
        # ... and the twin's own checks hold
        assert entry(n=-1) == hip.EQH_ERR_ARG and entry(grad=None) == hip.EQH_ERR_ARG
        assert entry(grad=ok + 4) == hip.EQH_ERR_ALIGN
    assert plain(lr=None) == hip.EQH_ERR_ARG
    assert clip(partials=None) == hip.EQH_ERR_ARG and clip(readout=None) == hip.EQH_ERR_ARG
    assert clip(max_norm=0.0) == hip.EQH_ERR_ARG and clip(partials=ok + 4) == hip.EQH_ERR_ALIGN
    swap = L.eqh_swap_f32
    assert swap(ok, other, 0, None) == hip.EQH_OK and swap(None, None, 0, None) == hip.EQH_OK
    assert swap(ok, other, -1, None) == hip.EQH_ERR_ARG
    assert swap(None, other, 4, None) == hip.EQH_ERR_ARG and swap(ok, None, 4, None) == hip.EQH_ERR_ARG
    assert swap(ok, ok, 4, None) == hip.EQH_ERR_ARG                       # the same buffer
    assert swap(ok, ok + 16, 8, None) == hip.EQH_ERR_ARG                  # two ranges that overlap
    assert swap(ok + 16, ok, 8, None) == hip.EQH_ERR_ARG
    assert swap(ok + 4, other, 4, None) == hip.EQH_ERR_ALIGN
    assert swap(ok, other + 4, 4, None) == hip.EQH_ERR_ALIGN


@pytest.mark.parametrize("bad", BAD_DECAYS)
def test_a_decay_outside_the_unit_interval_is_refused(bad):
    from equihgnn_amd.fit import Fitter
    from equihgnn_amd.trainer import FlatAdam
    with pytest.raises(ValueError, match="ema_decay must lie in"):
        FlatAdam(torch.nn.Parameter(torch.zeros(8)), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay must lie in"):
        TrainStep(torch.nn.Linear(2, 1), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay must lie in"):
        Fitter(torch.nn.Linear(2, 1), ema_decay=bad)


# ---- TrainStep on the CPU oracle -------------------------------------------------------------------------------------------
def test_train_step_ema_equals_averaged_model():
    """Five steps, decay 0.9: the shadows against torch's own EMA of the same model, updated after every step."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    model = _oracle()
    batches = trajectory_batches(NAME)
    tr = TrainStep(model, lr=1e-2, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no optimiser yet"):
        tr.ema_state_dict()
    with pytest.raises(RuntimeError, match="no optimiser yet"):
        with tr.averaged():
            pass
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    peak = {k: 0.0 for k, _ in model.named_parameters()}
    for t in range(STEPS):
        tr.step(batches[t % len(batches)])
        avg.update_parameters(model)
        for k, p in model.named_parameters():
            peak[k] = max(peak[k], float(p.detach().abs().max()))
    assert tr.ema_updates == STEPS and len(tr.ema_shadows) == len(tr.flat.params)
    ema, ref = tr.ema_state_dict(), dict(avg.module.named_parameters())
    live = {id(p) for p in tr.flat.params}
    moved = 0
    for k, p in model.named_parameters():
        err = float((ema[k] - ref[k].detach()).abs().max())
        print(k, "max |e - AveragedModel|", err, "bound", _bound(STEPS, peak[k]))
        assert err <= _bound(STEPS, peak[k]), k
        if id(p) in live:
            moved += int(not torch.equal(ema[k], p.detach()))
        else:
            assert torch.equal(ema[k], p.detach()), k         # never updated: its own average
    assert moved > 0
    # the buffers and the other entries of the state are the live ones, as clones
    sd = model.state_dict()
    assert list(ema) == list(sd)
    for k in set(sd) - set(ref):
        assert torch.equal(ema[k], sd[k]) and ema[k].data_ptr() != sd[k].data_ptr(), k


@pytest.mark.parametrize("decay,warmup", [(0.9, True), (0.999, True), (0.9, False), (0.0, False)])
def test_train_step_ema_equals_the_float64_recurrence(decay, warmup):
    """e_1 = p_1; e_t = e_{t-1} + (1 - d_t)(p_t - e_{t-1}), d_t = min(d, (1 + t) / (10 + t)) with warm-up, restated in float64
    from per-step snapshots of the live parameters.  (0.999 with warm-up: the warm-up governs all five steps; decay 0: the
    average is the last parameter.)"""
    model = _oracle()
    batches = trajectory_batches(NAME)
    tr = TrainStep(model, lr=1e-2, ema_decay=decay, ema_warmup=warmup)
    e64, peak = None, None
    for t in range(1, STEPS + 1):
        tr.step(batches[(t - 1) % len(batches)])
        snap = [p.detach().double().clone() for p in tr.flat.params]
        if t == 1:
            e64, peak = snap, [float(s.abs().max()) for s in snap]
        else:
            d_t = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
            assert ema_decay_at(decay, t, warmup) == d_t
            e64 = [e + (1.0 - d_t) * (s - e) for e, s in zip(e64, snap)]
            peak = [max(pk, float(s.abs().max())) for pk, s in zip(peak, snap)]
    for e, want, pk, p in zip(tr.ema_shadows, e64, peak, tr.flat.params):
        assert float((e.double() - want).abs().max()) <= _bound(STEPS, pk)
        if decay == 0.0:
            assert torch.equal(e, p.detach())
    if warmup and decay == 0.999:
        plain = TrainStep(_oracle(), lr=1e-2, ema_decay=decay)
        for t in range(STEPS):
            plain.step(batches[t % len(batches)])
        assert any(not torch.equal(a, b) for a, b in zip(plain.ema_shadows, tr.ema_shadows))


def test_without_a_decay_nothing_is_kept():
    model = _oracle()
    tr = TrainStep(model, lr=1e-2)
    tr.step(trajectory_batches(NAME)[0])
    assert tr.ema_decay is None and tr.ema_shadows is None and tr.ema_updates == 0
    with pytest.raises(RuntimeError, match="without ema_decay"):
        tr.ema_state_dict()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with tr.averaged():
            pass


def test_averaged_round_trip_restores_the_live_weights_bit_for_bit():
    model = _oracle()
    batches = trajectory_batches(NAME)
    tr = TrainStep(model, lr=1e-2, ema_decay=0.5)
    for t in range(3):
        tr.step(batches[t])
    live = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ema = tr.ema_state_dict()
    assert any(not torch.equal(live[k], ema[k]) for k in live)

    def same(a):
        return all(torch.equal(v, a[k]) for k, v in model.state_dict().items())
    with tr.averaged() as inside:
        assert inside is tr and same(ema) and not same(live)
        assert same(tr.ema_state_dict())                      # inside, the parameters themselves are the average
        with pytest.raises(RuntimeError, match="already inside"):
            with tr.averaged():
                pass
        assert same(ema)                                      # the refused entry exchanged nothing
        with pytest.raises(RuntimeError, match="inside averaged"):
            tr.step(batches[0])
    assert same(live)
    with pytest.raises(KeyError):
        with tr.averaged():
            assert same(ema)
            raise KeyError("from the body")
    assert same(live)
    after = tr.ema_state_dict()
    assert all(torch.equal(ema[k], after[k]) for k in ema)
    tr.step(batches[0])                                       # and training goes on from the live weights
    assert not same(live)


# ---- Fitter ----------------------------------------------------------------------------------------------------------------
def _data(seed, n=9):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(x=torch.randn(n, 5, generator=g), y=3.0 * torch.randn(n, generator=g))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(5, 1)

    def forward(self, data):
        return self.a(data.x).squeeze(-1)


def test_fitter_hands_the_keywords_over_only_when_given():
    from equihgnn_amd.fit import Fitter
    seen = []

    def old_factory(model, lr, weight_decay):
        seen.append((lr, weight_decay))
        return TrainStep(model, lr=lr, weight_decay=weight_decay)
    fitter = Fitter(_Net(), lr=1e-2, step_factory=old_factory)
    assert seen == [(1e-2, 0.0)] and fitter.ema_decay is None and fitter.step.ema_decay is None
    res = fitter.fit([_data(1), _data(2)], [_data(3)], epochs=1)
    assert res.best_state is not None and fitter.step.ema_shadows is None
    with pytest.raises(TypeError):
        Fitter(_Net(), lr=1e-2, step_factory=old_factory, ema_decay=0.9)
    got = Fitter(_Net(), lr=1e-2, ema_decay=0.9, ema_warmup=True).step
    assert got.ema_decay == 0.9 and got.ema_warmup is True


def test_fit_checkpoints_the_averaged_weights_with_the_live_buffers():
    """Two epochs of ``Fitter(ema_decay=0.5)`` on the CPU oracle of ``mhnnm`` (BatchNorm): every evaluation runs on the
    average, ``best_state`` is the averaged state of the best epoch -- parameters unlike the live ones, BatchNorm buffers
    the live ones -- and ``test`` without a state evaluates the average, with ``best_state`` the loaded weights as they are."""
    from equihgnn_amd.fit import Fitter, MolLoader
    rng = np.random.default_rng(5)
    mols = [synth_molecule(rng) for _ in range(40)]
    for m in mols:
        m.y = float(m.x.shape[0]) / 10.0
    model = _oracle("mhnnm", hidden=32, seed=85)
    assert any("running_mean" in k for k in model.state_dict())
    fitter = Fitter(model, lr=3e-3, ema_decay=0.5)
    clone = lambda sd: {k: v.detach().clone() for k, v in sd.items()}
    epochs, real = [], fitter.step.averaged

    @contextlib.contextmanager
    def recording():
        before = clone(model.state_dict())
        epochs.append({"live": before, "ema": fitter.step.ema_state_dict(), "training": model.training})
        with real() as s:
            yield s
        assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())      # evaluation moved nothing
    fitter.step.averaged = recording
    train, valid = MolLoader(mols[:24], 8, True, seed=0), MolLoader(mols[24:32], 8, False)
    res = fitter.fit(train, valid, epochs=2)
    assert len(epochs) == 2 and model.training                # one exchange per epoch: validation and checkpoint share it
    best = epochs[res.best_epoch]
    params = {k for k, _ in model.named_parameters()}
    assert list(res.best_state) == list(best["ema"])
    for k, v in res.best_state.items():
        assert torch.equal(v, best["ema"][k]), k
        if k not in params:
            assert torch.equal(v, best["live"][k]), k          # BatchNorm statistics, batch counters: the live ones
    assert any(not torch.equal(res.best_state[k], best["live"][k]) for k in params)
    assert any(k.endswith("running_mean") for k in res.best_state)
    # test(): the average when no state is given (one more exchange), the loaded state as it stands otherwise (none)
    te = MolLoader(mols[32:], 8, False)
    _, t_avg = fitter.test(te)
    assert len(epochs) == 3
    _, table = fitter.test(te, res.best_state)
    assert len(epochs) == 3 and table.shape == (8, 2) and np.isfinite(table).all()
    if res.best_epoch == 1:                                    # the last epoch's average IS the checkpoint
        assert np.array_equal(t_avg, table)
    plain = Fitter(_oracle("mhnnm", hidden=32, seed=85), lr=3e-3)
    res0 = plain.fit(MolLoader(mols[:24], 8, True, seed=0), MolLoader(mols[24:32], 8, False), epochs=2)
    assert [r["train_loss"] for r in res0.history] == [r["train_loss"] for r in res.history]   # training is untouched
    assert [r["val_mae_mean"] for r in res0.history] != [r["val_mae_mean"] for r in res.history]
