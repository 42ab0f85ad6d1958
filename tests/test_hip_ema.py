"""The exponential moving average (EMA) of the weights on the device: the EMA form of the update kernel (csrc/optim.hip:
eqh_adam_step_ema / eqh_adam_step_clip_ema, ``trainer.FlatAdam(ema_decay=..)``) against a float64 restatement of the
recurrence, the in-place exchange (eqh_swap_f32), the average inside the captured step
(``trainer.GraphedTrainStep(ema_decay=..)``), evaluation on it through ``averaged()`` without a re-capture, and
``fit.Fitter(ema_decay=..)``.

The bound.  With t = 1..T the updates, p_t the kernel's own parameters after update t and M = max_t |p_t| ELEMENTWISE, the
average is held to ``|e - e64| <= 4 T 2^-24 M``, e64 the recurrence e_1 = p_1, e_t = e_{t-1} + (1 - d_t)(p_t - e_{t-1}) in
float64.  The kernel's order of operations is subtract, scale, add -- three fp32 roundings per update (no contraction: the
library is built with -ffp-contract=off) on magnitudes of at most 2 M (the average is a convex combination of the p_t, so
|p_t - e| <= 2 M and |e_t| <= M); the weight 1 - d_t is formed in double and rounded once.  Update 1 is a copy and rounds
nothing; the contraction of earlier errors by d_t is ignored."""
import contextlib

import numpy as np
import pytest
import torch

from golden.common import fill_state_dict, golden_args, trajectory_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, MARK = 64, 7.25
NAME, HIDDEN, SEED, LR = "trajectory_egnn_equihnns_c64_b", 64, 107, 1e-3
# adam_step's launch line: 16 elements per thread, 256 threads, at most 2048 workgroups -> 8 388 608 elements per trip;
# 4096 more are one full second trip of workgroup 0, 3 more the ragged tail
SIZES = [3, 70003, 2048 * 256 * 16 + 4096 + 3]
ADAM = ("eqh_adam_step", "eqh_adam_step_clip", "eqh_adam_step_ema", "eqh_adam_step_clip_ema", "eqh_grad_sumsq", "eqh_swap_f32")


@contextlib.contextmanager
def _counting(*names):
    from equihgnn_amd import hip
    lib, calls = hip.lib(), {n: 0 for n in names}
    with pytest.MonkeyPatch.context() as mp:
        for n in names:
            def counted(*a, _n=n, _inner=getattr(lib, n)):
                calls[_n] += 1
                return _inner(*a)
            mp.setattr(lib, n, counted, raising=True)
        yield calls


def _guarded(n, dtype=torch.float32, guard=GUARD):
    """a buffer of n elements with ``guard`` marked elements behind it: (the whole allocation, its head)"""
    buf = torch.full((n + guard,), MARK, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _d_t(decay, t, warmup):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def _recurrence(snaps, decay, warmup):
    """(e64, M): the float64 recurrence over the snapshots p_1..p_T, and max_t |p_t| elementwise"""
    e64 = snaps[0].double()
    peak = snaps[0].abs().double()
    for t, s in enumerate(snaps[1:], start=2):
        s64 = s.double()
        e64 = e64 + (1.0 - _d_t(decay, t, warmup)) * (s64 - e64)
        peak = torch.maximum(peak, s64.abs())
    return e64, peak


def _assert_average(e, snaps, decay, warmup, what):
    T = len(snaps)
    e64, peak = _recurrence(snaps, decay, warmup)
    err = (e.double() - e64).abs()
    over = err - 4.0 * T * 2.0 ** -24 * peak
    worst = int(over.argmax())
    print(what, "max |e - e64|", float(err.max()), "largest err / bound",
          float((err / (4.0 * T * 2.0 ** -24 * peak).clamp(min=1e-300)).max()))
    assert float(over[worst]) <= 0.0, (what, worst, float(err[worst]), float(peak[worst]))


# ---- 1. the kernel against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("warmup", [False, True])
def test_flat_adam_ema_is_the_float64_recurrence_and_leaves_the_update_alone(n, clip, warmup):
    """Five steps of growing gradients with weight decay, grad_scale 0.25 and the gradient cleared in the step; every device
    buffer (the average included) has guard floats behind it.  Parameters and both moments: bit for bit those of the entry
    without the average on the same inputs, after every step.  With warm-up the average's buffer is filled with NaN before
    step 1 (update 1 copies whatever it held); without, it stays the constructor's clone.  When clipping, the threshold is
    half the first step's norm, so the clip is active."""
    from equihgnn_amd.trainer import FlatAdam
    decay, T = 0.9, 5
    gen = torch.Generator(device=DEV).manual_seed(11 + n % 7)
    w0 = torch.randn(n, generator=gen, device=DEV)
    grads = [torch.randn(n, generator=gen, device=DEV) * (0.5 + t) for t in range(T)]
    c = 0.5 * float(torch.linalg.vector_norm((0.25 * grads[0]).double())) if clip else None
    kw = dict(lr=1e-2, weight_decay=0.1, max_grad_norm=c)

    def set_up(opt):
        opt.grad_scale, opt.zero_grad_in_step = 0.25, True
    # the entry without the average
    p0 = torch.nn.Parameter(w0.clone())
    p0.grad = torch.zeros_like(w0)
    o0 = FlatAdam(p0, **kw)
    set_up(o0)
    assert "ema" not in o0.state[p0]
    ref = []
    for gr in grads:
        p0.grad.copy_(gr)
        o0.step()
        ref.append((p0.detach().clone(), o0.state[p0]["exp_avg"].clone(), o0.state[p0]["exp_avg_sq"].clone()))
    # ... and with it, every buffer guarded
    whole, heads = zip(*[_guarded(n) for _ in range(5)])
    heads[0].copy_(w0)
    heads[2].zero_()
    heads[3].zero_()
    p1 = torch.nn.Parameter(heads[0])
    p1.grad = heads[1]
    o1 = FlatAdam(p1, ema_decay=decay, ema_warmup=warmup, **kw)
    set_up(o1)
    st = o1.state[p1]
    assert torch.equal(st["ema"], w0) and st["ema"].data_ptr() != p1.data_ptr()
    heads[4].copy_(st["ema"])
    st["exp_avg"], st["exp_avg_sq"], st["ema"] = heads[2], heads[3], heads[4]
    whole, sizes = list(whole), [n] * 5
    if clip:
        part_whole, part = _guarded(st["clip_partials"].numel(), torch.float64, GUARD // 2)
        read_whole, read = _guarded(4)
        read.zero_()
        st["clip_partials"], o1.grad_norm = part, read
        whole += [part_whole, read_whole]
        sizes += [part.numel(), 4]
    if warmup:
        st["ema"].fill_(float("nan"))
    snaps = []
    with _counting(*ADAM) as calls:
        for t, gr in enumerate(grads):
            p1.grad.copy_(gr)
            o1.sync_lr()
            o1.step()
            snaps.append(p1.detach().clone())
            for got, want, k in zip((p1.detach(), st["exp_avg"], st["exp_avg_sq"]), ref[t], ("param", "exp_avg", "exp_avg_sq")):
                assert torch.equal(got, want), (k, t)
            assert not bool(p1.grad.any())                          # cleared by the update
            if t == 0:
                assert torch.equal(st["ema"], p1.detach())          # update 1 copies
    twin, mine = ("eqh_adam_step_clip", "eqh_adam_step_clip_ema") if clip else ("eqh_adam_step", "eqh_adam_step_ema")
    assert calls == {**{k: 0 for k in ADAM}, mine: T, "eqh_grad_sumsq": T if clip else 0}, (calls, twin)
    assert bool(torch.isfinite(st["ema"]).all())
    _assert_average(st["ema"], snaps, decay, warmup, f"n={n} clip={clip} warmup={warmup}")
    assert st["step_block"].tolist() == [T, 0]
    if clip:
        assert o1.grad_norm.tolist()[3] == T                        # clipped at every step
    for buf, head in zip(whole, sizes):
        assert bool((buf[head:] == MARK).all())


# ---- 2. eqh_swap_f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_two_buffers_in_place_and_is_capturable(n):
    from equihgnn_amd import hip, ops
    L = hip.lib()
    gen = torch.Generator(device=DEV).manual_seed(3 + n % 5)
    (wa, a), (wb, b) = _guarded(n), _guarded(n)
    a.copy_(torch.randn(n, generator=gen, device=DEV))
    b.copy_(torch.randn(n, generator=gen, device=DEV))
    a[0], b[n - 1] = float("nan"), float("-inf")                     # bits, not values
    a0, b0 = a.clone().view(torch.int32), b.clone().view(torch.int32)

    def swap():
        hip.check(L.eqh_swap_f32(ops._ptr(a), ops._ptr(b), n, ops._stream(a.device)), "eqh_swap_f32")

    def state():
        return torch.equal(a.view(torch.int32), a0), torch.equal(a.view(torch.int32), b0), \
            torch.equal(b.view(torch.int32), b0), torch.equal(b.view(torch.int32), a0)
    swap()
    assert state() == (False, True, False, True)
    swap()
    assert state() == (True, False, True, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        swap()
        swap()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        swap()
    assert state() == (True, False, True, False)                     # captured, not run
    g.replay()
    assert state() == (False, True, False, True)
    g.replay()
    assert state() == (True, False, True, False)
    assert bool((wa[n:] == MARK).all()) and bool((wb[n:] == MARK).all())


# ---- 3. inside the captured step -------------------------------------------------------------------------------------------
STEPS = 6


def _model_and_batches():
    from equihgnn_amd.batch import bucket_sizes, pad_batch
    from equihgnn_amd.models import MODELS
    model = MODELS["mhnns"](1, golden_args("mhnns", HIDDEN))
    fill_state_dict(model, SEED)
    model.to(DEV).train()
    raw = trajectory_batches(NAME)
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz, 64) for b in raw]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    return model, [pad_batch(b, *tgt).to(DEV) for b in raw]


def _graphed_run(clip):
    """Six steps of GraphedTrainStep(ema_decay=0.9, keep_grads=False): the eager bootstrap, the capture and four replays;
    ``pflat`` after every step, and the native calls made behind the bootstrap."""
    from equihgnn_amd.trainer import GraphedTrainStep
    model, batches = _model_and_batches()
    tr = GraphedTrainStep(model, lr=LR, ema_decay=0.9, keep_grads=False, clip_gnorm=clip)
    with pytest.raises(RuntimeError, match="no optimiser yet"):
        tr.ema_state_dict()
    snaps = []
    with _counting(*ADAM) as boot:
        tr.step(batches[0])
        snaps.append(tr.pflat.detach().clone())
    assert torch.equal(tr.ema_flat, snaps[0])                        # update 1 copies
    with _counting(*ADAM) as calls:
        for t in range(1, STEPS):
            tr.step(batches[t % len(batches)])
            snaps.append(tr.pflat.detach().clone())
    torch.cuda.synchronize()
    return {"tr": tr, "model": model, "batches": batches, "snaps": snaps, "boot": boot, "calls": calls,
            "ema": tr.ema_flat.clone()}


@pytest.fixture(scope="module")
def run():
    out = _graphed_run(None)
    yield out
    out["tr"].close()


def test_graphed_step_keeps_the_average_in_the_captured_update(run):
    tr, snaps = run["tr"], run["snaps"]
    graphs = len(tr.slots) + len(getattr(tr.form_calibration, "aside", None) or {})     # (those set aside while the second form is timed)
    assert graphs >= 1 and len(snaps) == STEPS
    mine = "eqh_adam_step_ema"
    assert run["boot"] == {**{k: 0 for k in ADAM}, mine: 1}
    assert run["calls"] == {**{k: 0 for k in ADAM}, mine: graphs}     # once per captured graph; a replay calls nothing
    assert all(not torch.equal(snaps[t], snaps[t + 1]) for t in range(STEPS - 1))
    assert tr.opt.state[tr.pflat]["step_block"].tolist() == [STEPS, 0]
    _assert_average(run["ema"], snaps, 0.9, False, "graphed step")
    assert not torch.equal(run["ema"], snaps[-1])
    assert "ema" in tr.opt.state_dict()["state"][0]


def test_graphed_step_with_an_unreachable_threshold_keeps_the_same_average(run):
    other = _graphed_run(1e30)
    try:
        tr = other["tr"]
        graphs = len(tr.slots) + len(getattr(tr.form_calibration, "aside", None) or {})     # (those set aside while the second form is timed)
        mine = "eqh_adam_step_clip_ema"
        assert other["boot"] == {**{k: 0 for k in ADAM}, mine: 1, "eqh_grad_sumsq": 1}
        assert other["calls"] == {**{k: 0 for k in ADAM}, mine: graphs, "eqh_grad_sumsq": graphs}
        for t in range(STEPS):
            assert torch.equal(other["snaps"][t], run["snaps"][t]), t
        assert torch.equal(other["ema"], run["ema"])
    finally:
        other["tr"].close()


# ---- 4. evaluating on the average ------------------------------------------------------------------------------------------
def test_evaluation_inside_averaged_replays_the_same_graphs_on_the_average(run):
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.trainer import GraphedEvalStep
    tr, model, data = run["tr"], run["model"], run["batches"][1]
    before = tr.pflat.detach().clone()
    second = MODELS["mhnns"](1, golden_args("mhnns", HIDDEN)).to(DEV)
    second.load_state_dict(tr.ema_state_dict())
    assert torch.equal(tr.pflat.detach(), before)                    # ema_state_dict() does not disturb the live weights
    second.eval()
    want = GraphedEvalStep(second)(data).clone()
    model.eval()
    try:
        ev = GraphedEvalStep(model)
        with _counting("eqh_swap_f32") as calls:
            got = []
            for cycle in range(2):
                with tr.averaged():
                    assert torch.equal(tr.pflat.detach(), run["ema"])
                    with pytest.raises(RuntimeError, match="already inside"):
                        with tr.averaged():
                            pass
                    got.append(ev(data).clone())
                assert torch.equal(tr.pflat.detach(), before) and torch.equal(tr.ema_flat, run["ema"])
                live = ev(data).clone()
        assert calls == {"eqh_swap_f32": 4}
        with pytest.raises(ZeroDivisionError):
            with tr.averaged():
                1 / 0
        assert torch.equal(tr.pflat.detach(), before) and torch.equal(tr.ema_flat, run["ema"])
        assert ev.recaptures == 0 and len(ev.slots) == 1
        for g in got:
            assert torch.equal(g.view(torch.int32), want.view(torch.int32))
        assert not torch.equal(live, want) and bool(torch.isfinite(live).all())
    finally:
        model.train()


def test_averaged_and_ema_state_dict_need_a_decay():
    from equihgnn_amd.trainer import GraphedTrainStep
    model, _ = _model_and_batches()
    tr = GraphedTrainStep(model, lr=LR)
    for call in (tr.ema_state_dict, lambda: tr.averaged().__enter__()):
        with pytest.raises(RuntimeError, match="without ema_decay"):
            call()


# ---- 5. Fitter -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    from equihgnn_amd.batch import MolStore, synth_molecule
    rng = np.random.default_rng(41)
    mols = [synth_molecule(rng, "qm9") for _ in range(64)]
    n = np.array([m.x.shape[0] for m in mols], dtype=np.float64)
    for m, v in zip(mols, (n - n.mean()) / n.std()):
        m.y = float(np.float32(v))
    return MolStore(mols).to_device(DEV)


def _fitter(store, **kw):
    from equihgnn_amd.fit import BucketedLoader, Fitter
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.trainer import GraphedTrainStep
    model = MODELS["mhnns"](1, golden_args("mhnns", HIDDEN))
    fill_state_dict(model, SEED)
    model.to(DEV).train()
    fitter = Fitter(model, lr=3e-3, std=1.0, step_factory=GraphedTrainStep, device_metrics=True, **kw)
    train = BucketedLoader(store.subset(list(range(48))), 16, True, seed=0)
    valid = BucketedLoader(store.subset(list(range(48, 64))), 16, False)
    return model, fitter, train, valid


def test_fitter_evaluates_and_checkpoints_the_average(store):
    model, fitter, train, valid = _fitter(store, ema_decay=0.9)
    clone = lambda sd: {k: v.detach().clone() for k, v in sd.items()}
    epochs, real = [], fitter.step.averaged

    @contextlib.contextmanager
    def recording():
        epochs.append({"ema": fitter.step.ema_state_dict(), "live": clone(model.state_dict())})
        with real() as s:
            yield s
    fitter.step.averaged = recording
    res = fitter.fit(train, valid, epochs=2)
    assert len(epochs) == 2 and len(res.history) == 2 and model.training
    best = epochs[res.best_epoch]
    assert list(res.best_state) == list(best["ema"])
    assert all(torch.equal(v, best["ema"][k]) for k, v in res.best_state.items())
    assert any(not torch.equal(v, best["live"][k]) for k, v in res.best_state.items())
    tr = fitter.step
    before, ema = tr.pflat.detach().clone(), tr.ema_flat.clone()
    with _counting("eqh_swap_f32") as calls:
        val = fitter._evaluate(valid)
    assert calls == {"eqh_swap_f32": 2} and len(epochs) == 3
    assert torch.equal(tr.pflat.detach(), before) and torch.equal(tr.ema_flat, ema)
    assert model.training and np.isfinite(val["mae_mean"])
    assert fitter.eval_step is not None and fitter.eval_step.recaptures == 0
    tr.close()


def test_fitter_without_a_decay_makes_none_of_the_new_calls(store):
    model, fitter, train, valid = _fitter(store)
    with _counting(*ADAM) as calls:
        res = fitter.fit(train, valid, epochs=1)
    assert len(res.history) == 1
    assert calls["eqh_adam_step"] >= 2
    assert {k: v for k, v in calls.items() if k != "eqh_adam_step"} == {k: 0 for k in ADAM if k != "eqh_adam_step"}
    tr = fitter.step
    assert tr.ema_decay is None and tr.ema_flat is None and "ema" not in tr.opt.state[tr.pflat]
    with pytest.raises(RuntimeError, match="without ema_decay"):
        tr.ema_state_dict()
    tr.close()
