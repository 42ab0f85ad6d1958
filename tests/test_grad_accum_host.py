"""Gradient accumulation over k micro-batches, host side (no GPU): the ``accum_steps`` keyword of ``TrainStep``,
``GraphedTrainStep`` and ``Fitter``, ``TrainStep(accum_steps=k)`` on the CPU oracle model against a hand-written loop of
``(loss / k).backward()`` with one ``torch.optim.Adam.step()`` per k batches (Lightning's ``accumulate_grad_batches``),
``flush()`` on a trailing group, the ``optimizer_steps`` column of ``Fitter``, and the argument checks of eqh_add_many, which
return before anything is launched.  The two-rank gloo case is in test_grad_accum_gloo.py."""
import ctypes

import pytest
import torch

from equihgnn_amd.batch import synth_batch
from equihgnn_amd.trainer import GraphedTrainStep, TrainStep
from test_grad_clip_host import BASE_KEYS, _data, _Net
from test_trainer_gloo import _make_model

F = torch.nn.functional
LR = 1e-2


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2"])
def test_accum_steps_must_be_a_positive_integer(bad):
    from equihgnn_amd.fit import Fitter
    for build in (lambda: TrainStep(_Net(1), accum_steps=bad), lambda: GraphedTrainStep(_Net(1), accum_steps=bad),
                  lambda: Fitter(_Net(1), accum_steps=bad)):
        with pytest.raises(ValueError, match="accum_steps must be an integer >= 1"):
            build()


def test_accum_steps_defaults_to_one():
    from equihgnn_amd.fit import Fitter
    tr = TrainStep(_Net(1))
    assert tr.accum_steps == 1 and tr.micro == 0 and tr.updates == 0
    assert Fitter(_Net(1)).accum_steps == 1
    tr.flush()                              # no group is open: nothing happens, also before the first step
    assert tr.updates == 0 and tr.opt is None


@pytest.fixture
def one_thread():
    """The oracle's backward sums in an order that depends on the thread pool (as test_trainer_gloo.py notes); equality
    between two runs of it needs one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _batches(n):
    return [synth_batch(6, 700 + 10 * t) for t in range(n)]


def _hand_loop(model, batches, k, groups):
    """Lightning's loop: (loss / k).backward() per batch, Adam.step() + zero_grad() after every k-th, and once more on what an
    open group holds (``groups``: the batch counts of the groups, e.g. [2, 1] for a trailing group of one at k = 2).  Returns
    the losses and, per group, the gradients the optimiser saw."""
    opt, losses, seen, it = None, [], [], iter(batches)
    for size in groups:
        for p in model.parameters():
            p.grad = None
        for _ in range(size):
            data = next(it)
            loss = F.mse_loss(model(data), data.y)
            (loss / k).backward()
            losses.append(float(loss.detach()))
        if opt is None:     # (parameters of dead branches never receive a gradient: Adam skips them, TrainStep leaves them out)
            opt = torch.optim.Adam(list(model.parameters()), lr=LR)
        seen.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        opt.step()
    return losses, seen


@pytest.mark.parametrize("k", [2, 4])
def test_train_step_accumulates_like_the_loss_over_k_loop_bit_for_bit(k, one_thread):
    """Two groups of k.  Scaling by a power of two commutes with every sum and product of the backward pass, so the sum of
    k gradients times 1 / k IS the sum of the k gradients of loss / k: equality of every parameter, not closeness."""
    batches = _batches(2 * k)
    mine, ref = _make_model(3), _make_model(3)
    tr = TrainStep(mine, lr=LR, accum_steps=k)
    before = {n: p.detach().clone() for n, p in mine.named_parameters()}
    losses = []
    for t, data in enumerate(batches):
        losses.append(float(tr.step(data)))
        assert tr.micro == (t + 1) % k and tr.updates == (t + 1) // k
        if t < k - 1:       # the weights do not move inside a group
            assert all(torch.equal(p, before[n]) for n, p in mine.named_parameters())
    want, _ = _hand_loop(ref, batches, k, [k, k])
    assert losses == want                   # each micro-batch's own loss, unscaled
    moved = 0
    for (n, p), q in zip(mine.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n
        moved += int(not torch.equal(p, before[n]))
    assert moved > 0 and tr.updates == 2


def test_train_step_with_three_micro_batches_matches_the_loop_to_rounding(one_thread):
    """k = 3: 1 / 3 is no power of two, so the loop's gradient of loss / 3 and the step's (sum of three) * (1 / 3) differ by
    roundings -- of the final multiply here, of every product along the backward pass there.  Those are relative to a
    tensor's magnitude, not to an element that is the small difference of larger terms, so the bound is
    max |g - g_loop| <= 1e-6 max |g_loop| per parameter tensor.  Adam's m / sqrt(v) turns a rounding of a near-zero gradient
    element into an O(lr) difference of the parameter, so the update is checked the other way round: a mirror Adam fed the
    step's OWN gradient of each group gives the step's parameters bit for bit (one update per group, on that gradient)."""
    k, batches = 3, _batches(6)
    mine, ref, mirror = _make_model(3), _make_model(3), _make_model(3)
    tr = TrainStep(mine, lr=LR, accum_steps=k)
    names = {id(p): n for n, p in mine.named_parameters()}
    live, opt = dict(mirror.named_parameters()), None
    for g in range(2):
        # the loop's gradient ON THE STEP'S WEIGHTS (equal to the mirror's, asserted below): after an update the two runs'
        # weights differ by Adam's amplified roundings, and a gradient taken elsewhere says nothing about the sum
        ref.load_state_dict(mine.state_dict())
        _, seen = _hand_loop(ref, batches[k * g:k * g + k], k, [k])
        for data in batches[k * g:k * g + k]:
            tr.step(data)
        assert tr.micro == 0 and tr.updates == g + 1
        assert sorted(names[id(p)] for p in tr.flat.params) == sorted(seen[0])
        for p in tr.flat.params:
            want = seen[0][names[id(p)]]
            err = float((p.grad - want).abs().max())
            assert err <= 1e-6 * float(want.abs().max()), (g, names[id(p)], err)
            live[names[id(p)]].grad = p.grad.clone()
        if opt is None:
            opt = torch.optim.Adam([live[names[id(p)]] for p in tr.flat.params], lr=LR)
        opt.step()
        for n, p in mine.named_parameters():
            assert torch.equal(p, live[n]), (g, n)


def test_flush_closes_a_trailing_group_with_the_scale_of_a_full_one(one_thread):
    """k = 2 over three batches: the third is a group of one, closed by flush(): the loop's loss / 2 step."""
    batches = _batches(3)
    mine, ref = _make_model(5), _make_model(5)
    tr = TrainStep(mine, lr=LR, accum_steps=2)
    for data in batches:
        tr.step(data)
    assert tr.micro == 1 and tr.updates == 1
    tr.flush()
    assert tr.micro == 0 and tr.updates == 2
    _hand_loop(ref, batches, 2, [2, 1])
    for (n, p), q in zip(mine.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n
    held = [p.detach().clone() for p in mine.parameters()]
    tr.flush()                              # nothing is open: nothing happens
    assert tr.updates == 2 and all(torch.equal(p, h) for p, h in zip(mine.parameters(), held))


def test_averaged_weights_are_updated_once_per_group():
    tr = TrainStep(_Net(2), lr=LR, accum_steps=2, ema_decay=0.5)
    for t in range(4):
        tr.step(_data(20 + t))
        if t == 2:          # inside an open group the weights have not moved: the average is a whole state
            with tr.averaged():
                pass
            assert tr.micro == 1
    assert tr.updates == 2 and tr.ema_updates == 2


def test_fitter_flushes_at_the_end_of_an_epoch_and_counts_optimizer_steps():
    from equihgnn_amd.fit import Fitter
    train, valid = [_data(60 + t) for t in range(5)], [_data(70)]
    seen_kw = []

    def factory(model, lr, weight_decay, **kw):
        seen_kw.append(kw)
        return TrainStep(model, lr=lr, weight_decay=weight_decay, **kw)
    fitter = Fitter(_Net(4), lr=LR, step_factory=factory, accum_steps=2)
    losses, micro_at_eval = [], []
    real_step, real_eval = fitter.step.step, fitter._evaluate

    def step(data):
        loss = real_step(data)
        losses.append(float(loss))
        return loss
    fitter.step.step = step
    fitter._evaluate = lambda loader: (micro_at_eval.append(fitter.step.micro), real_eval(loader))[1]
    res = fitter.fit(train, valid, epochs=2)
    assert seen_kw == [{"accum_steps": 2}]
    assert [list(row) for row in res.history] == [BASE_KEYS + ["optimizer_steps"]] * 2
    assert micro_at_eval == [0, 0]          # the group of one was closed before the validation pass
    for e, row in enumerate(res.history):
        assert row["optimizer_steps"] == 3 and isinstance(row["optimizer_steps"], int)
        assert row["train_loss"] == pytest.approx(sum(losses[5 * e:5 * e + 5]) / 5, rel=1e-12)
    assert fitter.step.updates == 6
    # without the keyword the factory sees none and the rows are those of before
    seen_kw.clear()
    res = Fitter(_Net(4), lr=LR, step_factory=factory).fit(train, valid, epochs=1)
    assert seen_kw == [{}] and [list(row) for row in res.history] == [BASE_KEYS]


def test_add_many_is_declared_bound_and_checks_its_arguments():
    from equihgnn_amd import hip, ops
    L = hip.lib()
    assert "eqh_add_many" in hip.SIGNATURES and hasattr(L, "eqh_add_many") and callable(ops.add_many)
    res, args = hip.SIGNATURES["eqh_add_many"]
    assert res is ctypes.c_int and len(args) == len(hip.SIGNATURES["eqh_copy_many"][1]) + 2
    held = ctypes.create_string_buffer(256)          # addresses that are never read: no call below gets as far as a launch
    ok = (ctypes.addressof(held) + 15) // 16 * 16
    one = (ctypes.c_void_p * 1)(ok)
    n4 = (ctypes.c_int64 * 1)(4)
    assert L.eqh_add_many(-1, one, one, n4, None, 0, None) == hip.EQH_ERR_ARG
    assert L.eqh_add_many(1, one, one, n4, ok, 6, None) == hip.EQH_ERR_ARG          # no multiple of 4
    assert L.eqh_add_many(1, one, one, n4, None, 4, None) == hip.EQH_ERR_ARG        # nothing to clear 4 floats of
    assert L.eqh_add_many(1, one, one, n4, ok, -4, None) == hip.EQH_ERR_ARG
    assert L.eqh_add_many(1, one, one, n4, ok + 4, 4, None) == hip.EQH_ERR_ARG      # not 16-byte aligned
    assert L.eqh_add_many(1, None, one, n4, None, 0, None) == hip.EQH_ERR_ARG
    assert L.eqh_add_many(1, one, one, (ctypes.c_int64 * 1)(-1), None, 0, None) == hip.EQH_ERR_ARG
    assert L.eqh_add_many(1, one, (ctypes.c_void_p * 1)(None), n4, None, 0, None) == hip.EQH_ERR_ARG
    assert L.eqh_add_many(0, None, None, None, None, 0, None) == hip.EQH_OK         # nothing to add or clear: no launch
    assert L.eqh_add_many(1, one, one, (ctypes.c_int64 * 1)(0), None, 0, None) == hip.EQH_OK
