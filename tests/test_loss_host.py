"""The training losses beside the MSE, host side (no GPU): the one parametrised form behind "l1", "smooth_l1" and "huber"
(csrc/loss_family.h, ops.loss_spec) against torch's three functions and their autograd gradients in float64,
``ops.loss_spec``'s mapping and errors, ``TrainStep(loss=..)`` against a hand-written ``F.<loss>`` / Adam loop,
``Fitter(loss=..)``, and the argument checks of the five native entries, which return before anything is launched."""
import ctypes
import math
import types

import pytest
import torch

from equihgnn_amd.trainer import TrainStep
from test_grad_clip_host import BASE_KEYS, _data, _Net

F = torch.nn.functional


def family(d, beta, scale):
    """(term, slope) of the family, stated in the input's precision: the branch is a select, so beta = 0 never divides"""
    a = d.abs()
    quad = a < beta
    safe = beta if beta > 0 else 1.0
    term = scale * torch.where(quad, 0.5 * d * d / safe, a - 0.5 * beta)
    slope = scale * torch.where(quad, d / safe, torch.sign(d))
    return term, slope


def _grid(beta):
    eps = 2.0 ** -20
    pts = [0.0, 1e-300, -1e-300, 1e-9, -1e-9, 0.1, -0.1, 0.75, -0.75, 1.5, -1.5, 7.0, -7.0, 1e3, -1e3, 1e12, -1e12]
    for s in (1.0, -1.0):
        pts += [s * beta, s * beta * (1 + eps), s * beta * (1 - eps), s * 0.5 * beta, s * 3.0 * beta]
    return torch.tensor(pts, dtype=torch.float64)


def _close(a, b):
    return bool(((a - b).abs() <= 1e-15 * b.abs()).all())


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0, 2.0])
def test_family_is_torchs_three_losses_in_float64(beta):
    """term / slope against F.l1_loss, F.smooth_l1_loss and F.huber_loss (reduction none) and their autograd gradients, to 1e-15
    relative, on a grid with 0, +-beta, +-beta (1 +- 2^-20) and values far on both sides"""
    d = _grid(beta)
    assert bool((d == 0).any()) and bool((d == beta).any()) and bool((d == -beta).any())
    pred, target = d.clone().requires_grad_(True), torch.zeros_like(d)

    def check(fn, b, scale):
        out = fn(pred, target)
        (g,) = torch.autograd.grad(out.sum(), pred)
        term, slope = family(d, b, scale)
        assert _close(term, out.detach()), (fn, b, scale)
        assert _close(slope, g), (fn, b, scale)
        assert bool(torch.isfinite(term).all()) and bool(torch.isfinite(slope).all())

    check(lambda p, t: F.smooth_l1_loss(p, t, reduction="none", beta=beta), beta, 1.0)
    # ... and the specs of ops.loss_spec name that form: the package's loss of a spec is the mean of its terms
    from equihgnn_amd import ops
    near = d.abs() <= 1e3                 # (a mean that 1e12 does not swamp)
    for kind in ("smooth_l1",) + (("huber",) if beta > 0 else ("l1",)):
        spec = ops.loss_spec(kind, beta)
        got = ops.regression_loss(d[near], target[near], spec)
        want = family(d[near], *spec)[0].mean()
        assert abs(float(got) - float(want)) <= 1e-15 * float(want), (kind, beta)
    if beta == 0.0:
        check(lambda p, t: F.l1_loss(p, t, reduction="none"), 0.0, 1.0)
        term, slope = family(d, 0.0, 1.0)
        assert torch.equal(term, d.abs()) and torch.equal(slope, torch.sign(d))       # the quadratic branch is never selected
    else:
        check(lambda p, t: F.huber_loss(p, t, reduction="none", delta=beta), beta, beta)


def test_loss_spec_mapping_and_errors():
    from equihgnn_amd import ops
    assert ops.loss_spec("mse") is None and ops.loss_spec("mse", 7.0) is None
    assert ops.loss_spec("l1") == (0.0, 1.0) and ops.loss_spec("l1", 3.0) == (0.0, 1.0)
    assert ops.loss_spec("smooth_l1") == (1.0, 1.0) and ops.loss_spec("smooth_l1", 0.5) == (0.5, 1.0)
    assert ops.loss_spec("smooth_l1", 0.0) == (0.0, 1.0)                               # beta = 0 is l1, as in torch
    assert ops.loss_spec("huber") == (1.0, 1.0) and ops.loss_spec("huber", 2.0) == (2.0, 2.0)
    for kind in ("mae", "MSE", "", None, "smoothl1"):
        with pytest.raises(ValueError):
            ops.loss_spec(kind)
    for kind in ("smooth_l1", "huber"):
        for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError):
                ops.loss_spec(kind, bad)
    with pytest.raises(ValueError):
        ops.loss_spec("huber", 0.0)
    # regression_loss off the device is the torch function
    g = torch.Generator().manual_seed(1)
    p, t = torch.randn(40, generator=g) * 2, torch.randn(40, generator=g)
    assert torch.equal(ops.regression_loss(p, t, None), F.mse_loss(p, t))
    assert torch.equal(ops.regression_loss(p, t, ops.loss_spec("l1")), F.l1_loss(p, t))
    assert torch.equal(ops.regression_loss(p, t, ops.loss_spec("smooth_l1", 0.5)), F.smooth_l1_loss(p, t, beta=0.5))
    assert torch.equal(ops.regression_loss(p, t, ops.loss_spec("huber", 2.0)), F.huber_loss(p, t, delta=2.0))
    for bad in ((-1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            ops.regression_loss(p, t, bad)


LOSSES = {"l1": (1.0, F.l1_loss),
          "smooth_l1": (0.5, lambda p, t: F.smooth_l1_loss(p, t, beta=0.5)),
          "huber": (2.0, lambda p, t: F.huber_loss(p, t, delta=2.0))}


@pytest.mark.parametrize("kind", sorted(LOSSES))
def test_train_step_loss_equals_the_torch_loss_then_adam(kind):
    """three steps: the same losses and parameters as the hand-written loop, bit for bit; and another fit than the MSE's"""
    beta, fn = LOSSES[kind]
    batches = [_data(40 + t) for t in range(3)]
    mine, ref, mse = _Net(3), _Net(3), _Net(3)
    tr = TrainStep(mine, lr=1e-2, weight_decay=0.1, loss=kind, loss_beta=beta)
    tr_mse = TrainStep(mse, lr=1e-2, weight_decay=0.1)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=0.1)
    for data in batches:
        loss = tr.step(data)
        tr_mse.step(data)
        for p in ref.parameters():
            p.grad = None
        ref_loss = fn(ref(data), data.y)
        ref_loss.backward()
        opt.step()
        assert torch.equal(loss, ref_loss.detach())
        for (k, p), q in zip(mine.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), k
    assert not all(torch.equal(p, q) for p, q in zip(mine.parameters(), mse.parameters()))
    assert tr_mse.loss == "mse" and tr_mse.loss_spec is None


def test_trainers_check_the_loss_at_construction():
    from equihgnn_amd.trainer import GraphedTrainStep
    for cls in (TrainStep, GraphedTrainStep):
        for kw in (dict(loss="mae"), dict(loss="huber", loss_beta=0.0), dict(loss="smooth_l1", loss_beta=-1.0),
                   dict(loss="smooth_l1", loss_beta=float("nan"))):
            with pytest.raises(ValueError):
                cls(_Net(1), **kw)
        assert cls(_Net(1), loss="l1", loss_beta=-3.0).loss_spec == (0.0, 1.0)         # "l1" and "mse" ignore loss_beta
        assert cls(_Net(1)).loss_spec is None
        assert cls(_Net(1), loss="huber", loss_beta=0.5).loss_spec == (0.5, 0.5)


def test_fitter_hands_the_loss_to_the_step():
    from equihgnn_amd.fit import Fitter
    train, valid = [_data(60 + t) for t in range(4)], [_data(70)]
    seen_kw = []

    def old_factory(model, lr, weight_decay):
        seen_kw.append((lr, weight_decay))
        return TrainStep(model, lr=lr, weight_decay=weight_decay)

    def new_factory(model, **kw):
        seen_kw.append(kw)
        return TrainStep(model, **kw)
    # "mse": the keywords are not handed on, so a factory without them keeps working
    res = Fitter(_Net(4), lr=1e-2, step_factory=old_factory).fit(train, valid, epochs=1)
    Fitter(_Net(4), lr=1e-2, step_factory=old_factory, loss="mse", loss_beta=3.0)
    assert seen_kw == [(1e-2, 0.0)] * 2 and [list(row) for row in res.history] == [BASE_KEYS]
    fitter = Fitter(_Net(4), lr=1e-2, step_factory=new_factory, loss="l1")
    assert seen_kw[-1] == dict(lr=1e-2, weight_decay=0.0, loss="l1", loss_beta=1.0)
    assert fitter.step.loss == "l1" and fitter.step.loss_spec == (0.0, 1.0)
    res_l1 = fitter.fit(train, valid, epochs=1)
    assert [list(row) for row in res_l1.history] == [BASE_KEYS]
    # train_loss is the mean of the steps' L1 values: the hand-written loop's
    ref = _Net(4)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    tot = 0.0
    for data in train:
        for p in ref.parameters():
            p.grad = None
        loss = F.l1_loss(ref(data), data.y)
        loss.backward()
        opt.step()
        tot += float(loss.detach())
    assert math.isclose(res_l1.history[0]["train_loss"], tot / len(train), rel_tol=1e-12)
    assert res_l1.history[0]["train_loss"] != res.history[0]["train_loss"]
    with pytest.raises(ValueError):
        Fitter(_Net(4), loss="huber", loss_beta=0.0)
    with pytest.raises(ValueError):
        Fitter(_Net(4), loss="mae")


BAD = ((-0.5, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, float("nan")), (1.0, float("inf")))


def test_native_entries_validate_before_launching():
    """eqh_smooth_l1_fwd_bwd and the four hg_readout*_sl1_* entries: EQH_ERR_ARG for a null pointer, beta < 0, scale <= 0 and a
    beta or scale that is not finite, ahead of any launch (no GPU here)"""
    from equihgnn_amd import hip

    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    held = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    s = [ctypes.addressof(held) + 8 * i for i in range(4)]
    # --- the lone launch
    for beta, scale in BAD:
        assert L.eqh_smooth_l1_fwd_bwd(a, a, 4, beta, scale, a, a, None) == hip.EQH_ERR_ARG, (beta, scale)
    for i in range(4):
        ptrs = [a, a, a, a]
        ptrs[i] = None
        assert L.eqh_smooth_l1_fwd_bwd(ptrs[0], ptrs[1], 4, 0.5, 1.0, ptrs[2], ptrs[3], None) == hip.EQH_ERR_ARG, i
    for n in (0, -1, 65537):
        assert L.eqh_smooth_l1_fwd_bwd(a, a, n, 0.5, 1.0, a, a, None) == hip.EQH_ERR_ARG, n

    # --- the heads: the checks of their MSE twins, and the two floats first
    def single(beta, scale, n_graphs=0, n_real=0, C=64, H=64):
        return L.hg_readout_sl1_f32(None, None, n_graphs, n_real, C, H, None, 1e-5, None, None, None, None, None, 0, None, 0,
                                    None, beta, scale, None)

    def single_drop(beta, scale, p_x=0.3, p_h=0.1, seeds=(s[0], s[2], s[3]), n_graphs=0, n_real=0, C=64, H=64):
        return L.hg_readout_sl1_drop_f32(None, None, n_graphs, n_real, C, H, None, 1e-5, None, None, None, None, None, 0, None,
                                         0, None, p_x, p_h, *seeds, beta, scale, None)

    def pair(beta, scale, n_graphs=0, n_real=0, C=64, H=128):
        return L.hg_readout_pair_sl1_f32(None, None, None, None, None, None, 0, n_graphs, n_real, C, H, None, 1e-5, None, None,
                                         None, None, None, None, 0, None, 0, None, beta, scale, None)

    def pair_drop(beta, scale, p_x=0.3, p_h=0.1, seeds=tuple(s), n_graphs=0, n_real=0, C=64, H=128):
        return L.hg_readout_pair_sl1_drop_f32(None, None, None, None, None, None, 0, n_graphs, n_real, C, H, None, 1e-5, None,
                                              None, None, None, None, None, 0, None, 0, None, p_x, p_h, *seeds, beta, scale, None)

    for entry in (single, single_drop, pair, pair_drop):
        assert entry(0.0, 1.0) == hip.EQH_OK and entry(2.0, 2.0) == hip.EQH_OK           # n_graphs = 0: nothing to do
        for beta, scale in BAD:
            assert entry(beta, scale) == hip.EQH_ERR_ARG, (entry.__name__, beta, scale)
            assert entry(beta, scale, n_graphs=4, n_real=4) == hip.EQH_ERR_ARG
        assert entry(0.5, 1.0, n_graphs=4, n_real=4) == hip.EQH_ERR_ARG                  # null pointers
        assert entry(0.5, 1.0, n_graphs=4, n_real=5) == hip.EQH_ERR_ARG                  # n_real > n_graphs
        assert entry(0.5, 1.0, C=96) == hip.EQH_ERR_ARG                                  # unsupported (C, H)
    for entry in (single_drop, pair_drop):
        assert entry(0.5, 1.0, p_x=0.0, p_h=0.0) == hip.EQH_ERR_ARG                      # no active site
        assert entry(0.5, 1.0, p_x=1.0) == hip.EQH_ERR_ARG
    assert single_drop(0.5, 1.0, seeds=(None, s[2], s[3])) == hip.EQH_ERR_ARG            # an active site without its seed
    assert pair_drop(0.5, 1.0, seeds=(s[0], None, s[2], s[3])) == hip.EQH_ERR_ARG
    # everything present but the target's partner: a training call without its loss pointer
    w = (ctypes.c_void_p * 10)(*[a] * 10)
    rc = L.hg_readout_sl1_f32(a, a, 1, 1, 64, 64, w, 1e-5, a, a, None, a, w, 0, a, 1 << 20, a, 0.5, 1.0, None)
    assert rc == hip.EQH_ERR_ARG
    rc = L.hg_readout_pair_sl1_f32(a, a, None, None, None, None, 0, 1, 1, 64, 128, w, 1e-5, a, a, None, a, None, w, 0, a, 1 << 20,
                                   a, 0.5, 1.0, None)
    assert rc == hip.EQH_ERR_ARG


def test_head_tuple_without_a_spec_is_the_mse():
    from equihgnn_amd.layers import head_loss, head_spec
    g = torch.Generator().manual_seed(2)
    out, y = torch.randn(6, generator=g), torch.randn(6, generator=g)
    assert head_spec((y, 4)) is None and head_spec((y, 4, True)) is None and head_spec((y, 4, True, None)) is None
    assert head_spec((y, 4, True, (0.5, 1.0))) == (0.5, 1.0)
    assert torch.equal(head_loss(out, (y, 4)), F.mse_loss(out[:4], y[:4]))
    assert torch.equal(head_loss(out, (y, 4, False, (0.0, 1.0))), F.l1_loss(out[:4], y[:4]))
    assert torch.equal(head_loss(out, (y, None, False, (2.0, 2.0))), F.huber_loss(out, y, delta=2.0))
