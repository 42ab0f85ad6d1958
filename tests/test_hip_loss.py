"""The L1 / smooth-L1 / Huber training losses on the device (csrc/loss_family.h): the lone launch k_smooth_l1
(eqh_smooth_l1_fwd_bwd, ops.regression_loss), the SL1 forms of the two one-launch read-out heads (hg_readout_sl1_* and
hg_readout_pair_sl1_*; ops.readout_mse / readout_pair_mse with ``loss=``) against the float64 heads of
tests/test_hip_readout_dropout.py and tests/test_hip_paired_readout.py with their masks made explicit, the models with the fused
path on and off, and GraphedTrainStep(loss=..).

Head cases.  The targets are constructed, not drawn: y_b = out64_b - r_b with out64 the float64 predictions and r_b cycling
through {+0.25 b', -0.5 b', +(2 b' + 0.3), -(3 b' + 0.1)}, b' = max(beta, 1), so every real molecule's residual keeps 0.25 from 0
and from +-beta (asserted on the float64 residuals; the fp32 rounding of y_b moves them by < 1e-6), both branches occur and for
L1 both signs.  The kinds are l1, smooth_l1(beta = 1) and huber(delta = 2): with b' = max(beta, 1) the cycle's -0.5 b' would sit
exactly on -beta for beta = 0.5, so the heads take smooth_l1 at beta = 1 (the lone kernel, which is tested AT |d| = beta,
takes beta = 0.5).

Limits: ``_limits`` of the two files named above, unchanged.  dy is +-scale / n_real or d scale / (beta n_real), no larger in
magnitude or rounding than the MSE's 2 d / n_real at these residuals."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, golden_args, make_batch  # noqa: E402
import test_hip_paired_readout as tp  # noqa: E402
import test_hip_readout_dropout as ts  # noqa: E402
from test_loss_host import family  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional
KINDS = [("l1", 1.0), ("smooth_l1", 0.5), ("huber", 2.0)]               # the lone kernel's
HEAD_KINDS = [("l1", 1.0), ("smooth_l1", 1.0), ("huber", 2.0)]           # the heads' (see the module docstring)
PROBS = [(0.0, 0.0), (0.1, 0.1)]


def _ops():
    from equihgnn_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# the lone kernel
# ---------------------------------------------------------------------------------------------------------------------
def _lone_inputs(n, beta):
    """pred and target on the grid of multiples of 2^-10 below 8, so pred - target is exact in fp32 and in float64 alike: the
    residuals start 0, +beta, -beta, a quarter of beta, 3 beta + 1, then grid values in [-4, 4]"""
    g = torch.Generator().manual_seed(n)
    pred = torch.randint(-4096, 4096, (n,), generator=g).float() / 1024.0
    r = torch.randint(-4096, 4096, (n,), generator=g).float() / 1024.0
    head = torch.tensor([0.0, beta, -beta, 0.25 * beta, 3.0 * beta + 1.0])[:n]
    r[:head.shape[0]] = head
    target = pred - r
    assert torch.equal(pred - target, r) and torch.equal(pred.double() - target.double(), r.double())
    return pred, target, r


@pytest.mark.parametrize("kind,beta", KINDS)
@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 65536])
def test_lone_kernel_matches_float64(n, kind, beta):
    """one element, below / at / above the 1024-thread stride and the cap; d == 0 and |d| == beta occur exactly.  Gradient:
    exact where the family gives +-scale / n or 0, 1e-6 relative in the quadratic branch; loss to 1e-6 max(1, loss); two runs are
    the same bits."""
    ops = _ops()
    spec = ops.loss_spec(kind, beta)
    b, scale = spec
    pred, target, r = _lone_inputs(n, b)
    assert float(r[0]) == 0.0 and (n < 5 or (abs(float(r[1])) == b and abs(float(r[2])) == b))
    term, slope = family(r.double(), b, scale)
    want_loss = float(term.mean())
    quad = r.abs() < b
    unit = torch.tensor(scale, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)     # fp32 scale / n

    def run():
        p = pred.to(DEV).requires_grad_(True)
        loss = ops.regression_loss(p, target.to(DEV), spec)
        loss.backward()
        return loss.detach().cpu(), p.grad.cpu()

    loss, grad = run()
    again = run()
    assert torch.equal(loss, again[0]) and torch.equal(grad, again[1])
    print(f"n={n} {kind}({beta}): loss {float(loss):.8g} vs {want_loss:.8g}, quadratic elements {int(quad.sum())}")
    assert abs(float(loss) - want_loss) <= 1e-6 * max(1.0, want_loss)
    lin = ~quad
    assert torch.equal(grad[lin], torch.sign(r[lin]) * unit)                # +-scale / n, and exactly 0 at d == 0
    if bool(quad.any()):
        want = (slope[quad] / n)
        assert float(((grad[quad].double() - want).abs() - 1e-6 * want.abs()).max()) <= 0.0
    assert float(grad[0]) == 0.0
    # the conditions of the one launch are mse_loss's: anything else goes through torch
    if n == 5:
        p64 = pred.double().to(DEV)
        assert ops.regression_loss(p64, target.double().to(DEV), spec).dtype == torch.float64
        assert torch.equal(ops.regression_loss(pred.to(DEV), target.to(DEV), None), ops.mse_loss(pred.to(DEV), target.to(DEV)))


# ---------------------------------------------------------------------------------------------------------------------
# the two heads against float64
# ---------------------------------------------------------------------------------------------------------------------
def _targets(out64, n_real, beta):
    """y (fp32, [B]) with the constructed residuals, and the asserted margins of the float64 residuals"""
    bp = max(beta, 1.0)
    cycle = torch.tensor([0.25 * bp, -0.5 * bp, 2.0 * bp + 0.3, -(3.0 * bp + 0.1)], dtype=torch.double)
    r = cycle[torch.arange(out64.shape[0]) % 4]
    y = (out64 - r).float()
    y[n_real:] = 0.0
    d = (out64 - y.double())[:n_real]
    margin = float(torch.minimum(d.abs(), (d.abs() - beta).abs()).min())
    assert margin >= 0.25 - 1e-6, margin
    if n_real >= 4:
        assert bool((d.abs() < beta).any()) == (beta > 0) and bool((d.abs() > beta).any())
        assert bool((d > 0).any()) and bool((d < 0).any())
    return y


def _family_loss(out, y, n_real, spec):
    term, _ = family(out[:n_real] - y[:n_real].double(), spec[0], spec[1])
    return term.mean()


_SINGLE = {}


def _single_case(C, H, B, n_real, p_x, p_h):
    key = (C, H, B, n_real, p_x, p_h)
    if key not in _SINGLE:
        _SINGLE[key] = ts._case(C, H, B, n_real, p_x, p_h)
    return _SINGLE[key]


def _check_head(tag, lim, run, ref_grads, ref_loss, out64, n_real, row_names):
    """What both head tests assert of one case.  ``run(unit_grad)`` -> (loss, pred, row gradients, mlp); ``ref_grads``: the float64
    gradients of the rows, then of the ten parameters."""
    ops = _ops()
    loss, pred, rows, mlp = run(False, 3.0)
    perr = float(((pred[:n_real].cpu().double() - out64[:n_real]).abs() - lim["pred_rtol"] * out64[:n_real].abs()).max())
    errs = {n: tp._rel(g / 3.0, r) for n, g, r in zip(row_names, rows, ref_grads)}
    for (n, q), r in zip(mlp.named_parameters(), ref_grads[len(rows):]):
        errs[n] = tp._rel(q.grad / 3.0, r)
    print(f"{tag}: predictions {perr:.2e} (limit {lim['pred_atol']:.2e}), loss {abs(float(loss) - ref_loss):.2e}, "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (limits rows {lim['dx']:.2e}, parameters {lim['param']:.2e})")
    assert perr <= lim["pred_atol"]
    assert abs(float(loss) - ref_loss) < lim["loss"] * max(1.0, ref_loss)
    for n in row_names:
        assert errs[n] < lim["dx"], (n, errs[n])
    for n, _ in mlp.named_parameters():
        assert errs[n] < lim["param"], (n, errs[n])
    # trainer mode: unit incoming gradient, parameter gradients ADDED to persistent accumulators, eagerly and deferred
    for deferred in (False, True):
        for q in mlp.parameters():
            q.grad = None
            q._eqh_gbuf = torch.full_like(q, 0.5)
        if deferred:
            ops.defer_begin(DEV)
        loss2, _, rows2, _ = run(True, 1.0)
        if deferred:
            ops.defer_flush(DEV)
        assert float(loss2) == float(loss)
        for g2, g, r in zip(rows2, rows, ref_grads):
            assert torch.equal(g2, g / 3.0) or tp._rel(g2, r) < lim["dx"]
        for (n, q), r in zip(mlp.named_parameters(), ref_grads[len(rows):]):
            assert q.grad is None, n
            assert tp._rel(q._eqh_gbuf - 0.5, r) < lim["param"], (n, deferred)
        for q in mlp.parameters():
            del q._eqh_gbuf
    return rows


@pytest.mark.parametrize("kind,beta", HEAD_KINDS)
@pytest.mark.parametrize("p_x,p_h", PROBS)
@pytest.mark.parametrize("C,H,B,n_real", [(64, 64, 16, 16), (128, 64, 5, 4), (256, 128, 37, 33)])
def test_single_head_matches_float64(C, H, B, n_real, p_x, p_h, kind, beta):
    """a full tile; a padded batch in one workgroup; three workgroups with a ragged last one at the widest C (the ticket across
    workgroups) -- with and without the three dropout sites, incoming gradient 3, then the trainer's accumulate mode"""
    ops = _ops()
    spec = ops.loss_spec(kind, beta)
    c = _single_case(C, H, B, n_real, p_x, p_h)
    lim = ts._limits(p_x, p_h)
    rowptr64, x = c["rowptr64"], c["x"]
    y = _targets(c["out"], n_real, spec[0])
    # float64: the same head, fresh leaves (the shared case keeps its own gradients)
    batch = torch.repeat_interleave(torch.arange(B), rowptr64[1:] - rowptr64[:-1])
    xd = x.double().requires_grad_(True)
    out, _ = ts._forward64(c["ref"], xd, batch, B, H, c["keeps"])
    assert torch.equal(out.detach(), c["out"])
    ref_loss = _family_loss(out, y, n_real, spec)
    ref_grads = torch.autograd.grad(ref_loss, [xd, *c["ref"].parameters()])
    drop = p_x > 0 or p_h > 0
    seeds = ts._device_seeds(p_x, p_h) if drop else None
    mlp = copy.deepcopy(c["mlp"]).to(DEV).train()     # (the shared case keeps its own head untouched)
    rowptr = rowptr64.int().to(DEV)

    def run(unit_grad, scale):
        if not unit_grad:
            for q in mlp.parameters():
                q.grad = None
        xg = x.to(DEV).requires_grad_(True)
        loss, pred = ops.readout_mse(xg, rowptr, mlp, y.to(DEV), n_real, unit_grad=unit_grad, p_x=p_x, seeds=seeds, loss=spec)
        (scale * loss).backward()
        return loss.detach().cpu(), pred, (xg.grad,), mlp

    (dx,) = _check_head(f"single C={C} H={H} B={B} p=({p_x}, {p_h}) {kind}({beta})", lim, run, ref_grads, float(ref_loss.detach()),
                        c["out"], n_real, ("dx",))
    # exact zeros: rows of padding molecules, dropped elements
    if n_real < B:
        assert float(dx[int(rowptr64[n_real]):].abs().max()) == 0.0
    real = slice(0, int(rowptr64[n_real]))
    assert float(dx[real].abs().max()) > 0.0
    if p_x > 0:
        assert float(dx[real][c["keeps"][0][real] == 0].abs().max()) == 0.0


@pytest.mark.parametrize("kind,beta", HEAD_KINDS)
@pytest.mark.parametrize("p_x,p_h", PROBS)
@pytest.mark.parametrize("C,H,B,n_real", [(64, 128, 5, 4), (256, 256, 37, 33)])
def test_paired_head_matches_float64(C, H, B, n_real, p_x, p_h, kind, beta):
    """one padded workgroup, and three workgroups with a partial last tile at the widest (C, H) -- with and without the four
    dropout sites, incoming gradient 3, then the trainer's accumulate mode"""
    ops = _ops()
    spec = ops.loss_spec(kind, beta)
    c = tp._case(C, H, B, n_real, p_x, p_h)          # shared with that file's tests and left as it is
    lim = tp._limits(p_x, p_h, C, H)
    x, e = c["x"], c["e"]
    y = _targets(c["out"], n_real, spec[0])
    batch = torch.repeat_interleave(torch.arange(B), c["rowptr64"][1:] - c["rowptr64"][:-1])
    xd, ed = x.double().requires_grad_(True), e.double().requires_grad_(True)
    out, _ = tp._forward64(c["ref"], xd, ed, batch, c["e_mol"], (c["order"] > 2).double(), B, H, c["keeps"])
    assert torch.equal(out.detach(), c["out"])
    ref_loss = _family_loss(out, y, n_real, spec)
    ref_grads = torch.autograd.grad(ref_loss, [xd, ed, *c["ref"].parameters()])
    drop = p_x > 0 or p_h > 0
    seeds = tp._device_seeds(p_x, p_h) if drop else None
    mlp = copy.deepcopy(c["mlp"]).to(DEV).train()     # (the shared case keeps its own head untouched)
    index, order = tp._index(c, B, null_perm=(C == 64)), c["order"].to(DEV)

    def run(unit_grad, scale):
        if not unit_grad:
            for q in mlp.parameters():
                q.grad = None
        xg, eg = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
        loss, pred = ops.readout_pair_mse(xg, eg, index, None, order, mlp, y.to(DEV), n_real, unit_grad=unit_grad, p_x=p_x,
                                          seeds=seeds, loss=spec)
        (scale * loss).backward()
        return loss.detach().cpu(), pred, (xg.grad, eg.grad), mlp

    dx, de = _check_head(f"paired C={C} H={H} B={B} p=({p_x}, {p_h}) {kind}({beta})", lim, run, ref_grads, float(ref_loss.detach()),
                         c["out"], n_real, ("dx", "de"))
    # exact zeros: rows of padding molecules, hyperedge rows of order <= 2, dropped elements
    e_mol, low = c["e_mol"], (c["order"] <= 2)
    assert bool(low.any()) and bool((~low).any())
    assert float(de[low.to(DEV)].abs().max()) == 0.0
    assert float(de[(~low & (e_mol < n_real)).to(DEV)].abs().max()) > 0.0
    if n_real < B:
        assert float(dx[int(c["rowptr64"][n_real]):].abs().max()) == 0.0
        assert float(de[(e_mol >= n_real).to(DEV)].abs().max()) == 0.0
    if p_x > 0:
        real = slice(0, int(c["rowptr64"][n_real]))
        assert float(dx[real][c["keeps"][0][real] == 0].abs().max()) == 0.0
        assert float(de.cpu()[c["keeps"][1] == 0].abs().max()) == 0.0


@pytest.mark.parametrize("head", ["single", "paired"])
def test_two_runs_of_a_head_are_bitwise_equal(head):
    """three workgroups, dropout on: the partials are summed in workgroup order by whichever workgroup arrives last"""
    ops = _ops()
    spec = ops.loss_spec("huber", 2.0)
    if head == "single":
        C, H, B, n_real = 256, 128, 37, 33
        c = _single_case(C, H, B, n_real, 0.1, 0.1)
        seeds, rowptr = ts._device_seeds(0.1, 0.1), c["rowptr64"].int().to(DEV)
    else:
        C, H, B, n_real = 256, 256, 37, 33
        c = tp._case(C, H, B, n_real, 0.1, 0.1)
        seeds, index, order = tp._device_seeds(0.1, 0.1), tp._index(c, B), c["order"].to(DEV)
    y = _targets(c["out"], n_real, spec[0]).to(DEV)
    mlp = copy.deepcopy(c["mlp"]).to(DEV).train()     # (the shared case keeps its own head untouched)

    def run():
        for q in mlp.parameters():
            q.grad = None
        x = c["x"].to(DEV).requires_grad_(True)
        if head == "single":
            loss, pred = ops.readout_mse(x, rowptr, mlp, y, n_real, p_x=0.1, seeds=seeds, loss=spec)
            rows = [x]
        else:
            e = c["e"].to(DEV).requires_grad_(True)
            loss, pred = ops.readout_pair_mse(x, e, index, None, order, mlp, y, n_real, p_x=0.1, seeds=seeds, loss=spec)
            rows = [x, e]
        loss.backward()
        return [loss.detach().clone(), pred.clone()] + [r.grad.clone() for r in rows] + [q.grad.clone() for q in mlp.parameters()]

    first, again = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and all(bool(torch.isfinite(t).all()) for t in first)


# ---------------------------------------------------------------------------------------------------------------------
# the models: fused path on and off
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("hg_readout_sl1_f32", "hg_readout_sl1_drop_f32", "hg_readout_pair_sl1_f32", "hg_readout_pair_sl1_drop_f32",
           "hg_readout_mse_f32", "hg_readout_pair_mse_f32", "eqh_smooth_l1_fwd_bwd", "eqh_mse_fwd_bwd")


def _step(m, data, head):
    for q in m.parameters():
        q.grad = None
    torch.manual_seed(21)
    loss = m(data, head=head)
    loss.backward()
    return float(loss.detach()), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}


def _same(lim, on, off, tag):
    (loss_on, g_on), (loss_off, g_off) = on, off
    print(f"{tag}: loss {loss_on} vs {loss_off}")
    assert abs(loss_on - loss_off) < lim["loss"] * max(1.0, abs(loss_off))
    assert sorted(g_on) == sorted(g_off) and len(g_off) > 5
    for n in g_off:
        err = float((g_on[n] - g_off[n]).abs().max() / g_off[n].abs().max().clamp(min=1e-9))
        print(f"{tag} {n}: {err:.2e}")
        assert err < lim["param"], (n, err)


@pytest.mark.parametrize("method", ["mhnns", "mhnn"])
def test_models_take_the_sl1_head_and_agree_with_the_separate_launches(method, monkeypatch):
    """mhnns (single head) and mhnn (paired head), 8 molecules, huber(0.5): with the fused head the sl1 entry runs exactly once
    and nothing of the MSE; with it off (the supported-queries False / ops.PAIRED_READOUT False) the tail ends in the lone
    k_smooth_l1 launch; loss and every parameter gradient agree within the limits of the MSE on / off tests."""
    ops = _ops()
    spec = ops.loss_spec("huber", 0.5)
    paired = method == "mhnn"
    lim = tp._limits(0.0, 0.0) if paired else ts._limits(0.0, 0.0)
    data = make_batch(11, 7).to(DEV)
    m = tp._model(method, 0.0).train()
    calls = tp._count(monkeypatch, *ENTRIES)
    fused = "hg_readout_pair_sl1_f32" if paired else "hg_readout_sl1_f32"
    head = (data.y.view(-1), None, False, spec)
    on = _step(m, data, head)
    assert {n: v for n, v in calls.items() if v} == {fused: 1}, dict(calls)
    for n in calls:
        calls[n] = 0
    if paired:
        monkeypatch.setattr(ops, "PAIRED_READOUT", False)
    else:
        monkeypatch.setattr(ops, "readout_mse_supported", lambda *a, **k: False)
        monkeypatch.setattr(ops, "readout_mse_drop_supported", lambda *a, **k: False)
    off = _step(m, data, head)
    assert {n: v for n, v in calls.items() if v} == {"eqh_smooth_l1_fwd_bwd": 1}, dict(calls)
    _same(lim, on, off, f"{method} huber(0.5)")
    # and the loss is another one than the MSE, which still takes its own entries
    for n in calls:
        calls[n] = 0
    mse = _step(m, data, (data.y.view(-1), None))
    assert {n: v for n, v in calls.items() if v} == {"eqh_mse_fwd_bwd": 1} and mse[0] != off[0]


def test_gin_ends_in_the_lone_launch(monkeypatch):
    """gin (no fused head): head = (y, n, False, spec) ends in one k_smooth_l1 launch; loss and gradients against
    F.huber_loss on the model's predictions.  Limits: the loss and parameter limits of the heads' on / off tests (1e-5, 5e-5) --
    the two runs differ in the last operator only, whose gradient is +-delta / n or d / n in fp32 either way."""
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import synth_graph_batch
    ops = _ops()
    spec = ops.loss_spec("huber", 0.5)
    lim = ts._limits(0.0, 0.0)
    data = synth_graph_batch(8, 700, "pcqm").to(DEV)
    m = GNN_2D(1, num_layer=2, emb_dim=64, gnn_type="gin", drop_ratio=0.0)
    fill_state_dict(m, 5)
    m = m.to(DEV).train()
    calls = tp._count(monkeypatch, "eqh_smooth_l1_fwd_bwd", "eqh_mse_fwd_bwd")
    y = data.y.view(-1)
    on = _step(m, data, (y, None, False, spec))
    assert dict(calls) == {"eqh_smooth_l1_fwd_bwd": 1, "eqh_mse_fwd_bwd": 0}
    for q in m.parameters():
        q.grad = None
    loss = F.huber_loss(m(data), y, delta=0.5)
    loss.backward()
    off = (float(loss.detach()), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})
    assert dict(calls) == {"eqh_smooth_l1_fwd_bwd": 1, "eqh_mse_fwd_bwd": 0}
    _same(lim, on, off, "gin huber(0.5)")


# ---------------------------------------------------------------------------------------------------------------------
# graphed training
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_training_on_l1(monkeypatch):
    """GraphedTrainStep(loss="l1") on mhnns, a padded batch: the eager step, the capture and three replays with the fused head
    against the same trainer with the head as separate launches, within the limits of
    tests/test_hip_paired_readout.py::test_one_graphed_training_step (lr 0: every step is the same step); the sl1 entry is
    the only loss entry the eager step and the captures call.  A GraphedTrainStep() built in the same process -- before and after the L1
    trainers -- trains on the MSE: the MSE head's entry alone, the same losses bit for bit both times, another number than L1."""
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    ops = _ops()
    lim = ts._limits(0.0, 0.0)
    m_on = tp._model("mhnns", 0.0).train()
    m_off, m_mse0, m_mse1 = copy.deepcopy(m_on), copy.deepcopy(m_on), copy.deepcopy(m_on)
    raw = synth_batch(8, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 8
    assert batch.y.shape[0] > 8                       # padded: n_real < B
    calls = tp._count(monkeypatch, "hg_readout_sl1_f32", "hg_readout_mse_f32", "eqh_smooth_l1_fwd_bwd", "eqh_mse_fwd_bwd")

    def train(model, steps, **kw):
        batch._hyper_index = None
        for n in calls:
            calls[n] = 0
        tr = GraphedTrainStep(model, lr=0.0, keep_grads=True, **kw)
        tr.index_prefetch = False
        losses = [float(tr.step(batch)) for _ in range(steps)]      # eager, capture, replays
        torch.cuda.synchronize()
        assert len(tr.slots) == 1 and all(np.isfinite(losses)), losses
        assert len(set(losses[2:])) == 1, losses
        grads = {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}
        tr.close()
        used = {n: v for n, v in calls.items() if v}
        assert len(used) == 1 and sum(used.values()) >= 2, used     # one entry alone: the eager step and the capture(s)
        return losses, grads, list(used)[0]

    mse_before = train(m_mse0, 4)
    assert mse_before[2] == "hg_readout_mse_f32"
    l_on, g_on, entry = train(m_on, 5, loss="l1")
    assert entry == "hg_readout_sl1_f32"
    supported = (ops.readout_mse_supported, ops.readout_mse_drop_supported)
    monkeypatch.setattr(ops, "readout_mse_supported", lambda *a, **k: False)
    monkeypatch.setattr(ops, "readout_mse_drop_supported", lambda *a, **k: False)
    l_off, g_off, entry = train(m_off, 5, loss="l1")
    assert entry == "eqh_smooth_l1_fwd_bwd"
    monkeypatch.setattr(ops, "readout_mse_supported", supported[0])
    monkeypatch.setattr(ops, "readout_mse_drop_supported", supported[1])
    print("graphed mhnns l1, fused head on / off:", l_on, l_off)
    for a, b in zip(l_on, l_off):
        assert abs(a - b) < lim["loss"] * max(1.0, abs(b)), (l_on, l_off)
    assert sorted(g_on) == sorted(g_off) and len(g_off) > 10
    for n in g_off:
        assert bool(torch.isfinite(g_on[n]).all()), n
        err = float((g_on[n] - g_off[n]).abs().max() / g_off[n].abs().max().clamp(min=1e-9))
        assert err < lim["param"], (n, err)
    # --- the default trainer is the MSE trainer it was
    mse_after = train(m_mse1, 4)
    assert mse_after[2] == "hg_readout_mse_f32" and mse_after[0] == mse_before[0], (mse_before[0], mse_after[0])
    assert all(torch.equal(mse_after[1][n], g) for n, g in mse_before[1].items())
    assert mse_after[0][0] != l_on[0]
