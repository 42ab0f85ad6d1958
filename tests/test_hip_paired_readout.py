"""The paired tail's read-out head as one launch (k_readout_pair_mse, hg_readout_pair_mse_f32 / _drop_f32; csrc/readout_pair.hip,
ops.readout_pair_mse, models._PairedBase): the operator against float64 autograd with the four dropout masks made explicit,
its bitwise repeatability, the models with the switch on against the separate launches under one seed pool, and one graphed
training step.

The keep matrix of a site is what ``ops.dropout_add(ones[R, C], None, p, seed)`` returns; it is also computed on the host by the
numpy twin of csrc/drop_hash.h in tests/test_readout_dropout_host.py, and the two are asserted equal, so a case (a seed whose
float64 pre-activations keep 2e-5 from the ReLU kink WITH the masks applied) is chosen without the device.

Tolerances (``_limits``): those of tests/test_hip_kernels.py::test_readout_mse_matches_float64_reference -- 2e-5 abs + 1e-5 rel on
the predictions, 1e-5 on the loss, 3e-5 on dX and dE, 5e-5 on the parameter gradients, each relative to the reference's max --
times s = 1 / ((1 - p_x) (1 - p_h)^2) for the masks on the path, as tests/test_hip_readout_dropout.py::_limits does, and times
2 where 2C > 256 or H > 128: the longest dot product doubles from 256 to 512 terms and worst-case rounding grows linearly in its
length."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, golden_args, make_batch  # noqa: E402
from test_readout_dropout_host import keep_matrix  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional
SHAPES = [(64, 128, 5, 4),
          (128, 128, 17, 17),       # the second workgroup holds one molecule; the hyperedge pool has a non-identity perm
          (256, 256, 37, 33),       # partial last tile plus padding molecules
          (128, 256, 11, 10)]       # molecules of up to 150 atoms and 40 hyperedges: several pooling rounds
PROBS = [(0.0, 0.0), (0.0, 0.1), (0.1, 0.1), (0.5, 0.3)]
SEEDS = (0x1234567, 0x7654321FF, 0x89ABCDEF01, 0x3C3C3C3C3C3C)        # pre-pool x, pre-pool e, hidden 1, hidden 2


def _ops():
    from equihgnn_amd import ops
    return ops


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _limits(p_x, p_h, C=64, H=128):
    s = (2.0 if (2 * C > 256 or H > 128) else 1.0) / ((1.0 - p_x) * (1.0 - p_h) ** 2)
    return dict(pred_atol=2e-5 * s, pred_rtol=1e-5 * s, loss=1e-5 * s, dx=3e-5 * s, param=5e-5 * s)


def _rel(a, b):
    b = b.detach().cpu().double()
    return float((a.detach().cpu().double() - b).abs().max() / b.abs().max().clamp(min=1e-9))


def _head(C, H, p_h, seed):
    from equihgnn_amd.layers import MLP
    torch.manual_seed(seed)
    mlp = MLP(2 * C, H, 1, 3, dropout=p_h, Normalization="ln", InputNorm=False)
    g = torch.Generator().manual_seed(seed + 1)
    for q in mlp.parameters():
        q.data.add_(0.1 * torch.randn(q.shape, generator=g))
    return mlp


def _forward64(ref, xd, ed, batch, e_mol, high, B, H, keeps):
    """the head in float64 with the four masks as tensors: (predictions, smallest |pre-activation|)"""
    kx, ke, k1, k2 = keeps
    C = xd.shape[1]
    px = torch.zeros(B, C, dtype=torch.double).index_add_(0, batch, xd * kx)
    pe = torch.zeros(B, C, dtype=torch.double).index_add_(0, e_mol, ed * ke * high.unsqueeze(-1))
    h, margin = torch.cat((px, pe), -1), float("inf")
    for i, k in enumerate((k1, k2)):
        pre = ref.lins[i](h)
        margin = min(margin, float(pre.detach().abs().min()))
        h = F.layer_norm(torch.relu(pre), (H,), ref.normalizations[i + 1].weight, ref.normalizations[i + 1].bias, 1e-5) * k
    return ref.lins[2](h).view(-1), margin


_CASES = {}


def _case(C, H, B, n_real, p_x, p_h):
    """The first seed (of at most 200) whose float64 pre-activations, masks applied, all keep 2e-5 from the ReLU kink: host only,
    the masks are the numpy twin's.  Every case has a molecule without atoms, one without a hyperedge of order > 2 (and one
    without any hyperedge), and hyperedge rows of order <= 2 between higher ones; the 17-molecule case stores its hyperedges
    in a scrambled order, so its pool's perm is not the identity.  Built once per parameter set and left unchanged."""
    key = (C, H, B, n_real, p_x, p_h)
    if key in _CASES:
        return _CASES[key]
    from equihgnn_amd.layers import MLP
    big = B == 11
    margin = 0.0
    for seed in range(C + H + B, C + H + B + 200):
        g = torch.Generator().manual_seed(seed)
        sizes = torch.randint(1, 150 if big else 30, (B,), generator=g)
        sizes[min(2, B - 1)] = 0                                # a molecule without atoms
        n_he = torch.randint(1, 40 if big else 12, (B,), generator=g)
        n_he[min(3, B - 1)] = 0                                 # a molecule without any hyperedge
        rowptr64 = torch.cat((torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)))
        N, M = int(sizes.sum()), int(n_he.sum())
        batch = torch.repeat_interleave(torch.arange(B), sizes)
        e_mol = torch.repeat_interleave(torch.arange(B), n_he)
        order = torch.tensor([2, 2, 3, 2, 5, 4], dtype=torch.int64)[torch.randint(0, 6, (M,), generator=g)]
        order[e_mol == 1] = 2                                   # a molecule with no hyperedge of order > 2
        order[e_mol == 0] = torch.tensor([2, 3, 2, 4, 1, 3] * 10)[:int(n_he[0])]     # interleaved on purpose
        if B == 17:                                             # hyperedges not stored molecule by molecule
            shuffle = torch.randperm(M, generator=g)
            e_mol, order = e_mol[shuffle], order[shuffle]
        perm = torch.sort(e_mol, stable=True).indices
        e_rowptr64 = torch.cat((torch.zeros(1, dtype=torch.int64), torch.bincount(e_mol, minlength=B).cumsum(0)))
        x, e = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
        y = torch.randn(B, generator=g)
        mlp = _head(C, H, p_h, B)
        ref = MLP(2 * C, H, 1, 3, dropout=0.0, Normalization="ln", InputNorm=False).double()
        ref.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
        keeps = (torch.from_numpy(keep_matrix(N, C, p_x, SEEDS[0])).double(),
                 torch.from_numpy(keep_matrix(M, C, p_x, SEEDS[1])).double(),
                 torch.from_numpy(keep_matrix(B, H, p_h, SEEDS[2])).double(),
                 torch.from_numpy(keep_matrix(B, H, p_h, SEEDS[3])).double())
        xd, ed = x.double().requires_grad_(True), e.double().requires_grad_(True)
        out, margin = _forward64(ref, xd, ed, batch, e_mol, (order > 2).double(), B, H, keeps)
        if margin >= 2e-5:
            break
    assert margin >= 2e-5, "no seed of 200 keeps the pre-activations off the ReLU kink"
    loss_ref = ((out[:n_real] - y[:n_real].double()) ** 2).mean()
    loss_ref.backward()
    assert bool((order[e_mol == 1] <= 2).all()) and int((e_mol == min(3, B - 1)).sum()) == 0 and int(sizes[min(2, B - 1)]) == 0
    assert (B == 17) != bool(torch.equal(perm, torch.arange(M)))
    c = dict(rowptr64=rowptr64, e_rowptr64=e_rowptr64, perm=perm, e_mol=e_mol, order=order, N=N, M=M, x=x, e=e, y=y, mlp=mlp,
             ref=ref, xd=xd, ed=ed, out=out.detach(), loss=float(loss_ref.detach()), keeps=keeps)
    _CASES[key] = c
    return c


def _index(c, B, null_perm=False):
    """what ops.readout_pair_mse asks of a HyperIndex: the atom pool's rowptr, N and the hyperedge pool"""
    he = SimpleNamespace(rowptr=c["e_rowptr64"].int().to(DEV), perm=None if null_perm else c["perm"].int().to(DEV), n_rows=B)
    return SimpleNamespace(pool=SimpleNamespace(rowptr=c["rowptr64"].int().to(DEV), n_rows=B), N=c["N"],
                           hyperedge_pool=lambda n_e: (he, c["e_mol"].int().to(DEV)))


def _device_seeds(p_x, p_h):
    return (_seed(SEEDS[0]) if p_x > 0 else None, _seed(SEEDS[1]) if p_x > 0 else None,
            _seed(SEEDS[2]) if p_h > 0 else None, _seed(SEEDS[3]) if p_h > 0 else None)


@pytest.mark.parametrize("p_x,p_h", PROBS)
@pytest.mark.parametrize("C,H,B,n_real", SHAPES)
def test_readout_pair_mse_matches_float64_with_explicit_masks(C, H, B, n_real, p_x, p_h):
    """[node pool | order > 2 hyperedge pool] -> MLP(2C, H, H, 1; LN after ReLU, dropout behind the LN) -> MSE over the first
    n_real molecules with the four dropout sites inside the one launch, against the same head in float64 autograd times the keep
    matrices; the incoming gradient is 3; then the accumulate-in-place mode the trainer uses, eagerly and with the reductions
    deferred."""
    ops = _ops()
    c = _case(C, H, B, n_real, p_x, p_h)
    lim = _limits(p_x, p_h, C, H)
    N, M, x, e, y = c["N"], c["M"], c["x"], c["e"], c["y"]
    seeds = _device_seeds(p_x, p_h)
    # the masks the expectation was built from are the device's
    sites = ((N, C, p_x, seeds[0]), (M, C, p_x, seeds[1]), (B, H, p_h, seeds[2]), (B, H, p_h, seeds[3]))
    for (rows, cols, p, s), k in zip(sites, c["keeps"]):
        if p > 0:
            got = ops.dropout_add(torch.ones(rows, cols, device=DEV), None, p, s).cpu()
            assert torch.equal(got, k.float()), "the numpy twin of drop_hash.h disagrees with the device"
            assert 0.0 < float((got == 0).float().mean()) < 1.0
    mlp = c["mlp"].to(DEV).train()
    xg, eg = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    index = _index(c, B, null_perm=(C == 64))          # hyperedges stored molecule by molecule: a null perm is the identity
    order = c["order"].to(DEV)
    if p_x > 0 or p_h > 0:
        assert ops.readout_pair_mse_drop_supported(xg, eg, mlp, p_x) and not ops.readout_pair_mse_supported(xg, eg, mlp)
    else:
        assert ops.readout_pair_mse_supported(xg, eg, mlp) and not ops.readout_pair_mse_drop_supported(xg, eg, mlp, p_x)
    kw = dict(p_x=p_x, seeds=seeds if (p_x > 0 or p_h > 0) else None)
    loss, pred = ops.readout_pair_mse(xg, eg, index, None, order, mlp, y.to(DEV), n_real, **kw)
    (3.0 * loss).backward()                                # a non-unit incoming gradient scales everything
    out = c["out"]
    perr = float(((pred[:n_real].cpu().double() - out[:n_real]).abs() - lim["pred_rtol"] * out[:n_real].abs()).max())
    errs = {"dx": _rel(xg.grad / 3.0, c["xd"].grad), "de": _rel(eg.grad / 3.0, c["ed"].grad)}
    for (n, q), qr in zip(mlp.named_parameters(), c["ref"].parameters()):
        errs[n] = _rel(q.grad / 3.0, qr.grad)
    print(f"C={C} H={H} B={B} p=({p_x}, {p_h}): predictions {perr:.2e} (limit {lim['pred_atol']:.2e}), loss "
          f"{abs(float(loss.detach()) - c['loss']):.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" (limits dx/de {lim['dx']:.2e}, parameters {lim['param']:.2e})")
    assert perr <= lim["pred_atol"]
    assert abs(float(loss.detach()) - c["loss"]) < lim["loss"] * max(1.0, c["loss"])
    assert errs["dx"] < lim["dx"] and errs["de"] < lim["dx"]
    assert mlp.lins[0].weight.grad.shape == (H, 2 * C)
    for n, _ in mlp.named_parameters():
        assert errs[n] < lim["param"], (n, errs[n])
    # exact zeros: rows of padding molecules, hyperedge rows of order <= 2, dropped elements
    e_mol, low = c["e_mol"], (c["order"] <= 2)
    assert bool(low.any()) and bool((~low).any())
    assert float(eg.grad[low.to(DEV)].abs().max()) == 0.0
    assert float(eg.grad[(~low & (e_mol < n_real)).to(DEV)].abs().max()) > 0.0
    if n_real < B:
        assert float(xg.grad[int(c["rowptr64"][n_real]):].abs().max()) == 0.0
        assert float(eg.grad[(e_mol >= n_real).to(DEV)].abs().max()) == 0.0
    if p_x > 0:
        real = slice(0, int(c["rowptr64"][n_real]))
        assert float(xg.grad[real][c["keeps"][0][real] == 0].abs().max()) == 0.0
        assert float(eg.grad.cpu()[c["keeps"][1] == 0].abs().max()) == 0.0
    # trainer mode: unit incoming gradient, parameter gradients ADDED to persistent accumulators
    for deferred in (False, True):
        for q in mlp.parameters():
            q.grad = None
            q._eqh_gbuf = torch.full_like(q, 0.5)
        xg2, eg2 = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
        if deferred:
            ops.defer_begin(DEV)
        loss2, _ = ops.readout_pair_mse(xg2, eg2, index, None, order, mlp, y.to(DEV), n_real, unit_grad=True, **kw)
        loss2.backward()
        if deferred:
            ops.defer_flush(DEV)
        assert float(loss2.detach()) == float(loss.detach())
        assert torch.equal(xg2.grad, xg.grad / 3.0) or _rel(xg2.grad, c["xd"].grad) < lim["dx"]
        assert torch.equal(eg2.grad, eg.grad / 3.0) or _rel(eg2.grad, c["ed"].grad) < lim["dx"]
        for (n, q), qr in zip(mlp.named_parameters(), c["ref"].parameters()):
            assert q.grad is None, n
            assert _rel(q._eqh_gbuf - 0.5, qr.grad) < lim["param"], (n, deferred)
        for q in mlp.parameters():
            del q._eqh_gbuf


@pytest.mark.parametrize("p_x,p_h", [(0.0, 0.0), (0.1, 0.1)])
def test_two_runs_are_bitwise_equal(p_x, p_h):
    """no atomics, fixed-order slab sums: loss, predictions, dX, dE and the ten gradients of two runs are the same bits"""
    ops = _ops()
    C, H, B, n_real = 256, 256, 37, 33
    c = _case(C, H, B, n_real, p_x, p_h)
    mlp = c["mlp"].to(DEV).train()
    index, order, y = _index(c, B), c["order"].to(DEV), c["y"].to(DEV)
    seeds = _device_seeds(p_x, p_h) if (p_x > 0 or p_h > 0) else None

    def run():
        for q in mlp.parameters():
            q.grad = None
        x, e = c["x"].to(DEV).requires_grad_(True), c["e"].to(DEV).requires_grad_(True)
        loss, pred = ops.readout_pair_mse(x, e, index, None, order, mlp, y, n_real, p_x=p_x, seeds=seeds)
        loss.backward()
        return [loss.detach().clone(), pred.clone(), x.grad.clone(), e.grad.clone()] + [q.grad.clone() for q in mlp.parameters()]

    first, again = run(), run()
    assert len(first) == 14 and all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(bool(torch.isfinite(t).all()) for t in first)


def _count(monkeypatch, *names):
    """Count the calls of the native entry points ``names`` (as tests/test_hip_readout_dropout.py does)"""
    from equihgnn_amd import hip
    lib, calls = hip.lib(), {n: 0 for n in names}
    for n in names:
        def counted(*a, _n=n, _inner=getattr(lib, n)):
            calls[_n] += 1
            return _inner(*a)
        monkeypatch.setattr(lib, n, counted, raising=True)
    return calls


def _model(method, dropout):
    from equihgnn_amd import models
    m = models.MODELS[method](1, golden_args(method, 64, dropout=dropout, All_num_layers=2, output_hidden=64))
    fill_state_dict(m, 13)
    return m.to(DEV)


NEW = ("hg_readout_pair_mse_f32", "hg_readout_pair_mse_drop_f32")


@pytest.mark.parametrize("P", [0.0, 0.3])
@pytest.mark.parametrize("method", ["mhnn", "egnn_equihnn"])
def test_models_are_the_same_function_with_the_switch_on_and_off(method, P, monkeypatch):
    """mhnn and egnn_equihnn at MLP_hidden = 64, output_hidden = 64 (head 128 -> 128 -> 128 -> 1), training, with a head, under
    one seed pool (torch.manual_seed in front of the pass): with the switch on the new entry -- its drop form under dropout --
    runs exactly once and never with it off; under dropout the head's two hg_bias_relu_ln_drop_fwd launches are gone and so
    are the last application's two faf_dropout_add passes, each way (2 fewer calls in the forward pass, 2 fewer in the
    backward); loss and every gradient agree with the switch-off run within the float64 test's limits.  In eval mode, with
    taps and without a head the entry is never called."""
    ops = _ops()
    lim = _limits(P, P)
    data = make_batch(11, 7).to(DEV)            # 8 molecules with the isolated one (no hyperedge at all)
    m = _model(method, P).train()
    calls = _count(monkeypatch, *NEW, "hg_bias_relu_ln_drop_fwd", "faf_dropout_add")

    def step(switch):
        monkeypatch.setattr(ops, "PAIRED_READOUT", switch)
        for n in calls:
            calls[n] = 0
        for q in m.parameters():
            q.grad = None
        torch.manual_seed(21)                     # the seed pool's draw
        loss = m(data, head=(data.y.view(-1), None))
        fwd = dict(calls)
        loss.backward()
        return float(loss.detach()), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}, fwd, dict(calls)

    loss_on, g_on, fwd_on, on = step(True)
    # --- the path: this is what fails without the feature
    assert (on[NEW[0]], on[NEW[1]]) == ((0, 1) if P > 0 else (1, 0)), on
    loss_off, g_off, fwd_off, off = step(False)
    assert off[NEW[0]] == 0 and off[NEW[1]] == 0, off
    if P > 0:
        assert on["hg_bias_relu_ln_drop_fwd"] == off["hg_bias_relu_ln_drop_fwd"] - 2, (on, off)
        assert fwd_on["faf_dropout_add"] == fwd_off["faf_dropout_add"] - 2, (fwd_on, fwd_off)
        assert on["faf_dropout_add"] - fwd_on["faf_dropout_add"] == off["faf_dropout_add"] - fwd_off["faf_dropout_add"] - 2, (on, off)
    print(f"{method} p={P}: loss {loss_on} vs {loss_off}")
    assert abs(loss_on - loss_off) < lim["loss"] * max(1.0, abs(loss_off))
    assert sorted(g_on) == sorted(g_off) and len(g_off) > 10
    for n in g_off:
        err = float((g_on[n] - g_off[n]).abs().max() / g_off[n].abs().max().clamp(min=1e-9))
        print(f"{method} p={P} {n}: {err:.2e}")
        assert err < lim["param"], (n, err)
    # --- eval mode, taps, no head: the path it was
    monkeypatch.setattr(ops, "PAIRED_READOUT", True)
    for n in calls:
        calls[n] = 0
    m(data, taps={}, head=(data.y.view(-1), None)).backward()
    out = m(data)
    assert out.shape == (data.y.view(-1).shape[0],)
    m.eval()
    with torch.no_grad():
        m(data, head=(data.y.view(-1), None))
        m(data)
    assert calls[NEW[0]] == 0 and calls[NEW[1]] == 0, dict(calls)


def test_one_graphed_training_step(monkeypatch):
    """GraphedTrainStep on mhnn with the switch on: the eager first step, the capture and two replays (lr 0, no dropout: the
    replays repeat the captured step bit for bit), the loss of the switch-off step within the limits, and a gradient for every
    parameter the switch-off step reaches."""
    import copy
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    ops = _ops()
    lim = _limits(0.0, 0.0)
    m_on = _model("mhnn", 0.0).train()
    m_off = copy.deepcopy(m_on)
    raw = synth_batch(8, 900)
    batch = pad_batch(raw, *bucket_sizes(raw.num_nodes, raw.num_hyperedges, raw.nnz, 64)).to(DEV)
    batch.num_real_graphs = 8
    calls = _count(monkeypatch, *NEW)
    got = {}
    for switch, model in ((True, m_on), (False, m_off)):
        monkeypatch.setattr(ops, "PAIRED_READOUT", switch)
        batch._hyper_index = None
        tr = GraphedTrainStep(model, lr=0.0, keep_grads=True)
        tr.index_prefetch = False
        losses = [float(tr.step(batch)) for _ in range(4)]          # eager, capture, replay, replay
        torch.cuda.synchronize()
        assert len(tr.slots) == 1 and all(np.isfinite(losses)), losses
        assert losses[2] == losses[3], losses
        got[switch] = (losses, {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None})
        tr.close()
        if switch:
            assert calls[NEW[0]] >= 2 and calls[NEW[1]] == 0, dict(calls)      # the eager step and the capture; no call per replay
            on_calls = dict(calls)
    assert dict(calls) == on_calls                                             # never with the switch off
    (l_on, g_on), (l_off, g_off) = got[True], got[False]
    print("graphed mhnn, switch on / off:", l_on, l_off)
    for a, b in zip(l_on, l_off):
        assert abs(a - b) < lim["loss"] * max(1.0, abs(b)), (l_on, l_off)
    assert sorted(g_on) == sorted(g_off) and len(g_off) > 10
    for n in g_off:
        assert bool(torch.isfinite(g_on[n]).all()), n
        assert (float(g_on[n].abs().max()) > 0) == (float(g_off[n].abs().max()) > 0), n
        err = float((g_on[n] - g_off[n]).abs().max() / g_off[n].abs().max().clamp(min=1e-9))
        assert err < lim["param"], (n, err)
