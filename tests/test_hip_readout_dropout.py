"""Training dropout on the fused read-out head (the DROP form of k_readout_mse, hg_readout_mse_drop_f32; csrc/readout.hip,
ops/readout.py, layers.readout, models._STail): the operator against float64 autograd with the masks made explicit, against
the separate launches it replaces under the same seeds, the seeds read from device memory, and the models' launch lists.

The keep matrix of a site is what ``ops.dropout_add(ones[R, C], None, p, seed)`` returns; here it is ALSO computed on the host by
the numpy twin of csrc/drop_hash.h in tests/test_readout_dropout_host.py, and the two are asserted equal, so a case (a seed whose
float64 pre-activations keep away from the ReLU kink WITH the masks applied) is chosen without the device.

Tolerances (``_limits``): those of tests/test_hip_kernels.py::test_readout_mse_matches_float64_reference -- 2e-5 / 1e-5 on the
predictions, 1e-5 on the loss, 3e-5 on dX, 5e-5 on the parameter gradients -- times 1 / (1 - p) for each mask on the path: the
pre-pool mask and the two hidden masks sit in front of the prediction and, read backwards, in front of dX and of W1's gradient,
so every limit takes s = 1 / ((1 - p_x) (1 - p_h)^2)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import fill_state_dict, golden_args, make_batch  # noqa: E402
from test_readout_dropout_host import keep_matrix  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional
SHAPES = [(256, 128, 37, 33), (64, 64, 16, 16), (128, 64, 5, 4),
          (256, 128, 257, 256),     # the 17th workgroup holds one padding molecule
          (128, 128, 11, 10)]       # molecules of up to 150 atoms: several pooling rounds
PROBS = [(0.0, 0.1), (0.1, 0.1), (0.5, 0.3)]
SEEDS = (0x1234567, 0x89ABCDEF01, 0x3C3C3C3C3C3C)        # pre-pool, hidden 1, hidden 2


def _ops():
    from equihgnn_amd import ops
    return ops


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _limits(p_x, p_h):
    s = 1.0 / ((1.0 - p_x) * (1.0 - p_h) ** 2)
    return dict(pred_atol=2e-5 * s, pred_rtol=1e-5 * s, loss=1e-5 * s, dx=3e-5 * s, param=5e-5 * s)


def _rel(a, b):
    b = b.detach().cpu().double()
    return float((a.detach().cpu().double() - b).abs().max() / b.abs().max().clamp(min=1e-9))


def _head(C, H, p_h, seed):
    from equihgnn_amd.layers import MLP
    torch.manual_seed(seed)
    mlp = MLP(C, H, 1, 3, dropout=p_h, Normalization="ln", InputNorm=False)
    g = torch.Generator().manual_seed(seed + 1)
    for q in mlp.parameters():
        q.data.add_(0.1 * torch.randn(q.shape, generator=g))
    return mlp


def _forward64(ref, xd, batch, B, H, keeps):
    """the head in float64 with the three masks as tensors: (predictions, smallest |pre-activation|)"""
    kx, k1, k2 = keeps
    pooled = torch.zeros(B, xd.shape[1], dtype=torch.double).index_add_(0, batch, xd * kx)
    h, margin = pooled, float("inf")
    for i, k in enumerate((k1, k2)):
        pre = ref.lins[i](h)
        margin = min(margin, float(pre.detach().abs().min()))
        h = F.layer_norm(torch.relu(pre), (H,), ref.normalizations[i + 1].weight, ref.normalizations[i + 1].bias, 1e-5) * k
    return ref.lins[2](h).view(-1), margin


def _case(C, H, B, n_real, p_x, p_h):
    """The first seed whose float64 pre-activations, masks applied, all keep 2e-5 from the ReLU kink (a ReLU input within fp32
    rounding of zero has a different derivative in float32 and in float64): host only, the masks are the numpy twin's."""
    from equihgnn_amd.layers import MLP
    for seed in range(C + H + B, C + H + B + 200):
        g = torch.Generator().manual_seed(seed)
        sizes = torch.randint(1, 150 if B == 11 else 30, (B,), generator=g)
        sizes[min(2, B - 1)] = 0                               # a molecule without atoms pools to zero
        rowptr64 = torch.cat((torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)))
        N = int(rowptr64[-1])
        x = torch.randn(N, C, generator=g)
        y = torch.randn(B, generator=g)
        mlp = _head(C, H, p_h, B)
        ref = MLP(C, H, 1, 3, dropout=0.0, Normalization="ln", InputNorm=False).double()
        ref.load_state_dict({k: v.double() for k, v in mlp.state_dict().items()})
        keeps = (torch.from_numpy(keep_matrix(N, C, p_x, SEEDS[0])).double(),
                 torch.from_numpy(keep_matrix(B, H, p_h, SEEDS[1])).double(),
                 torch.from_numpy(keep_matrix(B, H, p_h, SEEDS[2])).double())
        xd = x.double().requires_grad_(True)
        batch = torch.repeat_interleave(torch.arange(B), sizes)
        out, margin = _forward64(ref, xd, batch, B, H, keeps)
        if margin >= 2e-5:
            break
    assert margin >= 2e-5
    loss_ref = ((out[:n_real] - y[:n_real].double()) ** 2).mean()
    loss_ref.backward()
    return dict(rowptr64=rowptr64, N=N, x=x, y=y, mlp=mlp, ref=ref, xd=xd, out=out.detach(), loss=float(loss_ref.detach()), keeps=keeps)


def _device_seeds(p_x, p_h):
    return (_seed(SEEDS[0]) if p_x > 0 else None, _seed(SEEDS[1]) if p_h > 0 else None, _seed(SEEDS[2]) if p_h > 0 else None)


@pytest.mark.parametrize("p_x,p_h", PROBS)
@pytest.mark.parametrize("C,H,B,n_real", SHAPES)
def test_readout_mse_under_dropout_matches_float64_with_explicit_masks(C, H, B, n_real, p_x, p_h):
    """pool -> MLP(C, H, H, 1; LN after ReLU, dropout behind the LN) -> MSE over the first n_real molecules with the three
    dropout sites inside the one launch, against the same head in float64 autograd times the keep matrices; the incoming
    gradient is 3; then the accumulate-in-place mode the trainer uses, eagerly and with the reductions deferred."""
    ops = _ops()
    c = _case(C, H, B, n_real, p_x, p_h)
    lim = _limits(p_x, p_h)
    N, rowptr64, x, y = c["N"], c["rowptr64"], c["x"], c["y"]
    seeds = _device_seeds(p_x, p_h)
    # the masks the expectation was built from are the device's
    for (rows, cols, p, s), k in zip(((N, C, p_x, seeds[0]), (B, H, p_h, seeds[1]), (B, H, p_h, seeds[2])), c["keeps"]):
        if p > 0:
            got = ops.dropout_add(torch.ones(rows, cols, device=DEV), None, p, s).cpu()
            assert torch.equal(got, k.float()), "the numpy twin of drop_hash.h disagrees with the device"
            assert 0.0 < float((got == 0).float().mean()) < 1.0
    mlp = c["mlp"].to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    rowptr = rowptr64.int().to(DEV)
    assert ops.readout_mse_drop_supported(xg, mlp, p_x) and not ops.readout_mse_supported(xg, mlp)
    loss, pred = ops.readout_mse(xg, rowptr, mlp, y.to(DEV), n_real, p_x=p_x, seeds=seeds)
    (3.0 * loss).backward()                                # a non-unit incoming gradient scales everything
    out = c["out"]
    perr = float(((pred[:n_real].cpu().double() - out[:n_real]).abs() - lim["pred_rtol"] * out[:n_real].abs()).max())
    errs = {"dx": _rel(xg.grad / 3.0, c["xd"].grad)}
    for (n, q), qr in zip(mlp.named_parameters(), c["ref"].parameters()):
        errs[n] = _rel(q.grad / 3.0, qr.grad)
    print(f"C={C} H={H} B={B} p=({p_x}, {p_h}): predictions {perr:.2e} (limit {lim['pred_atol']:.2e}), loss "
          f"{abs(float(loss.detach()) - c['loss']):.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert perr <= lim["pred_atol"]
    assert abs(float(loss.detach()) - c["loss"]) < lim["loss"] * max(1.0, c["loss"])
    assert errs["dx"] < lim["dx"]
    for n, _ in mlp.named_parameters():
        assert errs[n] < lim["param"], (n, errs[n])
    # rows of padding molecules get exactly zero
    if n_real < B:
        assert float(xg.grad[int(rowptr64[n_real]):].abs().max()) == 0.0
    # a dropped element of x gets exactly zero, a kept one does not lose its gradient to the mask
    if p_x > 0:
        real = slice(0, int(rowptr64[n_real]))
        assert float(xg.grad[real][c["keeps"][0][real] == 0].abs().max()) == 0.0
    # trainer mode: unit incoming gradient, parameter gradients ADDED to persistent accumulators
    for deferred in (False, True):
        for q in mlp.parameters():
            q.grad = None
            q._eqh_gbuf = torch.full_like(q, 0.5)
        xg2 = x.to(DEV).requires_grad_(True)
        if deferred:
            ops.defer_begin(DEV)
        loss2, _ = ops.readout_mse(xg2, rowptr, mlp, y.to(DEV), n_real, unit_grad=True, p_x=p_x, seeds=seeds)
        loss2.backward()
        if deferred:
            ops.defer_flush(DEV)
        assert float(loss2.detach()) == float(loss.detach())
        assert torch.equal(xg2.grad, xg.grad / 3.0) or _rel(xg2.grad, c["xd"].grad) < lim["dx"]
        for (n, q), qr in zip(mlp.named_parameters(), c["ref"].parameters()):
            assert q.grad is None, n
            assert _rel(q._eqh_gbuf - 0.5, qr.grad) < lim["param"], (n, deferred)
        for q in mlp.parameters():
            del q._eqh_gbuf


@pytest.mark.parametrize("p_x,p_h", PROBS)
@pytest.mark.parametrize("n_mols", [7, 40])
def test_layers_readout_is_the_same_function_with_the_switch_on_and_off(n_mols, p_x, p_h, monkeypatch):
    """layers.readout under one fixed seed pool: the one launch (draws: pre-pool, hidden 1, hidden 2) against the separate
    launches (drop(x), pool_sum, Linear, bias_relu_ln, Linear, bias_relu_ln, Linear, mse_loss: the same draws in the same
    order) -- loss, dX and the ten gradients within the float64 test's limits, the switch-off run as the reference."""
    from equihgnn_amd import hip
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import readout
    from equihgnn_amd.ops import frames
    ops = _ops()
    C, H = 64, 64
    lim = _limits(p_x, p_h)
    data = make_batch(11, n_mols).to(DEV)
    index = HyperIndex.from_batch(data)
    B, N = index.pool.n_rows, data.x.shape[0]
    x_host = torch.randn(N, C, generator=torch.Generator().manual_seed(5))
    y = torch.randn(B, generator=torch.Generator().manual_seed(6)).to(DEV)
    mlp = _head(C, H, p_h, 3).to(DEV).train()
    pool = torch.randint(0, 2 ** 62, (64,), dtype=torch.int64, generator=torch.Generator().manual_seed(8)).to(DEV)
    lib, calls = hip.lib(), {"hg_readout_mse_drop_f32": 0, "hg_readout_mse_f32": 0}
    for n in calls:
        def counted(*a, _n=n, _inner=getattr(lib, n)):
            calls[_n] += 1
            return _inner(*a)
        monkeypatch.setattr(lib, n, counted, raising=True)

    def run(switch):
        monkeypatch.setattr(ops, "READOUT_DROPOUT", switch)
        for q in mlp.parameters():
            q.grad = None
        x = x_host.to(DEV).requires_grad_(True)
        monkeypatch.setitem(frames._SEED_POOL, "buf", pool)
        monkeypatch.setitem(frames._SEED_POOL, "next", 0)
        try:
            loss = readout(mlp, x, index, None, (y, None), p_x=p_x, drop=(lambda t: ops.dropout_add(t, None, p_x)) if p_x > 0 else None)
            drawn = frames._SEED_POOL["next"]
        finally:
            monkeypatch.setitem(frames._SEED_POOL, "buf", None)
        loss.backward()
        return float(loss.detach()), x.grad.clone(), {n: q.grad.clone() for n, q in mlp.named_parameters()}, drawn

    on = run(True)
    assert calls == {"hg_readout_mse_drop_f32": 1, "hg_readout_mse_f32": 0}
    off = run(False)
    assert calls == {"hg_readout_mse_drop_f32": 1, "hg_readout_mse_f32": 0}
    assert on[3] == off[3] == (3 if p_x > 0 else 2)          # pre-pool only when p_x > 0, then hidden 1, hidden 2
    print(f"n_mols={n_mols} p=({p_x}, {p_h}): loss {abs(on[0] - off[0]):.2e}, dx {_rel(on[1], off[1]):.2e}, "
          + ", ".join(f"{n} {_rel(on[2][n], off[2][n]):.2e}" for n in on[2]))
    assert abs(on[0] - off[0]) < lim["loss"] * max(1.0, abs(off[0]))
    assert _rel(on[1], off[1]) < lim["dx"]
    assert len(on[2]) == 10
    for n in on[2]:
        assert _rel(on[2][n], off[2][n]) < lim["param"], n


def test_the_seeds_are_read_from_device_memory():
    """one run; a seed tensor changed in place: another loss; restored: the first run bit for bit (no atomics, fixed-order sums)"""
    ops = _ops()
    C, H, B, n_real, p_x, p_h = 128, 64, 37, 33, 0.1, 0.1
    g = torch.Generator().manual_seed(1)
    sizes = torch.randint(1, 30, (B,), generator=g)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), sizes.cumsum(0))).int().to(DEV)
    x_host, y = torch.randn(int(sizes.sum()), C, generator=g), torch.randn(B, generator=g).to(DEV)
    mlp = _head(C, H, p_h, 2).to(DEV).train()
    seeds = _device_seeds(p_x, p_h)

    def run():
        for q in mlp.parameters():
            q.grad = None
        x = x_host.to(DEV).requires_grad_(True)
        loss, pred = ops.readout_mse(x, rowptr, mlp, y, n_real, p_x=p_x, seeds=seeds)
        loss.backward()
        return [loss.detach().clone(), pred.clone(), x.grad.clone()] + [q.grad.clone() for q in mlp.parameters()]

    first = run()
    for i, s in enumerate(seeds):
        s.add_(1)
        other = run()
        assert float(other[0]) != float(first[0]), f"site {i} did not read its seed from the device"
        s.sub_(1)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def _count(monkeypatch, *names):
    """Count the calls of the native entry points ``names`` (as tests/test_hip_grid_trips.py does)"""
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


def _train_step(m, data, seed):
    for q in m.parameters():
        q.grad = None
    torch.manual_seed(seed)                     # the seed pool's draw
    loss = m(data, head=(data.y.view(-1), None))
    loss.backward()
    return float(loss.detach()), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("method", ["mhnns", "mhnnm"])
def test_models_run_the_fused_head_under_dropout(method, monkeypatch):
    """mhnns (S tail: the pre-pool dropout is a site of the launch) and mhnnm (M tail: the head's two sites) at C = 64, dropout
    0.3, training, with a head: hg_readout_mse_drop_f32 runs exactly once, the head's two hg_bias_relu_ln_drop_fwd launches and
    the S tail's faf_dropout_add pass in front of the pool (forward and backward) are gone; loss and every gradient agree with
    the switch-off run under the same seed pool; in eval mode and with dropout 0 the launch is hg_readout_mse_f32 as before."""
    ops = _ops()
    P = 0.3
    s_tail = method == "mhnns"
    lim = _limits(P if s_tail else 0.0, P)
    data = make_batch(11, 7).to(DEV)            # 8 molecules with the isolated one
    m = _model(method, P).train()
    names = ("hg_readout_mse_drop_f32", "hg_readout_mse_f32", "hg_bias_relu_ln_drop_fwd", "faf_dropout_add")
    calls = _count(monkeypatch, *names)
    monkeypatch.setattr(ops, "READOUT_DROPOUT", True)
    loss_on, g_on = _train_step(m, data, 21)
    on = dict(calls)
    # --- the path: this is what fails without the feature
    assert on["hg_readout_mse_drop_f32"] == 1 and on["hg_readout_mse_f32"] == 0, on
    for n in calls:
        calls[n] = 0
    monkeypatch.setattr(ops, "READOUT_DROPOUT", False)
    loss_off, g_off = _train_step(m, data, 21)
    off = dict(calls)
    assert off["hg_readout_mse_drop_f32"] == 0 and off["hg_readout_mse_f32"] == 0, off
    assert on["hg_bias_relu_ln_drop_fwd"] == off["hg_bias_relu_ln_drop_fwd"] - 2, (on, off)
    assert on["faf_dropout_add"] == off["faf_dropout_add"] - (2 if s_tail else 0), (on, off)
    print(f"{method}: loss {loss_on} vs {loss_off}")
    assert abs(loss_on - loss_off) < lim["loss"] * max(1.0, abs(loss_off))
    assert sorted(g_on) == sorted(g_off)
    for n in g_off:
        ref = g_off[n]
        if method == "mhnnm" and n.endswith(".W4.lins.1.bias"):
            # a bias in front of BatchNorm1d (the node rows of the M tail): its gradient is zero in exact arithmetic, both runs
            # hold the rounding residue of a sum that cancels (0.886 of each other, measured).  Its scale is that of the same
            # Linear's weight gradient, the other product of the same dY.
            ref = g_off[n[:-4] + "weight"]
        err = float((g_on[n] - g_off[n]).abs().max() / ref.abs().max().clamp(min=1e-9))
        print(f"{method} {n}: {err:.2e}")
        assert err < lim["param"], (n, err)
    # --- eval mode, and dropout 0: the launch it was
    monkeypatch.setattr(ops, "READOUT_DROPOUT", True)
    for model in (m.eval(), _model(method, 0.0).train()):
        for n in calls:
            calls[n] = 0
        with torch.set_grad_enabled(model.training):
            model(data, head=(data.y.view(-1), None))
        assert calls["hg_readout_mse_f32"] == 1 and calls["hg_readout_mse_drop_f32"] == 0, dict(calls)
