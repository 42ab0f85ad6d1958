"""GPU: the edge-message kernels of the 2-D baselines (hg_edge_msg_fwd/bwd) against float64 torch, and GNN_2D (gin / gcn)
against the golden vectors captured from the reference's baseline_2d.py (tests/golden/make_golden_2d.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import GOLDEN_DIR, assert_close, fill_state_dict  # noqa: E402

DEV = "cuda:0"
BOND = (5, 6, 2)


# ------------------------------------------------------------------------------------------------------------------
# operator level
# ------------------------------------------------------------------------------------------------------------------
def _graph(N, E, F, seed, hub=True):
    """Random directed edges over N atoms: the last 8 atoms isolated, atom 0 a hub with ~200 incoming edges, a block of
    duplicated edges, and no symmetry (every edge one-way)."""
    g = torch.Generator().manual_seed(seed)
    live = N - 8
    src = torch.randint(0, live, (E,), generator=g)
    dst = torch.randint(0, live, (E,), generator=g)
    if hub and E >= 400:
        dst[:200] = 0
        src[200:230] = src[230:260]       # 30 duplicated edges
        dst[200:230] = dst[230:260]
    attr = torch.stack([torch.randint(0, BOND[f], (E,), generator=g) for f in range(F)], 1) if E else \
        torch.zeros((0, F), dtype=torch.int64)
    return torch.stack((src, dst)), attr


def _ref_fwd(x, tabs, param, ei, attr, mode):
    """float64 restatement of GINConv / GCNConv's message passing (baseline_2d.py:19-73)."""
    N = x.shape[0]
    src, dst = ei[0], ei[1]
    offs = np.cumsum((0,) + BOND)[: attr.shape[1]]
    bond = torch.zeros((ei.shape[1], x.shape[1]), dtype=x.dtype)
    for f in range(attr.shape[1]):
        bond = bond + tabs[int(offs[f]) + attr[:, f]]
    msg = torch.relu(x[src] + bond)
    if mode == 0:
        return (1 + param) * x + torch.zeros_like(x).index_add(0, dst, msg)
    deg = torch.zeros(N, dtype=x.dtype).index_add(0, src, torch.ones(src.numel(), dtype=x.dtype)) + 1
    dis = deg.pow(-0.5)
    norm = dis[src] * dis[dst]
    return torch.zeros_like(x).index_add(0, dst, norm.unsqueeze(-1) * msg) + torch.relu(x + param) / deg.unsqueeze(-1)


def _run_op(x, tabs, param, ei, attr, mode, dout):
    from equihgnn_amd.ops.gnn2d import GraphIndex, edge_msg
    N = x.shape[0]
    gi = GraphIndex(ei.to(DEV), attr.to(DEV), torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    xd = x.float().to(DEV).requires_grad_()
    td = tabs.float().to(DEV).requires_grad_()
    pd = param.float().to(DEV).requires_grad_()
    out = edge_msg(xd, td, pd, gi, mode)
    out.backward(dout.float().to(DEV))
    return [t.detach().cpu() for t in (out, xd.grad, td.grad, pd.grad)]


@pytest.mark.parametrize("C", [64, 300])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("E", [0, 1500])
def test_edge_msg_matches_float64(C, mode, F, E):
    torch.manual_seed(C + 10 * mode + F + E)
    N = 500
    ei, attr = _graph(N, E, F, seed=C + F + E)
    T = sum(BOND[:F])
    x = torch.randn(N, C, dtype=torch.float64)
    tabs = 0.5 * torch.randn(T, C, dtype=torch.float64)
    param = 0.3 * torch.randn(1, dtype=torch.float64) if mode == 0 else 0.2 * torch.randn(1, C, dtype=torch.float64)
    dout = torch.randn(N, C, dtype=torch.float64)
    xr, tr, pr = (t.clone().requires_grad_() for t in (x, tabs, param))
    ref = _ref_fwd(xr, tr, pr, ei, attr, mode)
    ref.backward(dout)
    got = _run_op(x, tabs, param, ei, attr, mode, dout)
    assert_close(got[0].numpy(), ref.detach().numpy(), 1e-5, "out")
    for name, g, r in (("dx", got[1], xr.grad), ("dtables", got[2], tr.grad), ("dparam", got[3], pr.grad)):
        r = r.numpy()
        err = float(np.abs(g.numpy().astype(np.float64) - r).max()) / max(float(np.abs(r).max()), 1.0)
        assert err <= 2e-5, (name, err)
    # determinism: a second run is bitwise equal
    again = _run_op(x, tabs, param, ei, attr, mode, dout)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# model level: golden vectors of the reference's GNN_2D
# ------------------------------------------------------------------------------------------------------------------
GNN2D_DIR = os.path.join(GOLDEN_DIR, "gnn2d")
CASES = sorted(f[:-4] for f in os.listdir(GNN2D_DIR) if f.startswith("gnn2d_") and f.endswith(".npz"))


def _load(name):
    with np.load(os.path.join(GNN2D_DIR, name + ".npz")) as z:
        return dict(z)


def _spec(name):
    from make_golden_2d import CASES as TABLE
    return TABLE[name]


def _batch(case):
    from equihgnn_amd.batch import GBatch
    t = torch.from_numpy
    y = case["in_y"]
    return GBatch(x=t(case["in_x"]), edge_index=t(case["in_edge_index"]), edge_attr=t(case["in_edge_attr"]),
                  batch=t(case["in_batch"]), y=t(y.astype(np.float32)), num_nodes=case["in_x"].shape[0],
                  num_edges=case["in_edge_index"].shape[1], num_graphs=y.shape[0])


def _model(name):
    from equihgnn_amd.baseline_2d import GNN_2D
    gnn_type, hidden, layers, _, seed, _, _ = _spec(name)
    m = GNN_2D(1, num_layer=layers, emb_dim=hidden, gnn_type=gnn_type)
    fill_state_dict(m, seed)
    return m.to(DEV)


def _grad_err(g, ref):
    ref = ref.astype(np.float64)
    return float(np.abs(g.astype(np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.mark.parametrize("name", CASES)
def test_gnn2d_matches_reference_golden(name):
    case = _load(name)
    gnn_type, hidden, _, _, _, mode, special = _spec(name)
    model = _model(name)
    data = _batch(case).to(DEV)
    if mode == "eval":
        model.eval()
        with torch.no_grad():
            out = model(data)
        assert_close(out.cpu().numpy(), case["out"], 1e-5, "out")
        return
    model.train()
    out = model(data)
    assert_close(out.detach().cpu().numpy(), case["out"], 1e-5, "out")
    loss = torch.nn.functional.mse_loss(out, data.y)
    tol_loss = (2e-5 if mode == "f64" else 1e-5) * max(1.0, float(case["loss"]))
    assert abs(float(loss.detach()) - float(case["loss"])) <= tol_loss
    loss.backward()
    # The tolerances of test_hip_models.py: float64 fixtures 5e-5 of the largest entry; float32 captures 3e-3 (the train-mode
    # BatchNorm models), 1e-2 at the wide size.  Every train-mode row's seed keeps the reference's ReLU inputs >= 1e-5 rms
    # from the kink (make_golden_2d.relu_margin), so no ReLU can flip between the two float32 evaluations.
    tol = 5e-5 if mode == "f64" else (1e-2 if hidden > 64 else 3e-3)
    params = dict(model.named_parameters())
    assert list(case["grad_names"]) == list(params)
    for k, present in zip(case["grad_names"], case["grad_present"]):
        p = params[str(k)]
        assert (p.grad is not None) == bool(present), k
        if p.grad is None:
            continue
        g = p.grad.detach().cpu().numpy()
        ref = case["g:" + str(k)]
        g = g[: ref.shape[0]] if g.ndim == 2 else g
        if str(k).endswith(("mlp.0.bias", "mlp.3.bias")):
            # GIN: these biases feed a train-mode BatchNorm, which removes any constant shift: their gradient is zero
            # analytically, so a relative bound measures nothing; both sides hold rounding noise only (~1e-17 in float64,
            # ~1e-8..1e-6 in float32)
            assert float(np.abs(g.astype(np.float64) - ref).max()) <= 1e-5, str(k)
            continue
        if special == "e0" and str(k).endswith(".eps"):
            # no edges: the conv is mlp((1 + eps) x), and the train-mode BatchNorm behind the first Linear is invariant to
            # that scale up to its own eps term -- d eps is ~1e-6 against ~1e-1 with edges, i.e. rounding-level on both sides
            assert float(np.abs(g.astype(np.float64) - ref).max()) <= 1e-5, str(k)
            continue
        assert _grad_err(g, ref) <= tol, (str(k), _grad_err(g, ref))
    sd = model.state_dict()
    for k in case:
        if k.startswith("rs:"):
            assert_close(sd[k[3:]].cpu().numpy(), case[k], 1e-5, k)


def test_edge_msg_large_n_matches_float64():
    """C = 300 at 70 000 atoms: past the forward's grid-stride bound (16 384 workgroups x 3 rows) and the backward's
    2 048-workgroup cap (several rows per lane group), with molecule-like local edges; float64 reference on the device.
    At 4e7 ReLU inputs some lie within float32 rounding of zero, so the reference takes each ReLU's on/off decision from the
    float32 pre-activation the kernels form (same summation order) and everything else in float64."""
    from equihgnn_amd.ops.gnn2d import GraphIndex, edge_msg
    N, C, F = 70000, 300, 3
    g = torch.Generator(device=DEV).manual_seed(5)
    E = 2 * N
    src = torch.randint(0, N, (E,), device=DEV, generator=g)
    dst = (src + torch.randint(-15, 16, (E,), device=DEV, generator=g)).clamp(0, N - 1)
    attr = torch.stack([torch.randint(0, BOND[f], (E,), device=DEV, generator=g) for f in range(F)], 1)
    gi = GraphIndex(torch.stack((src, dst)), attr, torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    offs = (0, 5, 11)
    for mode in (0, 1):
        x = torch.randn(N, C, device=DEV, generator=g)
        tabs = 0.5 * torch.randn(13, C, device=DEV, generator=g)
        param = (0.3 * torch.randn(1, device=DEV, generator=g) if mode == 0
                 else 0.2 * torch.randn(1, C, device=DEV, generator=g))
        dout = torch.randn(N, C, device=DEV, generator=g)
        xr, tr, pr = (t.double().requires_grad_() for t in (x, tabs, param))
        bond = sum(tr[offs[f] + attr[:, f]] for f in range(F))
        bond32 = tabs[offs[0] + attr[:, 0]] + tabs[offs[1] + attr[:, 1]] + tabs[offs[2] + attr[:, 2]]
        msg = torch.where(x[src] + bond32 > 0, xr[src] + bond, torch.zeros((), dtype=torch.float64, device=DEV))
        if mode == 0:
            ref = (1 + pr) * xr + torch.zeros_like(xr).index_add(0, dst, msg)
        else:
            deg = torch.zeros(N, dtype=torch.float64, device=DEV).index_add(0, src, torch.ones(E, dtype=torch.float64,
                                                                                                device=DEV)) + 1
            dis = deg.pow(-0.5)
            ref = (torch.zeros_like(xr).index_add(0, dst, (dis[src] * dis[dst]).unsqueeze(-1) * msg)
                   + torch.where(x + param > 0, xr + pr, torch.zeros((), dtype=torch.float64, device=DEV))
                   / deg.unsqueeze(-1))
        ref.backward(dout.double())
        xd, td, pd = (t.clone().requires_grad_() for t in (x, tabs, param))
        out = edge_msg(xd, td, pd, gi, mode)
        out.backward(dout)
        for name, got, want in (("out", out, ref), ("dx", xd.grad, xr.grad), ("dtables", td.grad, tr.grad),
                                ("dparam", pd.grad, pr.grad)):
            want = want.detach()
            err = float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1.0)
            assert err <= 2e-5, (mode, name, err)


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_msg_bwd_accumulates_inside_the_deferral_window(mode):
    """accumulate != 0: dtables is added to, and inside ops.defer_begin/flush the addition waits for the flush (one batched
    reduction launch) -- the path the model takes when the bond tables own persistent accumulators.  dextra (d eps / d root)
    is overwritten at once either way: autograd reads it before the window closes."""
    from equihgnn_amd import hip, ops
    from equihgnn_amd.ops._base import _ptr, _stream
    from equihgnn_amd.ops.gnn2d import GraphIndex
    N, C, F, T = 500, 300, 3, 13
    ei, attr = _graph(N, 1500, F, seed=9)
    gi = GraphIndex(ei.to(DEV), attr.to(DEV), torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    g = torch.Generator(device=DEV).manual_seed(1)
    x, dout = torch.randn(N, C, device=DEV, generator=g), torch.randn(N, C, device=DEV, generator=g)
    tabs = torch.randn(T, C, device=DEV, generator=g)
    param = torch.full((1,), 0.2, device=DEV) if mode == 0 else torch.randn(1, C, device=DEV, generator=g)
    eps, root = (param, None) if mode == 0 else (None, param)
    L = hip.lib()
    ws_bytes = L.hg_edge_msg_bwd_workspace_bytes(N, C, T)
    st = _stream(DEV)

    def bwd(dtab, dextra, acc, ws):
        hip.check(L.hg_edge_msg_bwd(mode, _ptr(x), _ptr(tabs), T, F, _ptr(gi.by_src.rowptr), _ptr(gi.dst_of_src),
                                    _ptr(gi.code_src), _ptr(eps), _ptr(root), _ptr(dout), N, C, _ptr(torch.empty_like(x)),
                                    _ptr(dtab), _ptr(dextra), acc, _ptr(ws), ws_bytes, st), "hg_edge_msg_bwd")

    fresh_t, fresh_e = torch.empty(T, C, device=DEV), torch.empty(C, device=DEV)
    bwd(fresh_t, fresh_e, 0, torch.empty(ws_bytes, dtype=torch.uint8, device=DEV))
    base_t, base_e = torch.randn(T, C, device=DEV, generator=g), torch.randn(C, device=DEV, generator=g)
    acc_t, acc_e = base_t.clone(), base_e.clone()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ops.defer_begin(torch.device(DEV))
    try:
        bwd(acc_t, acc_e, 1, ws)
        torch.cuda.synchronize()
        assert torch.equal(acc_t, base_t) and torch.equal(acc_e, fresh_e)     # tables recorded, not yet reduced
    finally:
        ops.defer_flush(torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(acc_t, base_t + fresh_t) and torch.equal(acc_e, fresh_e)
    bwd(acc_t, acc_e, 1, ws)                                                 # outside a window: added at once
    torch.cuda.synchronize()
    assert torch.equal(acc_t, base_t + fresh_t + fresh_t) and torch.equal(acc_e, fresh_e)


@pytest.mark.parametrize("gnn_type", ["gin", "gcn"])
def test_gnn2d_padded_batch_matches_unpadded(gnn_type):
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import graph_bucket_sizes, pad_graph_batch, synth_graph_batch

    b = synth_graph_batch(16, 5, "pcqm")
    p = pad_graph_batch(b, *graph_bucket_sizes(b.num_nodes, b.num_edges))
    assert p.num_nodes > b.num_nodes and p.num_edges > b.num_edges
    results = []
    for data in (b, p):
        m = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type=gnn_type)
        fill_state_dict(m, 7)
        m.to(DEV).train()
        d = data.to(DEV)
        nb = b.num_graphs
        loss = m(d, head=(d.y, nb))
        loss.backward()
        m.eval()
        with torch.no_grad():
            ev = m(d)[:nb]
        results.append((float(loss), {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None},
                        {k: v.detach().cpu() for k, v in m.state_dict().items() if "running" in k}, ev.cpu()))
    (l0, g0, r0, e0), (l1, g1, r1, e1) = results
    assert abs(l0 - l1) <= 1e-5 * max(1.0, abs(l0))
    assert set(g0) == set(g1)
    for k in g0:
        err = float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30)
        assert err <= 1e-4, (k, err)
    for k in r0:
        assert torch.allclose(r0[k], r1[k], rtol=1e-5, atol=1e-6), k
    assert_close(e1.numpy(), e0.numpy(), 1e-5, "eval outputs")


# ------------------------------------------------------------------------------------------------------------------
# trainers
# ------------------------------------------------------------------------------------------------------------------
def _padded_batches(n, seed, sizes):
    from equihgnn_amd.batch import pad_graph_batch, synth_graph_batch
    out = []
    for i in range(n):
        b = synth_graph_batch(8, seed + i, "pcqm")
        p = pad_graph_batch(b, *sizes[i % len(sizes)])
        out.append(p.to(DEV))
    return out


@pytest.mark.parametrize("gnn_type", ["gin", "gcn"])
def test_graphed_train_step_follows_the_eager_trajectory(gnn_type):
    """GraphedTrainStep (one captured step per (atoms, edges, molecules) bucket) against an eager loop -- model(data) ->
    mse_loss -> backward -> torch.optim.Adam -- over 10 steps that switch between two buckets."""
    import copy

    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.trainer import GraphedTrainStep

    torch.manual_seed(0)
    m1 = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type=gnn_type)
    fill_state_dict(m1, 3)
    m1.to(DEV).train()
    m2 = copy.deepcopy(m1)
    batches = _padded_batches(10, 300, [(384, 768), (512, 1024)])
    tr = GraphedTrainStep(m1, lr=1e-3)
    losses = [float(tr.step(b)) for b in batches]
    assert len(tr.slots) == 2
    opt, ref = None, []
    for b in batches:
        for p in m2.parameters():
            p.grad = None
        loss = torch.nn.functional.mse_loss(m2(b)[:8], b.y[:8])
        loss.backward()
        if opt is None:
            opt = torch.optim.Adam([p for p in m2.parameters() if p.grad is not None], lr=1e-3)
        opt.step()
        ref.append(float(loss))
    np.testing.assert_allclose(losses, ref, rtol=2e-4, atol=1e-6)


@pytest.mark.parametrize("gnn_type", ["gin", "gcn"])
def test_graphed_eval_step_matches_eager_eval(gnn_type):
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.trainer import GraphedEvalStep

    m = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type=gnn_type)
    fill_state_dict(m, 4)
    m.to(DEV).eval()
    ev = GraphedEvalStep(m)
    for b in _padded_batches(3, 700, [(384, 768)]):
        with torch.no_grad():
            want = m(b).clone()
        got = ev(b).clone()
        assert torch.equal(got[:8], want[:8])
