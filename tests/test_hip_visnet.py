"""GPU: the ViSNet front-end (vis_* kernels) against a float64 restatement of the reference (tests/visnet_ref.py): the
radius graph and its slot geometry, the full front-end forward and every parameter gradient, padded against unpadded
batches, run-to-run bit equality, and the three wrappers end to end."""
import numpy as np
import pytest
import torch

import visnet_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _batch(seed, n_mols=6, C_flavour="qm9"):
    """Synthetic molecules plus the crafted ones: a compact 24-atom molecule (every pair within 5 A: the 16-neighbour
    truncation binds), a one-atom molecule, and a molecule whose last atom lies 9 A from the rest (no neighbour in
    radius).  Molecules share the same region of space, so only the per-molecule search keeps them apart."""
    from equihgnn_amd.batch import collate, synth_molecule
    rng = np.random.default_rng(seed)
    mols = [synth_molecule(rng, C_flavour) for _ in range(n_mols)]
    dense = synth_molecule(rng, C_flavour, n_atoms=24)
    dense.pos[:] = rng.uniform(-1.6, 1.6, size=dense.pos.shape).astype(np.float32)
    lone = synth_molecule(rng, C_flavour, n_atoms=3)
    lone.pos[:] = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]], dtype=np.float32)   # three lone atoms
    far = synth_molecule(rng, C_flavour, n_atoms=6)
    far.pos[-1] = np.array([9.0, 9.0, 9.0], dtype=np.float32)
    mols = mols[:2] + [dense] + mols[2:] + [far]
    b = collate(mols + [lone])
    return b, mols, lone


def _margin(pos, batch):
    """Smallest |d2 - 25| over candidate pairs of a molecule (the strict < must not flip between fp32 and fp64)."""
    p = pos.double().cpu()
    m = float("inf")
    for b in batch.unique():
        idx = torch.nonzero(batch.cpu() == b).reshape(-1)
        d = p[idx].unsqueeze(0) - p[idx].unsqueeze(1)
        m = min(m, float((d.pow(2).sum(-1) - 25.0).abs().min()))
    return m


def _visnet(C, seed=0):
    from equihgnn_amd.visnet import ViSNet
    torch.manual_seed(seed)
    m = ViSNet(hidden_channels=C, lmax=2, max_num_neighbors=16)
    with torch.no_grad():      # non-trivial LayerNorm / bias values
        for n, p in m.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _index(b):
    from equihgnn_amd.index import HyperIndex
    return HyperIndex.from_batch(b)


def test_radius_graph_and_geometry():
    b, _, _ = _batch(1)
    b = b.to(DEV)
    m = _visnet(64)
    de = m.representation_model.distance_expansion.to(DEV)
    g = _index(b).radius(b.pos, 5.0, 16, de.means, de.betas)
    ei, eid = g.edge_index()
    want = visnet_ref.radius_graph(b.pos, b.batch)
    assert torch.equal(ei.cpu(), want)
    cnt = g.cnt.cpu()
    assert int(cnt.max()) == 16                                          # the truncation binds somewhere
    assert int(cnt.min()) == 1                                           # an atom with only its self-loop
    src, dst = want
    # geometry against float64
    pos = b.pos.double().cpu()
    vec = pos[src] - pos[dst]
    w = vec.norm(dim=-1)
    mask = src != dst
    rbf_ref = visnet_ref._cut(w).unsqueeze(-1) * torch.exp(
        -de.betas.double().cpu() * (torch.exp(-w).unsqueeze(-1) - de.means.double().cpu()) ** 2)
    vec[mask] = vec[mask] / w[mask].unsqueeze(-1)
    sh_ref = visnet_ref._sphere(vec)
    eid = eid.cpu()
    torch.testing.assert_close(g.r.cpu()[eid].double(), w, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(g.cut.cpu()[eid].double(), visnet_ref._cut(w), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(g.rbf.cpu()[eid].double(), rbf_ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(g.sh.cpu()[eid].double(), sh_ref, rtol=1e-5, atol=1e-5)
    empty = torch.ones(g.r.numel(), dtype=torch.bool)
    empty[eid] = False
    assert float(g.rbf.cpu()[empty].abs().sum()) == 0 and float(g.cut.cpu()[empty].abs().sum()) == 0
    # the transposed (by-source) lists: every kept edge exactly once, ascending edge id
    starts, counts, lst = g.src_start.cpu(), g.src_cnt.cpu(), g.src_eid.cpu()
    seen = []
    for j in range(cnt.numel()):
        e = lst[starts[j]:starts[j] + counts[j]]
        assert torch.all(e[1:] > e[:-1])
        assert torch.all(g.slot.reshape(-1).cpu()[e.long()] == j)
        seen += e.tolist()
    assert sorted(seen) == sorted(eid.tolist())


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("C", [64, 256])
def test_front_end_matches_float64_reference(C):
    b, _, _ = _batch(2 + C)
    assert _margin(b.pos, b.batch) > 1e-3
    m = _visnet(C, seed=C)
    sd64 = {k: v.double().clone().requires_grad_(v.is_floating_point() and k in dict(m.named_parameters()))
            for k, v in m.state_dict().items()}
    want = visnet_ref.visnet(sd64, b.x, b.pos, b.batch)
    wgt = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    (want * wgt).sum().backward()

    m = m.to(DEV)
    bd = b.to(DEV)
    got = m(bd.x, bd.pos, _index(bd))
    (got * wgt.float().to(DEV)).sum().backward()
    assert _rel(got.detach().cpu(), want.detach()) < 1e-3, _rel(got.detach().cpu(), want.detach())
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        gr = sd64[n].grad
        if float(gr.abs().max()) == 0:
            assert float(p.grad.abs().max()) == 0, n
            continue
        assert _rel(p.grad.cpu(), gr) < 5e-3, (n, _rel(p.grad.cpu(), gr))
    # the last block's vector output reaches the loss only through "* 0": zero gradients, not None
    last = m.output_model.output_network[1]
    assert float(last.vec2_proj.weight.grad.abs().max()) == 0
    assert float(last.update_net[2].weight.grad[C:].abs().max()) == 0


def test_padded_batch_matches_unpadded():
    from equihgnn_amd.batch import pad_batch
    b, _, _ = _batch(7)
    N, M, nnz = b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0]
    p = pad_batch(b, N + 9, M + 3, nnz + 4)
    p.pos[N:] = 3.0e4               # every pad atom on one position
    outs = []
    for bb in (b, p):
        m = _visnet(64, seed=3).to(DEV)
        bd = bb.to(DEV)
        y = m(bd.x, bd.pos, _index(bd))
        y[:N].square().sum().backward()
        grads = {n: q.grad.clone() for n, q in m.named_parameters()}
        assert all(torch.isfinite(t).all() for t in grads.values())
        outs.append((y[:N].detach(), grads))
    torch.testing.assert_close(outs[1][0], outs[0][0], rtol=1e-5, atol=1e-6)
    for n in outs[0][1]:
        torch.testing.assert_close(outs[1][1][n], outs[0][1][n], rtol=1e-4, atol=1e-6)


def test_gradients_are_bitwise_reproducible():
    b, _, _ = _batch(11)
    bd = b.to(DEV)
    runs = []
    for _ in range(2):
        m = _visnet(256, seed=1).to(DEV)
        bd._hyper_index = None
        y = m(bd.x, bd.pos, _index(bd))
        y.square().sum().backward()
        runs.append([q.grad.clone() for q in m.parameters()])
    assert all(torch.equal(a, c) for a, c in zip(*runs))


@pytest.mark.parametrize("name,extra", [("visnet_equihnns", {}), ("visnet_equihnn", {}),
                                        ("visnet_equihnnm", {"normalization": "bn"})])
def test_wrappers_train_and_pad(name, extra):
    """Each wrapper: finite loss and gradients, and a padded batch gives the real molecules the unpadded results."""
    from equihgnn_amd.batch import pad_batch
    import equihgnn_amd.models  # noqa: F401  (registers the classes)
    from equihgnn_amd.registry import default_args, registry
    b, _, _ = _batch(13)
    B = b.y.shape[0]
    N, M, nnz = b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0]
    res = []
    for bb in (b, pad_batch(b, N + 7, M + 3, nnz + 4)):
        torch.manual_seed(0)
        m = registry.get_model_class(name)(1, default_args(MLP_hidden=64, output_hidden=32, **extra)).to(DEV).train()
        bd = bb.to(DEV)
        out = m(bd)
        loss = torch.nn.functional.mse_loss(out[:B], bd.y[:B])
        loss.backward()
        g = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
        assert torch.isfinite(loss) and all(torch.isfinite(t).all() for t in g.values())
        assert any("visnet_layer" in n for n in g)
        res.append((out[:B].detach(), g))
    torch.testing.assert_close(res[1][0], res[0][0], rtol=1e-4, atol=1e-5)
    for n in res[0][1]:
        torch.testing.assert_close(res[1][1][n], res[0][1][n], rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize("prefetch", [False, True])
def test_graphed_train_step_follows_eager(prefetch):
    import copy

    from equihgnn_amd.batch import pad_batch, synth_batch
    import equihgnn_amd.models  # noqa: F401  (registers the classes)
    from equihgnn_amd.registry import default_args, registry
    from equihgnn_amd.trainer import GraphedTrainStep
    torch.manual_seed(0)
    m1 = registry.get_model_class("visnet_equihnns")(1, default_args(MLP_hidden=64, output_hidden=32)).to(DEV).train()
    m2 = copy.deepcopy(m1)
    batches = []
    for i in range(5):
        bb = synth_batch(8, 900 + i)
        batches.append(pad_batch(bb, 256, 320, 800).to(DEV))
    tr = GraphedTrainStep(m1, lr=1e-3)
    tr.index_prefetch = prefetch
    losses = []
    for i, bb in enumerate(batches):
        nxt = batches[i + 1] if (prefetch and i + 1 < len(batches)) else None
        losses.append(float(tr.step(bb, nxt) if nxt is not None else tr.step(bb)))
    opt, ref = None, []
    for bb in batches:
        for q in m2.parameters():
            q.grad = None
        bb._hyper_index = None
        loss = torch.nn.functional.mse_loss(m2(bb)[:8], bb.y[:8])
        loss.backward()
        if opt is None:
            opt = torch.optim.Adam([q for q in m2.parameters() if q.grad is not None], lr=1e-3)
        opt.step()
        ref.append(float(loss))
    np.testing.assert_allclose(losses, ref, rtol=2e-3, atol=1e-5)


def test_graphed_eval_step_matches_eager():
    from equihgnn_amd.batch import pad_batch, synth_batch
    import equihgnn_amd.models  # noqa: F401  (registers the classes)
    from equihgnn_amd.registry import default_args, registry
    from equihgnn_amd.trainer import GraphedEvalStep
    torch.manual_seed(0)
    m = registry.get_model_class("visnet_equihnns")(1, default_args(MLP_hidden=64, output_hidden=32)).to(DEV).eval()
    ev = GraphedEvalStep(m)
    for i in range(3):
        bb = pad_batch(synth_batch(8, 950 + i), 256, 320, 800).to(DEV)
        with torch.no_grad():
            want = m(bb).clone()
        bb._hyper_index = None
        got = ev(bb).clone()
        torch.testing.assert_close(got[:8], want[:8], rtol=1e-5, atol=1e-6)
