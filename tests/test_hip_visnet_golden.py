"""GPU: the three ViSNet wrappers against the golden vectors of the reference's own equihnn_visnet.py
(tests/golden/make_golden_visnet.py), and each vis_* operator pair, forward and backward, against float64 torch."""
import functools
import math

import numpy as np
import pytest
import torch

import visnet_ref
from common import batch_from_case, fill_state_dict, golden_args, load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("visnet_equihnns_c64", "visnet_equihnns_c256", "visnet_equihnns_c64_f64", "visnet_equihnns_c256_f64",
         "visnet_equihnn_c64", "visnet_equihnnm_c64_bn", "visnet_equihnns_pcqm_c64")


def _case_model(case):
    import make_golden_visnet as mgv

    import equihgnn_amd.models  # noqa: F401
    from equihgnn_amd.registry import registry
    name = str(case["meta_name"])
    method, hidden, seed, _, _, extra, _ = mgv.CASES[name]
    torch.manual_seed(0)
    model = registry.get_model_class(method)(1, golden_args(method, hidden, **extra))
    visnet_ref.fill_visnet_model(model, seed, fill_state_dict)
    return model.to(DEV).train()


@pytest.mark.parametrize("name", CASES)
def test_wrapper_matches_golden(name):
    case = load_case("visnet/" + name)
    case["meta_name"] = np.array(name)
    model = _case_model(case)
    data = batch_from_case(case).to(DEV)
    out = model(data)
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    ref = case["out"].astype(np.float64)
    err = np.abs(out.detach().cpu().double().numpy() - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() < 2e-4, ("out", err.max())
    assert abs(float(loss.detach()) - float(case["loss"])) <= 2e-4 * max(1.0, abs(float(case["loss"])))
    params = dict(model.named_parameters())
    rows = int(case["grad_rows"])
    # rounding floor: a gradient that is analytically ~0 (a Linear's bias in front of a train-mode BatchNorm) is rounding
    # noise on both sides, so every bound also allows 1e-5 of the largest gradient norm of the model
    floor = 1e-5 * float(np.max(case["grad_stats"][:, 2]))
    for n, present, st in zip(case["grad_names"], case["grad_present"], case["grad_stats"]):
        p = params[str(n)]
        assert (p.grad is not None) == bool(present), n
        if not present:
            continue
        g = p.grad.detach().cpu().double()
        if st[1] == 0:                                   # zero gradients of the reference stay exactly zero
            assert float(g.abs().max()) == 0, n
            continue
        scale = max(float(g.abs().max()), 1e-30)
        got = (g[:rows] if g.dim() == 2 else g).numpy()
        want = case["grad_" + str(n)].astype(np.float64)
        assert np.abs(got - want).max() <= 3e-3 * scale + floor, (n, np.abs(got - want).max() / scale)
        assert abs(float(g.norm()) - st[2]) <= 3e-3 * st[2] + floor, (n, float(g.norm()), st[2])
    sd = model.state_dict()
    for k in case:
        if k.startswith("buf_"):
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), case[k], rtol=1e-4, atol=1e-5, err_msg=k)
    last = model.visnet_layer.output_model.output_network[1]
    C = last.vec2_proj.weight.shape[0]
    assert float(last.vec2_proj.weight.grad.abs().max()) == 0
    assert float(last.update_net[2].weight.grad[C:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------------
# operator pairs against float64 torch
# ------------------------------------------------------------------------------------------------------------------
def _graph():
    """A crafted batch (see test_hip_visnet._batch): binding truncation, lone atoms, an atom without neighbours."""
    from test_hip_visnet import _batch, _index
    b, _, _ = _batch(21)
    bd = b.to(DEV)
    from equihgnn_amd.visnet import ExpNormalSmearing
    de = ExpNormalSmearing(5.0, 32).to(DEV)
    g = _index(bd).radius(bd.pos, 5.0, 16, de.means, de.betas)
    ei, eid = g.edge_index()
    return g, ei[0].cpu(), ei[1].cpu(), eid.cpu()


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _check(op, ref, inputs, n_out, live_rows):
    """op(*inputs on the GPU, fp32) vs ref(*inputs, float64) forward, and both backward under the same random upstream
    gradients (edge outputs: rows of empty slots carry no meaning and get zero upstream gradient)."""
    x64 = [t.clone().requires_grad_(True) for t in inputs]
    x32 = [t.float().to(DEV).requires_grad_(True) for t in inputs]
    out64 = ref(*x64)
    out32 = op(*x32)
    out64 = out64 if isinstance(out64, tuple) else (out64,)
    out32 = out32 if isinstance(out32, tuple) else (out32,)
    assert len(out64) == len(out32) == n_out
    loss = 0
    loss32 = 0
    for k, (a, b) in enumerate(zip(out64, out32)):
        assert a.shape == b.shape
        up = _rand(*a.shape, seed=100 + k)
        if live_rows is not None and a.shape[0] == live_rows.numel():
            up = up * live_rows.to(up.dtype).view(-1, *([1] * (a.dim() - 1)))
        scale = float(a.detach().abs().max()) + 1e-30
        assert float((b.detach().cpu().double() - a.detach()).abs().max()) <= 2e-5 * scale + 1e-7, ("fwd", k)
        loss = loss + (a * up).sum()
        loss32 = loss32 + (b * up.float().to(DEV)).sum()
    loss.backward()
    loss32.backward()
    for k, (a, b) in enumerate(zip(x64, x32)):
        ga = a.grad if a.grad is not None else torch.zeros_like(a)
        scale = float(ga.abs().max()) + 1e-30
        assert float((b.grad.cpu().double() - ga).abs().max()) <= 2e-5 * scale + 1e-7, ("bwd", k)


# 8: one channel per head, 56 idle lanes; 72: a partial second lane round; 128: ViSNet's default width; 512: all 8 rounds
@pytest.mark.parametrize("C", [64, 256, 8, 72, 128, 320, 512])
def test_operator_pairs_against_float64(C):
    from equihgnn_amd import ops
    g, src, dst, eid = _graph()
    N, E = g.cnt.numel(), g.r.numel()
    cut = g.cut.cpu().double()
    sh = g.sh.cpu().double()
    live = torch.zeros(E, dtype=torch.bool)
    live[eid] = True
    G = visnet_ref.EdgeList(N, src, dst, eid, cut, sh)
    ref = {n: functools.partial(getattr(visnet_ref, n), G) for n in ("nbr_ref", "eemb_ref", "attn_ref", "vec_ref",
                                                                      "eupd_ref")}
    _check(lambda x, W: ops.vis_neighbor_sum(x, W, g), ref["nbr_ref"], [_rand(N, C, seed=1), _rand(E, C, seed=2)], 1,
           live)
    _check(lambda x, W: ops.vis_edge_embed(x, W, g), ref["eemb_ref"], [_rand(N, C, seed=3), _rand(E, C, seed=4)], 1,
           live)
    _check(lambda *t: ops.vis_attn(*t, g), ref["attn_ref"],
           [_rand(N, C, seed=5), _rand(N, C, seed=6), _rand(N, C, seed=7), _rand(E, C, seed=8), _rand(E, C, seed=9)],
           2, live)
    _check(lambda vec, sr: ops.vis_vec_msg(vec, sr, g), ref["vec_ref"],
           [_rand(N, 8, C, seed=10), _rand(E, 2 * C, seed=11)], 1, live)
    _check(lambda *t: ops.vis_edge_update(*t, g), ref["eupd_ref"],
           [_rand(N, 8, C, seed=12), _rand(N, 8, C, seed=13), _rand(E, C, seed=14)], 1, live)
    assert math.isfinite(float(g.rbf.sum()))
