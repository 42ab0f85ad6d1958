"""GPU: ``se3_transformer_equihnns`` against the golden vectors of the reference's own equihnn_se3_transformer.py
(tests/golden/make_golden_se3t.py), its symmetry, and the captured training step.

Bounds.  On the C = 32 fixture the REFERENCE's own float32 run sits this far from its float64 run (CPU, one thread;
stored in the fixture as out / out_f64 and ref_f32_grad_err / ref_f64_grad_max):
    output 6.0e-07, loss 1.2e-07, gradients 1.34e-05 of a parameter's largest entry (worst parameter); tiny case 1.31e-05.
The HIP path is allowed twice that against the float64 values -- but no less than 1e-5 on output and loss -- so
    forward / loss: 1e-5 (absolute below 1, relative above), gradients: 2.7e-5 of the parameter's largest float64 entry;
against the float32 fixture the reference's own error adds: 4.1e-5.  The front-end's output (entries up to 21) is the one
tensor where the reference's float32 run is itself further than 1e-5 from its float64 run: 3.33e-5 by the rule above
(3.81e-5 absolute), read from the two fixtures by the test, so that tap is allowed twice that, 6.7e-5.  No entry is
skipped or masked."""
import copy
import functools

import numpy as np
import pytest
import torch

from common import assert_close, batch_from_case, fill_state_dict, golden_args, load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METHOD = "se3_transformer_equihnns"
REF_GRAD_ERR = 1.34e-5
GRAD_TOL_F64, GRAD_TOL_F32 = 2 * REF_GRAD_ERR, 3 * REF_GRAD_ERR + 1e-6


def _model(seed, hidden=32):
    import equihgnn_amd.models  # noqa: F401
    from equihgnn_amd.registry import create_model
    torch.manual_seed(0)
    model = create_model(METHOD)(1, golden_args(METHOD, hidden))
    fill_state_dict(model, seed)
    return model.to(DEV).train()


def _grad_entries(g):
    from make_golden_se3t import GRAD_FULL_LIMIT, grad_sample_indices
    flat = g.reshape(-1)
    return flat if flat.numel() <= GRAD_FULL_LIMIT else flat[torch.from_numpy(grad_sample_indices(flat.numel()))]


def _run(name):
    case = load_case("se3t/" + name)
    model = _model(int(case["meta_seed"]))
    data = batch_from_case(case).to(DEV)
    taps = {}
    layer = model.se3_transformer_layer
    layer.forward = functools.partial(layer.forward, taps=taps)       # the layer's own taps (conv_in, the two blocks)
    out = model(data, taps=taps)
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    return case, model, out, loss, taps


def _check(case, model, out, loss, grad_tol, ref_out, ref_loss):
    print("out err", np.abs(out.detach().cpu().double().numpy() - ref_out).max(), "loss err", abs(float(loss) - float(ref_loss)))
    params = dict(model.named_parameters())
    worst = ("", 0.0)
    for n, present, st in zip(case["grad_names"], case["grad_present"], case["grad_stats"]):
        g = params[str(n)].grad
        assert (g is not None) == bool(present), n
        want = case["grad_" + str(n)].astype(np.float64)
        got = _grad_entries(g.detach().cpu().double()).numpy()
        rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, (str(n), float(rel)), key=lambda t: t[1])
    print("worst gradient", worst)
    assert_close(out.detach().cpu().numpy(), ref_out, 1e-5, "out")
    assert_close(float(loss.detach()), float(ref_loss), 1e-5, "loss")
    for n, present, st in zip(case["grad_names"], case["grad_present"], case["grad_stats"]):
        g = params[str(n)].grad.detach().cpu().double()
        want = case["grad_" + str(n)].astype(np.float64)
        got = _grad_entries(g).numpy()
        assert np.abs(got - want).max() <= grad_tol * np.abs(want).max(), (n, np.abs(got - want).max() / np.abs(want).max())
        assert abs(float(g.norm()) - st[2]) <= grad_tol * st[2] * 4, (n, float(g.norm()), st[2])


def test_matches_the_float64_reference():
    case, model, out, loss, taps = _run("se3_transformer_equihnns_c32_f64")
    for k in ("conv_in0", "conv_in1", "block0_0", "block0_1", "block1_0", "block1_1"):
        got = taps[k].detach().transpose(1, 2).cpu().numpy()
        ref = case["tap_" + k]
        print(k, np.abs(got - ref).max(), np.abs(ref).max())
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k
    # the reference's own float32 error on this tap, by assert_close's rule, from its two runs of the same fixture
    want, ref32 = case["tap_front_end"], load_case("se3t/se3_transformer_equihnns_c32")["tap_front_end"]
    ref_err = float((np.abs(ref32 - want) / np.maximum(1.0, np.abs(want))).max())
    print("front_end: reference float32 error", ref_err)
    assert_close(taps["front_end"].detach().cpu().numpy(), want, max(1e-5, 2 * ref_err), "front_end")
    _check(case, model, out, loss, GRAD_TOL_F64, case["out"], case["loss"])


def test_matches_the_float32_reference():
    case, model, out, loss, _ = _run("se3_transformer_equihnns_c32")
    _check(case, model, out, loss, GRAD_TOL_F32, case["out"], case["loss"])
    assert_close(out.detach().cpu().numpy(), case["out_f64"], 1e-5, "out vs float64")


def test_tiny_cloud():
    """N = 5: k = 4 < 16."""
    case, model, out, loss, _ = _run("se3_transformer_equihnns_tiny")
    _check(case, model, out, loss, GRAD_TOL_F32, case["out"], case["loss"])
    assert_close(out.detach().cpu().numpy(), case["out_f64"], 1e-5, "out vs float64")


def test_invariant_under_rotation_and_translation():
    case = load_case("se3t/se3_transformer_equihnns_c32")
    model = _model(int(case["meta_seed"])).eval()
    data = batch_from_case(case).to(DEV)
    with torch.no_grad():
        base = model(data).cpu().double()
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64))
        q = q * torch.sign(torch.linalg.det(q))
        moved = batch_from_case(case)
        moved.pos = (moved.pos.double() @ q.T + torch.tensor([0.7, -1.1, 0.4], dtype=torch.float64)).float()
        got = model(moved.to(DEV)).cpu().double()
    # the rotated coordinates are rounded to float32 again (1e-7 of |pos| ~ 30 at the far atom): the same 1e-5 rule
    assert_close(got.numpy(), base.numpy(), 1e-5, "rotated")


def test_graphed_step_equals_the_eager_step():
    from equihgnn_amd.batch import pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep, TrainStep
    m1 = _model(7)
    m2 = copy.deepcopy(m1)
    # the captured step takes the batch padded to its bucket and leaves the dummy molecule out of the loss; TrainStep averages
    # over every molecule it is given, so it gets the same batches unpadded (as tests/test_trajectory.py does)
    raw = [synth_batch(6, 900 + i) for i in range(3)]
    tr1, tr2 = GraphedTrainStep(m1, lr=1e-3), TrainStep(m2, lr=1e-3)
    l1 = [float(tr1.step(pad_batch(b, 256, 320, 800).to(DEV))) for b in raw]
    l2 = [float(tr2.step(b.to(DEV))) for b in raw]
    print(l1, l2)
    for a, b in zip(l1, l2):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (l1, l2)
