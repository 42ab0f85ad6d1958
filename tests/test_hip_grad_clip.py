"""Gradient clipping by global norm inside the optimiser step (csrc/optim.hip: eqh_grad_sumsq + eqh_adam_step_clip,
``trainer.FlatAdam(max_grad_norm=..)``, ``trainer.GraphedTrainStep(clip_gnorm=..)``) against
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` on the device.

Tolerances.  Parameters: those of test_flat_adam_matches_torch_adam, rtol 2e-6 / atol 2e-7 -- the clip perturbs the scaled
gradient by ~1e-7 relative (one rounding of coef, one of the product), and Adam's ratio m / sqrt(v) is scale-invariant, so the
perturbation lands far inside atol.  The norm readout: rtol 1e-6 against the float64 norm (double accumulation, then one fp32
rounding of the result)."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from golden.common import fill_state_dict, golden_args, trajectory_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, MARK = 64, 7.25
RTOL, ATOL = 2e-6, 2e-7


def _count(monkeypatch, *names):
    from equihgnn_amd import hip
    lib, calls = hip.lib(), {n: 0 for n in names}
    for n in names:
        def counted(*a, _n=n, _inner=getattr(lib, n)):
            calls[_n] += 1
            return _inner(*a)
        monkeypatch.setattr(lib, n, counted, raising=True)
    return calls


def _guarded(n, dtype=torch.float32, guard=GUARD):
    """a buffer of n elements with ``guard`` marked elements behind it: (the whole allocation, its head)"""
    buf = torch.full((n + guard,), MARK, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _clipped_pair(n, w0, max_norm, **kw):
    """FlatAdam(max_grad_norm) whose six device buffers (parameter, gradient, both moments, partials, readout) each have
    guard floats behind them, and the list of whole allocations"""
    from equihgnn_amd.trainer import FlatAdam
    whole, heads = zip(*[_guarded(n) for _ in range(4)])
    heads[0].copy_(w0)
    heads[2].zero_()
    heads[3].zero_()
    p1 = torch.nn.Parameter(heads[0])
    p1.grad = heads[1]
    o1 = FlatAdam(p1, max_grad_norm=max_norm, **kw)
    st = o1.state[p1]
    st["exp_avg"], st["exp_avg_sq"] = heads[2], heads[3]
    part_whole, part = _guarded(st["clip_partials"].numel(), torch.float64, GUARD // 2)
    read_whole, read = _guarded(4)
    read.zero_()
    st["clip_partials"], o1.grad_norm = part, read
    return p1, o1, list(whole) + [part_whole, read_whole]


def _assert_close(a, b, what):
    over = (a.detach() - b.detach()).abs() - (ATOL + RTOL * b.detach().abs())
    assert float(over.max()) <= 0.0, (what, float(over.max()), int(over.argmax()))


@pytest.mark.parametrize("n", [3, 70003, 2 ** 20 + 16 * 256 + 3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_flat_adam_clip_matches_clip_grad_norm_then_adam(n, grad_scale, monkeypatch):
    """T1 (grad_scale 1) and T3 (grad_scale 0.25: torch gets 0.25 g, the readout is the norm of 0.25 g).  n = 3: the ragged
    tail alone; 70003; 2^20 + 16 x 256 + 3: workgroup 0 of the capped sum-of-squares grid takes a second trip, a ragged
    quad and the tail.  The threshold is half the first step's norm and the gradients grow, so coef < 1 at every step.  Before
    step 2 the partials workspace is filled with NaN (every slot is rewritten by every launch)."""
    gen = torch.Generator(device=DEV).manual_seed(2 + n % 7)
    w0 = torch.randn(n, generator=gen, device=DEV)
    grads = [torch.randn(n, generator=gen, device=DEV) * (0.5 + t) for t in range(5)]
    c = 0.5 * float(torch.linalg.vector_norm((grad_scale * grads[0]).double()))
    p1, o1, whole = _clipped_pair(n, w0, c, lr=1e-2, weight_decay=0.1)
    o1.grad_scale = grad_scale
    p2 = torch.nn.Parameter(w0.clone())
    o2 = torch.optim.Adam([p2], lr=1e-2, weight_decay=0.1)
    calls = _count(monkeypatch, "eqh_adam_step", "eqh_grad_sumsq", "eqh_adam_step_clip")
    seen = 0.0
    for t, gr in enumerate(grads):
        p1.grad.copy_(gr)
        p2.grad = grad_scale * gr
        if t == 2:
            o1.state[p1]["clip_partials"].fill_(float("nan"))
        o1.sync_lr()
        o1.step()
        torch.nn.utils.clip_grad_norm_([p2], c)
        o2.step()
        assert bool(torch.isfinite(p1.detach()).all())
        _assert_close(p1, p2, ("param", t))
        total, coef, running, clipped = o1.grad_norm.tolist()
        want = float(torch.linalg.vector_norm((grad_scale * gr).double()))
        assert abs(total - want) <= 1e-6 * want, (t, total, want)
        assert coef < 1.0 and abs(coef - c / (want + 1e-6)) <= 1e-6 * coef, (t, coef)
        seen = max(seen, total)
        assert running == seen and clipped == t + 1
        assert torch.equal(p1.grad, gr)                  # zero_grad_in_step is off: the gradient is read, not scaled in place
    assert calls == {"eqh_adam_step": 0, "eqh_grad_sumsq": 5, "eqh_adam_step_clip": 5}
    assert o1.state[p1]["step_block"].tolist() == [5, 0]
    for buf, head in zip(whole, (n, n, n, n, o1.state[p1]["clip_partials"].numel(), 4)):
        assert bool((buf[head:] == MARK).all())


def test_flat_adam_clip_with_an_unreachable_threshold_is_the_plain_step(monkeypatch):
    """T2: max_grad_norm = 1e30 makes coef exactly 1: parameters and both moments equal the unclipped optimiser's bit for bit;
    the clipped optimiser never calls eqh_adam_step, the plain one makes exactly that one call per step."""
    from equihgnn_amd.trainer import FlatAdam
    n = 70003
    gen = torch.Generator(device=DEV).manual_seed(5)
    w0 = torch.randn(n, generator=gen, device=DEV)
    grads = [torch.randn(n, generator=gen, device=DEV) * (0.5 + t) for t in range(3)]
    p1, p2 = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone())
    o1 = FlatAdam(p1, lr=1e-2, weight_decay=0.1, max_grad_norm=1e30)
    o2 = FlatAdam(p2, lr=1e-2, weight_decay=0.1)
    assert o2.grad_norm is None and o2.max_grad_norm is None
    calls = _count(monkeypatch, "eqh_adam_step", "eqh_grad_sumsq", "eqh_adam_step_clip")
    for gr in grads:
        p1.grad = gr.clone()
        o1.step()
    assert calls == {"eqh_adam_step": 0, "eqh_grad_sumsq": 3, "eqh_adam_step_clip": 3}
    for gr in grads:
        p2.grad = gr.clone()
        o2.step()
    assert calls == {"eqh_adam_step": 3, "eqh_grad_sumsq": 3, "eqh_adam_step_clip": 3}
    assert torch.equal(p1, p2)
    for k in ("exp_avg", "exp_avg_sq", "step_block"):
        assert torch.equal(o1.state[p1][k], o2.state[p2][k]), k
    total, coef, running, clipped = o1.grad_norm.tolist()
    assert coef == 1.0 and clipped == 0.0 and running >= total > 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_flat_adam_clip_on_a_non_finite_gradient_is_torchs(bad):
    """T4: error_if_nonfinite = False.  One inf entry: the norm is inf, coef 0, that entry's 0 * inf a NaN, every other
    parameter moves by its weight decay alone; one NaN entry: coef is NaN (the clamp keeps it) and so is every parameter."""
    n = 70003
    gen = torch.Generator(device=DEV).manual_seed(9)
    w0 = torch.randn(n, generator=gen, device=DEV)
    gr = torch.randn(n, generator=gen, device=DEV)
    gr[4321] = bad
    p1, o1, whole = _clipped_pair(n, w0, 1.0, lr=1e-2, weight_decay=0.1)
    p2 = torch.nn.Parameter(w0.clone())
    o2 = torch.optim.Adam([p2], lr=1e-2, weight_decay=0.1)
    p1.grad.copy_(gr)
    p2.grad = gr.clone()
    o1.step()
    torch.nn.utils.clip_grad_norm_([p2], 1.0)
    o2.step()
    a, b = p1.detach(), p2.detach()
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    assert int(torch.isnan(b).sum()) == (1 if bad == float("inf") else n)
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=RTOL, atol=ATOL, equal_nan=True)
    fin = torch.isfinite(b)
    if bool(fin.any()):
        _assert_close(a[fin], b[fin], "finite parameters")
    total, coef, running, clipped = o1.grad_norm.tolist()
    if bad == float("inf"):
        assert total == float("inf") and coef == 0.0 and clipped == 1.0
    else:
        assert total != total and coef != coef
    for buf, head in zip(whole, (n, n, n, n, o1.state[p1]["clip_partials"].numel(), 4)):
        assert bool((buf[head:] == MARK).all())


# ---- in the captured step --------------------------------------------------------------------------------------------------
NAME, HIDDEN, SEED, LR = "trajectory_egnn_equihnns_c64_b", 64, 107, 1e-3


def _model_and_batches(dev):
    from equihgnn_amd.batch import bucket_sizes, pad_batch
    from equihgnn_amd.models import MODELS
    model = MODELS["egnn_equihnns"](1, golden_args("egnn_equihnns", HIDDEN))
    fill_state_dict(model, SEED)
    model.to(dev).train()
    raw = trajectory_batches(NAME)
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz, 64) for b in raw]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    return model, [pad_batch(b, *tgt).to(dev) for b in raw]


def _initial_flat(tr, dev):
    """the trainer's flat parameter buffer as it was before step 0: a fresh model with the same fill, laid out as ``pflat``
    (the padding between slots is zero and stays zero: zero gradient, zero moments)"""
    fresh, _ = _model_and_batches(dev)
    init = torch.zeros_like(tr.pflat.detach())
    base, size = tr.pflat.data_ptr(), tr.pflat.numel() * 4
    start = dict(fresh.named_parameters())
    placed = 0
    for name, p in tr.model.named_parameters():
        off = p.data_ptr() - base
        if 0 <= off < size:
            init[off // 4:off // 4 + p.numel()] = start[name].detach().reshape(-1)
            placed += 1
    assert placed == len(tr.live)
    return init


def _graphed_clip_run(dev, **kw):
    """T5: four steps (one eager bootstrap, three replays of ONE graph) of GraphedTrainStep(clip_gnorm = c) against a mirror
    torch Adam fed the step's own gflat, clipped by torch; coef < 1 at every step, from the readout.

    The threshold: half the SMALLEST norm an unclipped trainer reports over the same four steps.  Half the norm of step 0
    alone cannot keep the clip active on this trajectory: the reference model's own unclipped gradient norms (CPU oracle,
    fp32) are 25.97, 11.58, 10.36, 3.71 -- step 1 is already below 12.98, so torch's own coef is 1 from there on.  Adam's
    update is invariant to the gradient's scale (up to eps), so the clipped run sees nearly the same norms."""
    from equihgnn_amd.trainer import GraphedTrainStep
    model, batches = _model_and_batches(dev)
    probe = GraphedTrainStep(model, lr=LR, keep_grads=True, **kw)
    norms = []
    for t in range(4):
        probe.step(batches[t % 3])
        norms.append(float(torch.linalg.vector_norm(probe.gflat.double())) * (probe.opt.grad_scale if probe.opt else 1.0))
    assert probe.grad_norm is None
    print("unclipped gradient norms:", norms)
    c = 0.5 * min(norms)
    probe.close()
    model, batches = _model_and_batches(dev)
    tr = GraphedTrainStep(model, lr=LR, keep_grads=True, clip_gnorm=c, **kw)
    mirror, opt, coefs = None, None, []
    for t in range(4):
        tr.step(batches[t % 3])
        if mirror is None:
            mirror = torch.nn.Parameter(_initial_flat(tr, dev))
            opt = torch.optim.Adam([mirror], lr=LR)
        mirror.grad = tr.gflat.detach().clone() * tr.opt.grad_scale
        want = float(torch.linalg.vector_norm(mirror.grad.double()))
        torch.nn.utils.clip_grad_norm_([mirror], c)
        opt.step()
        _assert_close(tr.pflat, mirror, ("pflat", t))
        total, coef, running, clipped = tr.grad_norm.tolist()
        print("step", t, "norm", total, "float64 norm", want, "coef", coef, "clipped steps", clipped)
        assert abs(total - want) <= 1e-6 * want, (t, total, want)
        assert coef < 1.0 and abs(coef - c / (want + 1e-6)) <= 1e-6 * coef and clipped == t + 1, (t, coef, clipped)
        coefs.append(coef)
    assert len(tr.slots) == 1
    mode, err = tr.collective_mode, tr.capture_error
    tr.close()
    return {"mode": mode, "capture_error": err, "coefs": coefs, "clip": c}


def test_graphed_step_clips_inside_the_captured_graph():
    rep = _graphed_clip_run(torch.device(DEV))
    assert rep["mode"] == "none"


def _rccl_worker(rank, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    rep = _graphed_clip_run(dev, force_collective=True)
    rep["split"] = _graphed_clip_run(dev, force_collective=True, graph_collective=False)     # both launches in g_opt
    torch.cuda.synchronize()
    json.dump(rep, open(out_path, "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_graphed_step_clips_behind_the_captured_all_reduce(tmp_path):
    """T5 under a one-rank RCCL group with force_collective: sum-of-squares pass and update sit behind the all-reduce node;
    and once more with the collective kept out of the graph ("split": both launches in the second graph, same numbers)."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "report.json"
    mp.spawn(_rccl_worker, args=(port, str(out)), nprocs=1, join=True)      # RCCL lives and dies in a child process
    rep = json.load(open(out))
    print("clip behind the all-reduce:", json.dumps(rep))
    assert rep["mode"] == "in_graph" or (rep["mode"] == "split" and rep["capture_error"]), rep
    assert all(cf < 1.0 for cf in rep["coefs"])
    assert rep["split"]["mode"] == "split" and rep["split"]["coefs"] == rep["coefs"]


def test_graphed_step_with_an_unreachable_threshold_is_the_unclipped_step():
    """T6: clip_gnorm = 1e30 against None, both graphed, three steps on the same model and batches: every parameter equal."""
    from equihgnn_amd.trainer import GraphedTrainStep
    finals = {}
    for label, clip in (("none", None), ("huge", 1e30)):
        model, batches = _model_and_batches(torch.device(DEV))
        tr = GraphedTrainStep(model, lr=LR, clip_gnorm=clip)
        losses = [float(tr.step(batches[t])) for t in range(3)]
        torch.cuda.synchronize()
        finals[label] = ({k: v.detach().clone() for k, v in model.named_parameters()}, losses)
        if clip is None:
            assert tr.grad_norm is None
        else:
            total, coef, running, clipped = tr.grad_norm.tolist()
            assert coef == 1.0 and clipped == 0.0 and running >= total > 0.0
        assert len(tr.slots) == 1
        tr.close()
    assert finals["none"][1] == finals["huge"][1]
    for k, v in finals["none"][0].items():
        assert torch.equal(v, finals["huge"][0][k]), k
