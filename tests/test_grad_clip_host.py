"""Gradient clipping by global norm, host side (no GPU): ``TrainStep(clip_gnorm=c)`` against a hand-written
backward / ``torch.nn.utils.clip_grad_norm_`` / Adam loop, the two history columns ``Fitter(clip_gnorm=c)`` adds (and the
unchanged rows without it), two gloo ranks clipping the AVERAGED gradient, and the argument checks of the native entry
points (eqh_grad_sumsq, eqh_adam_step_clip), which return before anything is launched."""
import ctypes
import math
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from equihgnn_amd.trainer import TrainStep


class _Net(torch.nn.Module):
    """the plugin contract ``model(data) -> Tensor[B]`` on three parameter tensors and a bias-free layer"""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 1, bias=False)

    def forward(self, data):
        return self.b(torch.tanh(self.a(data.x))).squeeze(-1)


def _data(seed, n=9):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(x=torch.randn(n, 5, generator=g), y=3.0 * torch.randn(n, generator=g))


def _grads(model, data):
    for p in model.parameters():
        p.grad = None
    loss = torch.nn.functional.mse_loss(model(data), data.y)
    loss.backward()
    return loss


def test_train_step_clip_equals_clip_grad_norm_then_adam():
    """T7: three steps, weight decay on; the threshold is half the first step's norm, so the clip is active (checked from the
    readout, whose four entries are checked against the hand-written loop's norms)."""
    batches = [_data(40 + t) for t in range(3)]
    probe = _Net(3)
    _grads(probe, batches[0])
    c = 0.5 * float(torch.nn.utils.get_total_norm([p.grad for p in probe.parameters()]))
    mine, ref = _Net(3), _Net(3)
    tr = TrainStep(mine, lr=1e-2, weight_decay=0.1, clip_gnorm=c)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=0.1)
    norms = []
    for data in batches:
        loss = tr.step(data)
        ref_loss = _grads(ref, data)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), c)))
        opt.step()
        assert float(loss) == float(ref_loss.detach())
        for (k, p), q in zip(mine.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), k
    total, coef, seen, clipped = tr.grad_norm.tolist()
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert total == norms[-1] and seen == max(norms)
    assert clipped == sum(1 for v in norms if c / (v + 1e-6) < 1.0) >= 1
    assert math.isclose(coef, min(1.0, f32(c) / (norms[-1] + 1e-6)), rel_tol=1e-6)
    # off by default: no readout, and the step is the unclipped one
    plain, ref2 = _Net(3), _Net(3)
    tr2 = TrainStep(plain, lr=1e-2)
    opt2 = torch.optim.Adam(ref2.parameters(), lr=1e-2)
    for data in batches:
        tr2.step(data)
        _grads(ref2, data)
        opt2.step()
    assert tr2.grad_norm is None and tr2.clip_gnorm is None
    assert all(torch.equal(p, q) for p, q in zip(plain.parameters(), ref2.parameters()))
    assert not all(torch.equal(p, q) for p, q in zip(plain.parameters(), mine.parameters()))


BASE_KEYS = ["epoch", "train_loss", "lr", "val_mae_mean", "val_mae_std", "val_mse_mean", "val_mse_std"]


def test_fitter_reports_the_readout_once_per_epoch_and_only_when_clipping():
    from equihgnn_amd.fit import Fitter
    train, valid = [_data(60 + t) for t in range(4)], [_data(70)]
    # without the keyword: today's rows, also through a factory that does not know it
    seen_kw = []

    def old_factory(model, lr, weight_decay):
        seen_kw.append((lr, weight_decay))
        return TrainStep(model, lr=lr, weight_decay=weight_decay)
    for factory in (TrainStep, old_factory):
        res = Fitter(_Net(4), lr=1e-2, step_factory=factory).fit(train, valid, epochs=2)
        assert [list(row) for row in res.history] == [BASE_KEYS, BASE_KEYS]
    assert seen_kw == [(1e-2, 0.0)]
    # with it: two more columns per epoch, the running pair restarted after each read
    fitter = Fitter(_Net(4), lr=1e-2, clip_gnorm=1e-3)          # far below any of these gradients: every step is clipped
    reads = []
    real = fitter.step._clip

    def clip():
        real()
        reads.append(fitter.step.grad_norm[0].item())
    fitter.step._clip = clip
    res = fitter.fit(train, valid, epochs=2)
    assert [list(row) for row in res.history] == [BASE_KEYS + ["grad_norm_max", "clipped_steps"]] * 2
    assert len(reads) == 8
    for e, row in enumerate(res.history):
        assert row["clipped_steps"] == 4 and isinstance(row["clipped_steps"], int)
        assert row["grad_norm_max"] == max(reads[4 * e:4 * e + 4])
    assert fitter.step.grad_norm[2:].tolist() == [0.0, 0.0]
    # ... and the clipped fit is a different fit
    plain = Fitter(_Net(4), lr=1e-2).fit(train, valid, epochs=2)
    assert plain.history[-1]["train_loss"] != res.history[-1]["train_loss"]


# ---- T8: two gloo ranks ----------------------------------------------------------------------------------------------------
CLIP = 0.05


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _Net(100 + rank)                 # different init per rank: the broadcast fixes that
    tr = TrainStep(model, lr=1e-2, clip_gnorm=CLIP)
    for step in range(3):
        tr.step(_data(500 + 10 * step + rank))
    torch.save({"sd": {k: v.clone() for k, v in model.state_dict().items()}, "readout": tr.grad_norm.clone()},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_clip_the_averaged_gradient(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for k in r0["sd"]:
        assert torch.equal(r0["sd"][k], r1["sd"][k]), f"{k} differs across ranks"
    assert torch.equal(r0["readout"], r1["readout"])
    # single process: rank 0's init, Adam on the mean of the two ranks' gradients clipped by torch.  The sum of two numbers
    # does not depend on their order and halving is exact, so the all-reduced mean IS (g0 + g1) * 0.5: equality, not closeness
    # (products this small run on one thread whatever the pool's size, so the two processes' arithmetic is the same).
    model = _Net(100)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    norms, own = [], []
    for step in range(3):
        grads = []
        for rank in range(world):
            _grads(model, _data(500 + 10 * step + rank))
            grads.append([p.grad.clone() for p in model.parameters()])
        own.append([float(torch.nn.utils.get_total_norm(g)) for g in grads])
        for p, g0, g1 in zip(model.parameters(), *grads):
            p.grad = (g0 + g1) * 0.5
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)))
        opt.step()
    for k, v in model.state_dict().items():
        assert torch.equal(r0["sd"][k], v), k
    total, coef, seen, clipped = r0["readout"].tolist()
    assert total == norms[-1] and seen == max(norms) and clipped == 3 and coef < 1.0
    assert total not in own[-1] and total < max(own[-1])        # the norm of the average, not of a rank's own gradient


# ---- T9: header, library, argument checks ----------------------------------------------------------------------------------
def test_native_entry_points_are_bound_and_check_their_arguments():
    from equihgnn_amd import hip
    L = hip.lib()
    for name in ("eqh_grad_sumsq_workspace_bytes", "eqh_grad_sumsq", "eqh_adam_step_clip"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    assert L.eqh_grad_sumsq_workspace_bytes.restype is ctypes.c_size_t
    assert len(hip.SIGNATURES["eqh_adam_step_clip"][1]) == len(hip.SIGNATURES["eqh_adam_step"][1]) + 3
    # one double per workgroup of a grid that is capped at 256
    size = L.eqh_grad_sumsq_workspace_bytes
    assert size(-1) == 0 and size(0) == 8 and size(3) == 8 and size(70003) == 8 * 18
    assert size(2 ** 20 + 16 * 256 + 3) == 8 * 256 == size(2 ** 33)
    held = ctypes.create_string_buffer(256)          # addresses that are never read: no call below gets as far as a launch
    ok = (ctypes.addressof(held) + 15) // 16 * 16

    def clip(partials=ok, max_norm=5.0, readout=ok, n=4, grad=ok):
        return L.eqh_adam_step_clip(ok, grad, ok, ok, n, ok, 0.9, 0.999, 1e-8, 0.0, 1.0, ok, 0, None, 0,
                                    partials, max_norm, readout, None)
    assert clip(partials=None) == hip.EQH_ERR_ARG
    assert clip(readout=None) == hip.EQH_ERR_ARG
    for bad in (0.0, -5.0, float("nan")):
        assert clip(max_norm=bad) == hip.EQH_ERR_ARG, bad
    assert clip(partials=None, n=0) == hip.EQH_ERR_ARG           # (checked ahead of the empty-tensor return)
    assert clip(n=-1) == hip.EQH_ERR_ARG and clip(grad=None) == hip.EQH_ERR_ARG
    assert clip(partials=ok + 4) == hip.EQH_ERR_ALIGN
    assert clip(readout=ok + 4) == hip.EQH_ERR_ALIGN
    assert clip(grad=ok + 4) == hip.EQH_ERR_ALIGN
    assert clip(n=0) == hip.EQH_OK                               # nothing to update, nothing launched
    assert L.eqh_grad_sumsq(ok, 4, None, None) == hip.EQH_ERR_ARG
    assert L.eqh_grad_sumsq(None, 4, ok, None) == hip.EQH_ERR_ARG
    assert L.eqh_grad_sumsq(ok, -1, ok, None) == hip.EQH_ERR_ARG
    assert L.eqh_grad_sumsq(ok, 4, ok + 4, None) == hip.EQH_ERR_ALIGN
    assert L.eqh_grad_sumsq(ok + 4, 4, ok, None) == hip.EQH_ERR_ALIGN
    # the unclipped entry point keeps its checks
    assert L.eqh_adam_step(ok, ok, ok, ok, 4, None, 0.9, 0.999, 1e-8, 0.0, 1.0, ok, 0, None, 0, None) == hip.EQH_ERR_ARG


def test_flat_adam_refuses_a_threshold_that_is_not_positive():
    import pytest

    from equihgnn_amd.trainer import FlatAdam
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm must be positive"):
            FlatAdam(torch.nn.Parameter(torch.zeros(8)), max_grad_norm=bad)
