"""Gradient accumulation inside the captured step (``GraphedTrainStep(accum_steps=k)``, csrc/optim.hip: eqh_add_many) on the
device: the adding launch alone against torch's add, the sum a group leaves in ``gflat`` against the gradients of a k = 1
trainer on the same weights, a bucket first captured in the middle of a group, the one update per group against a mirror
``torch.optim.Adam`` fed the step's own gradient (test_hip_grad_clip.py's method, insensitive to summation order),
``flush()``, k = 1 against no keyword, and the one collective per group under a one-rank RCCL group.

Tolerances.  The sum: max |gflat - (g_a + g_b)| <= 1e-5 max |g_a + g_b| per parameter tensor -- the faults looked for (a
double-counted scratch, a slot copied over instead of added to, a micro-batch wiped by a capture) are of order one, fp32
re-association of order 1e-7.  The update: rtol 2e-6 / atol 2e-7, test_hip_grad_clip.py's."""
import json
import os
import socket

import pytest
import torch

from golden.common import fill_state_dict, golden_args, trajectory_batches
from test_hip_grad_clip import _assert_close, _count

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, MARK = 64, 7.25
LR = 1e-3
TRAJECTORY = {"egnn_equihnns": ("trajectory_egnn_equihnns_c64_b", 107), "mhnnm": ("trajectory_mhnnm_c64", 85)}


# ---- 1. the launch alone ---------------------------------------------------------------------------------------------------
def _between_guards(n, fill=None):
    """n floats with GUARD marked floats on either side: (the whole allocation, the n floats); 16-byte aligned"""
    whole = torch.full((n + 2 * GUARD,), MARK, dtype=torch.float32, device=DEV)
    mid = whole[GUARD:GUARD + n]
    if fill is not None:
        mid.copy_(fill)
    return whole, mid


def _guards_intact(whole, n):
    return bool((whole[:GUARD] == MARK).all()) and bool((whole[GUARD + n:] == MARK).all())


@pytest.mark.parametrize("zero_n", [0, 4096])
def test_add_many_adds_every_entry_and_clears_the_second_buffer(zero_n, monkeypatch):
    """Lengths 1, 3, 4, 5, 1023, 4097 (quad body, ragged tail, several workgroup rows), one source one float off 16-byte
    alignment (the scalar path), and 65 entries in all -- one more than a launch holds.  One fp32 add per element: the result
    IS torch's dst + src.  Guards on both sides of every destination and of the cleared range."""
    from equihgnn_amd import ops
    g = torch.Generator().manual_seed(5)
    lengths = [1, 3, 4, 5, 1023, 4097, 37] + [1 + (7 * i) % 29 for i in range(58)]
    assert len(lengths) == 65
    wholes, dsts, srcs, want = [], [], [], []
    for i, n in enumerate(lengths):
        whole, d = _between_guards(n, torch.randn(n, generator=g))
        s = torch.randn(n + 1, generator=g).to(DEV)
        s = s[1:] if i == 6 else s[:n]
        assert (s.data_ptr() % 16 == 4) == (i == 6) and d.data_ptr() % 16 == 0
        wholes.append(whole)
        dsts.append(d)
        srcs.append(s)
        want.append(d + s)
    zwhole, zbuf = _between_guards(zero_n, torch.randn(zero_n, generator=g)) if zero_n else (None, None)
    calls = _count(monkeypatch, "eqh_add_many", "eqh_copy_many")
    ops.add_many(dsts, srcs, zero_also=zbuf)
    torch.cuda.synchronize()
    assert calls == {"eqh_add_many": 1, "eqh_copy_many": 0}
    for i, n in enumerate(lengths):
        assert torch.equal(dsts[i], want[i]), (i, n)
        assert _guards_intact(wholes[i], n), (i, n)
    if zero_n:
        assert bool((zbuf == 0).all()) and _guards_intact(zwhole, zero_n)
        # ... and with nothing to add the launch still clears
        zbuf.fill_(3.0)
        ops.add_many([], [], zero_also=zbuf)
        torch.cuda.synchronize()
        assert bool((zbuf == 0).all()) and _guards_intact(zwhole, zero_n)


# ---- models and batches ----------------------------------------------------------------------------------------------------
def _build(kind, big=()):
    """(a fresh seeded model on the device, its three padded batches); ``big``: indices of the batches padded to a larger
    bucket than the others"""
    if kind == "gin":
        from equihgnn_amd.baseline_2d import GNN_2D
        from equihgnn_amd.batch import pad_graph_batch, synth_graph_batch
        model = GNN_2D(1, num_layer=3, emb_dim=64, gnn_type="gin")
        fill_state_dict(model, 3)
        model.to(DEV).train()
        return model, [pad_graph_batch(synth_graph_batch(8, 300 + i, "pcqm"), *((512, 1024) if i in big else (384, 768))).to(DEV)
                       for i in range(3)]
    from equihgnn_amd.batch import bucket_sizes, pad_batch
    from equihgnn_amd.models import MODELS
    name, seed = TRAJECTORY[kind]
    model = MODELS[kind](1, golden_args(kind, 64))
    fill_state_dict(model, seed)
    model.to(DEV).train()
    raw = trajectory_batches(name)
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz, 64) for b in raw]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    return model, [pad_batch(b, *(tuple(2 * x for x in tgt) if i in big else tgt)).to(DEV) for i, b in enumerate(raw)]


def _by_name(tr, flat):
    """{parameter name: its slice of a flat buffer laid out as the trainer's pflat / gflat}"""
    base, out = tr.pflat.data_ptr(), {}
    for name, p in tr.model.named_parameters():
        off = (p.data_ptr() - base) // 4
        if 0 <= off < tr.pflat.numel():
            out[name] = flat[off:off + p.numel()].clone()
    assert len(out) == len(tr.live)
    return out


def _reference_grads(kind, big, order):
    """g of every batch index in ``order`` from a k = 1 trainer with keep_grads and lr = 0 (the weights stay put), walked
    through ``order`` twice so that the second round's gradients come from replays"""
    from equihgnn_amd.trainer import GraphedTrainStep
    model, batches = _build(kind, big)
    tr = GraphedTrainStep(model, lr=0.0, keep_grads=True)
    grads = {}
    for i in list(order) + list(order):
        tr.step(batches[i])
        grads[i] = _by_name(tr, tr.gflat.detach())
    tr.close()
    return grads


def _check_sum(kind, big):
    from equihgnn_amd.trainer import GraphedTrainStep
    ref = _reference_grads(kind, big, (0, 1))
    model, batches = _build(kind, big)
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    tr = GraphedTrainStep(model, lr=0.0, keep_grads=True, accum_steps=2)
    worst = 0.0
    for group in range(3):      # group 0: eager bootstrap + capture; group 1: a's bucket captured (big) or replays; group 2: replays
        tr.step(batches[0])
        assert tr.micro == 1
        tr.step(batches[1])
        assert tr.micro == 0 and tr.updates == group + 1
        got = _by_name(tr, tr.gflat.detach())
        assert sorted(got) == sorted(ref[0])
        for name, g in got.items():
            want = ref[0][name] + ref[1][name]
            err, scale = float((g - want).abs().max()), float(want.abs().max())
            worst = max(worst, err / max(scale, 1e-30))
            assert err <= 1e-5 * scale, (kind, group, name, err, scale)
    print(f"{kind} big={big}: max |gflat - (g_a + g_b)| / max |g_a + g_b| over tensors and groups = {worst:.3e}")
    assert len(tr.slots) == (2 if big else 1)
    for n, p in model.named_parameters():       # lr = 0
        assert torch.equal(p, start[n]), n
    tr.close()


@pytest.mark.parametrize("kind", ["egnn_equihnns", "mhnnm", "gin"])
def test_a_group_leaves_the_sum_of_its_micro_batches_gradients(kind):
    """2: S tail with the conv stack, merged-weight scratch with BatchNorm, gradients almost all autograd-allocated."""
    _check_sum(kind, ())


@pytest.mark.parametrize("kind", ["egnn_equihnns", "mhnnm", "gin"])
def test_a_bucket_first_met_in_the_middle_of_a_group_keeps_the_groups_gradient(kind):
    """3: micro-batch b padded to a larger bucket than a: b's capture (warm-up passes, which clear and overwrite gflat)
    happens at micro-step 2 of the first group, a's at micro-step 1 of the second."""
    _check_sum(kind, (1,))


def test_keep_grads_off_gives_the_same_update_as_keep_grads_on():
    """The scratch-clearing side of the adding launch runs only without keep_grads (with it the merged accumulators are a
    fresh slab per pass), and then the update clears gflat: two groups of mhnnm, parameters equal bit for bit."""
    from equihgnn_amd.trainer import GraphedTrainStep
    finals = []
    for keep in (True, False):
        model, batches = _build("mhnnm")
        tr = GraphedTrainStep(model, lr=LR, keep_grads=keep, accum_steps=2)
        for t in range(6):
            tr.step(batches[t % 3])
        torch.cuda.synchronize()
        assert tr.updates == 3
        if not keep:
            assert not bool(tr.gflat.any()) and (tr.scratch.buf is None or not bool(tr.scratch.buf.any()))
        finals.append(tr.pflat.detach().clone())
        tr.close()
    assert torch.equal(finals[0], finals[1])


# ---- 4, 5. the update ------------------------------------------------------------------------------------------------------
def _initial_flat(tr):
    fresh, _ = _build("egnn_equihnns")
    init = torch.zeros_like(tr.pflat.detach())
    base, start = tr.pflat.data_ptr(), dict(fresh.named_parameters())
    for name, p in tr.model.named_parameters():
        off = (p.data_ptr() - base) // 4
        if 0 <= off < tr.pflat.numel():
            init[off:off + p.numel()] = start[name].detach().reshape(-1)
    return init


def _update_run(groups=3, clip=None, ema=None, on_create=None, **kw):
    """``groups`` groups at k = 2 with keep_grads against a mirror torch Adam fed the step's own gflat * grad_scale (clipped by
    torch, averaged by hand, when asked for).  Returns a report."""
    from equihgnn_amd.trainer import GraphedTrainStep
    model, batches = _build("egnn_equihnns")
    tr = GraphedTrainStep(model, lr=LR, keep_grads=True, accum_steps=2, clip_gnorm=clip, ema_decay=ema, **kw)
    if on_create is not None:
        on_create(tr)
    mirror, opt, avg, norms, coefs = None, None, None, [], []
    for t in range(2 * groups):
        prev = tr.pflat.detach().clone() if tr.pflat is not None else None
        tr.step(batches[t % 3])
        if mirror is None:
            mirror = torch.nn.Parameter(_initial_flat(tr))
            opt = torch.optim.Adam([mirror], lr=LR)
            prev = mirror.detach().clone()
        if tr.micro:            # a non-final micro-step: the weights have not moved
            assert torch.equal(tr.pflat.detach(), prev), t
            continue
        assert tr.opt.grad_scale == 0.5
        mirror.grad = tr.gflat.detach().clone() * tr.opt.grad_scale
        norms.append(float(torch.linalg.vector_norm(mirror.grad.double())))
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([mirror], clip)
            total, coef, _, clipped = tr.grad_norm.tolist()
            assert abs(total - norms[-1]) <= 1e-6 * norms[-1] and coef < 1.0 and clipped == len(norms), (t, total, coef, clipped)
            coefs.append(coef)
        opt.step()
        _assert_close(tr.pflat, mirror, ("pflat", t))
        if ema is not None:     # update 1 copies, then e += (1 - d) (p - e) on the step's own parameters: one update per GROUP
            p = tr.pflat.detach()
            avg = p.clone() if avg is None else avg + (1.0 - ema) * (p - avg)
            _assert_close(tr.ema_flat, avg, ("ema", t))
    assert tr.updates == groups and tr.micro == 0
    assert int(tr.opt.state[tr.pflat]["step_block"][0]) == groups
    assert len(tr.slots) == 1 and tr._g_update is not None
    rep = {"mode": tr.collective_mode, "capture_error": tr.capture_error, "norms": norms, "coefs": coefs,
           "pflat": tr.pflat.detach().cpu().clone()}
    tr.close()
    return rep


def test_one_update_per_group_matches_adam_on_the_groups_gradient():
    rep = _update_run()
    assert rep["mode"] == "none"
    print("group gradient norms:", rep["norms"])
    # once more clipped (half the smallest of those norms: coef < 1 in every group, from the readout) and averaged
    rep2 = _update_run(clip=0.5 * min(rep["norms"]), ema=0.5)
    print("clip coefs:", rep2["coefs"])
    assert len(rep2["coefs"]) == 3


def test_flush_closes_an_open_group_with_the_scale_of_a_full_one():
    from equihgnn_amd.trainer import GraphedTrainStep
    model, batches = _build("egnn_equihnns")
    tr = GraphedTrainStep(model, lr=LR, keep_grads=True, accum_steps=4)
    tr.flush()                              # before the first step: nothing is open
    assert tr.updates == 0 and tr.opt is None
    tr.step(batches[0])
    assert tr.micro == 1 and tr.opt.grad_scale == 0.25
    mirror = torch.nn.Parameter(_initial_flat(tr))
    opt = torch.optim.Adam([mirror], lr=LR)
    assert torch.equal(tr.pflat.detach(), mirror.detach())
    for n_micro in (1, 2):                  # the first close runs eagerly (nothing captured yet), the second the update graph
        if n_micro == 2:
            tr.step(batches[1])
            tr.step(batches[2])
            assert tr.micro == 2
        tr.flush()
        assert tr.micro == 0 and tr.updates == n_micro
        mirror.grad = tr.gflat.detach().clone() / 4
        opt.step()
        _assert_close(tr.pflat, mirror, ("pflat", n_micro))
        held = tr.pflat.detach().clone()
        tr.flush()                          # nothing is open: nothing happens
        assert tr.updates == n_micro and torch.equal(tr.pflat.detach(), held)
        assert int(tr.opt.state[tr.pflat]["step_block"][0]) == n_micro
    assert tr._g_update is not None
    tr.close()


# ---- 6. k = 1 --------------------------------------------------------------------------------------------------------------
def test_accum_steps_one_is_the_step_of_before(monkeypatch):
    from equihgnn_amd.trainer import GraphedTrainStep
    calls = _count(monkeypatch, "eqh_copy_many", "eqh_add_many")
    finals = []
    for kw in ({}, {"accum_steps": 1}):
        before = dict(calls)
        model, batches = _build("egnn_equihnns")
        tr = GraphedTrainStep(model, lr=LR, **kw)
        losses = [float(tr.step(batches[t])) for t in range(3)]
        torch.cuda.synchronize()
        assert tr.updates == 3 and tr.micro == 0 and tr._g_update is None
        assert int(tr.opt.state[tr.pflat]["step_block"][0]) == 3
        finals.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()},
                       calls["eqh_copy_many"] - before["eqh_copy_many"]))
        tr.close()
    assert calls["eqh_add_many"] == 0 and finals[0][2] == finals[1][2] > 0
    assert finals[0][0] == finals[1][0]
    for n, p in finals[0][1].items():
        assert torch.equal(p, finals[1][1][n]), n


# ---- 7. one rank of RCCL ---------------------------------------------------------------------------------------------------
def _rccl_worker(rank, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from equihgnn_amd.trainer import GraphedTrainStep
    out = {}
    for label, kw in (("in_graph", {}), ("split", {"graph_collective": False})):
        counts = {"eager": 0, "captured": 0}
        inside = []
        real_all_reduce, real_captured = dist.all_reduce, GraphedTrainStep._captured_all_reduce
        seen = {}

        def all_reduce(t, *a, _real=real_all_reduce, **k):
            tr = seen.get("tr")
            if tr is not None and tr.gflat is not None and t.data_ptr() == tr.gflat.data_ptr() and not inside:
                counts["eager"] += 1
            return _real(t, *a, **k)

        def captured(self, _real=real_captured):
            counts["captured"] += 1
            inside.append(1)
            try:
                return _real(self)
            finally:
                inside.pop()
        dist.all_reduce, GraphedTrainStep._captured_all_reduce = all_reduce, captured
        try:
            rep = _update_run(groups=2, force_collective=True, on_create=lambda tr: seen.update(tr=tr), **kw)
        finally:
            dist.all_reduce, GraphedTrainStep._captured_all_reduce = real_all_reduce, real_captured
        out[label] = {"mode": rep["mode"], "capture_error": rep["capture_error"], "counts": counts,
                      "pflat": rep["pflat"].tolist()}
    torch.cuda.synchronize()
    json.dump(out, open(out_path, "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_one_collective_per_group_under_one_rank_of_rccl(tmp_path):
    """Test 4's first two groups with force_collective: the first group's all-reduce is eager (it creates the communicator),
    the second group's is the first node of the update graph ("in_graph") or eager in front of it (graph_collective=False):
    one per group either way, grad_scale 1 / 2 (asserted in the run), and the same parameters in both forms."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "report.json"
    mp.spawn(_rccl_worker, args=(port, str(out)), nprocs=1, join=True)      # RCCL lives and dies in a child process
    rep = json.load(open(out))
    print({k: (v["mode"], v["capture_error"], v["counts"]) for k, v in rep.items()})
    a, b = rep["in_graph"], rep["split"]
    assert a["mode"] == "in_graph" or (a["mode"] == "split" and a["capture_error"]), a["mode"]
    if a["mode"] == "in_graph":             # group 1 eager, group 2 the node captured once and replayed once
        assert a["counts"] == {"eager": 1, "captured": 1}
    else:                                   # (the refused capture entered nothing)
        assert a["counts"] == {"eager": 2, "captured": 1}
    assert b["mode"] == "split" and b["counts"] == {"eager": 2, "captured": 0}
    assert a["pflat"] == b["pflat"]
