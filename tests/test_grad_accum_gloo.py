"""Gradient accumulation on two CPU ranks (gloo), in the style of test_trainer_gloo.py: with ``accum_steps=2`` both ranks
end every group with identical parameters and enter exactly ONE collective per group (DDP under ``no_sync``), and the
update is single-process Adam on the mean over ranks of the mean over micro-batches."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from equihgnn_amd.trainer import TrainStep
from test_grad_clip_host import _data, _free_port, _grads, _Net

K, GROUPS = 2, 2


def _batch(rank, t):
    return _data(900 + 10 * t + rank)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _Net(100 + rank)                 # different init per rank: the broadcast fixes that
    tr = TrainStep(model, lr=1e-2, accum_steps=K)
    entered, real = [], dist.all_reduce

    def counted(*a, **kw):
        entered.append(tr.micro)
        return real(*a, **kw)
    dist.all_reduce = counted
    after_group = []
    try:
        for t in range(K * GROUPS):
            tr.step(_batch(rank, t))
            if tr.micro == 0:
                after_group.append({k: v.clone() for k, v in model.state_dict().items()})
    finally:
        dist.all_reduce = real
    torch.save({"after_group": after_group, "entered": entered, "updates": tr.updates},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_enter_one_collective_per_group(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for r in (r0, r1):
        # one all-reduce per group, entered with the group's K micro-batches in the buffer
        assert r["entered"] == [K] * GROUPS and r["updates"] == GROUPS and len(r["after_group"]) == GROUPS
    for g in range(GROUPS):
        for k in r0["after_group"][g]:
            assert torch.equal(r0["after_group"][g][k], r1["after_group"][g][k]), (g, k)
    # single process: rank 0's init, Adam on ((a0 + b0) / 2 + (a1 + b1) / 2) / 2.  Halving is exact and the sum of two numbers
    # does not depend on their order, so this IS what the ranks formed: equality, as in test_grad_clip_host.py
    model = _Net(100)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    for g in range(GROUPS):
        per_rank = []
        for rank in range(world):
            total = None
            for t in range(K * g, K * g + K):
                _grads(model, _batch(rank, t))
                gs = [p.grad.clone() for p in model.parameters()]
                total = gs if total is None else [a + b for a, b in zip(total, gs)]
            per_rank.append([a * (1.0 / K) for a in total])
        for p, g0, g1 in zip(model.parameters(), *per_rank):
            p.grad = (g0 + g1) * 0.5
        opt.step()
        for k, v in model.state_dict().items():
            assert torch.equal(r0["after_group"][g][k], v), (g, k)
