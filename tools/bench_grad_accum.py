#!/usr/bin/env python3
"""What accumulating gradients over k micro-batches costs and gives back inside the replayed training step (not part of
bench.py).  Prints ONE JSON line and writes it to ``--out`` (default profiles/grad_accum_bench.json).  One process:

* the replayed training step (GraphedTrainStep; QM9-like) of ``egnn_equihnns`` (batch 256, hidden 256) and of ``mhnnm``
  (batch 256) at ``accum_steps`` = 1, 2, 4, 8: ms per MICRO-batch.  k = 1 is the headline's one graph per step; k > 1 replays
  the accumulate graph per micro-batch and the shared update graph once per group -- one graph launch more on a group's last
  micro-step, k - 1 update launches fewer per group.  One model and one trainer per k, fed copies of the same resident
  batches; after a warm-up the variants run in interleaved blocks of ``--steps`` micro-batches (a multiple of 8: whole groups
  at every k) on a host clock around a device synchronise;
* ``egnn_equihnns`` on PCQM-like batches of 1024 at k = 8 -- the effective step of BASELINE configs[3] (8 ranks x 1024) on one
  GPU: ms per group of eight micro-batches and molecules/s, in blocks of ``--c4-groups`` groups;
* the lone closing launch: eqh_add_many (with and without its clear) against eqh_copy_many over the list of gradients
  autograd allocates (``others``) in the BASELINE step, the mhnnm step and the gin step (768 PCQM-like molecules, width 300):
  hipGraphs of ``REPS`` launches, interleaved blocks of ``--inner`` replays between device events.  A step whose gradients
  all have accumulators has an empty list; that is recorded, nothing is timed for it.

The index form (built ahead / in the step graph) is pinned per method: the trainer's own calibration decides by a 1 % margin
between two timed windows, and variants that came out on different forms would not be comparable.

Per variant: the median block, ``spread`` = (max - min) / median of its blocks.  The cost is reported, not judged.

    python tools/bench_grad_accum.py [--blocks 7] [--steps 16] [--warmup 8] [--inner 3] [--c4-groups 2] [--skip-c4]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

REPS = 20
KS = (1, 2, 4, 8)


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


# the index form each method's calibration settles on at k = 1 (README, "step structure"), pinned here: the calibration's
# timed windows decide by a 1 % margin, and variants that came out on different forms would not be comparable
BUILT_AHEAD = {"egnn_equihnns": True, "mhnnm": False}


def _trainers(method, batch, flavour, seed0, ks, dev, hidden):
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    pool = 4
    host = [synth_batch(batch, seed0 + i, flavour) for i in range(pool)]
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    batches, trainers = {}, {}
    for k in ks:
        batches[k] = [pad_batch(b, *tgt).packed().to(dev) for b in host]     # (a trainer caches its index on its batches)
        for b in batches[k]:
            b.num_real_graphs = batch
        ns = default_args(method=method, batch_size=batch, MLP_hidden=hidden)
        torch.manual_seed(0)
        model = MODELS[method](1, ns).to(dev).train()
        trainers[k] = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd, accum_steps=k)
        trainers[k].index_prefetch = BUILT_AHEAD[method]
    counters = {k: 0 for k in ks}

    def step(k):
        n = counters[k]
        trainers[k].step(batches[k][n % pool], batches[k][(n + 1) % pool])
        counters[k] = n + 1
    return trainers, step


def _warm(trainers, step, warmup):
    """bootstrap, calibration, capture of both graphs and warm-up of each variant; ends on a group boundary"""
    for k, tr in trainers.items():
        for _ in range(2 * k + 1):
            step(k)
        while getattr(tr, "calibrating", False):
            step(k)
        for _ in range(warmup):
            step(k)
        while tr.micro:
            step(k)


def step_times(method, batch, seed0, a, dev, hidden=256):
    trainers, step = _trainers(method, batch, "qm9", seed0, KS, dev, hidden)
    _warm(trainers, step, a.warmup)
    times = {k: [] for k in KS}
    for _ in range(a.blocks):
        for k in KS:
            for _ in range(k):                        # (the first group after a switch of trainers is not timed)
                step(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(k)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    tr = trainers[KS[-1]]
    out = {"molecules": batch, "flavour": "qm9", "hidden": hidden, "parameter_floats": tr.pflat.numel(),
           "autograd_allocated_gradients": len(tr.others), "merged_scratch_floats": 0 if tr.scratch.buf is None else tr.scratch.buf.numel(),
           "accumulate_graphs": {str(k): len(t.slots) for k, t in trainers.items()},
           "update_graph": {str(k): t._g_update is not None for k, t in trainers.items()},
           "index_form": "built_ahead (pinned)" if BUILT_AHEAD[method] else "in_step (pinned)",
           "optimizer_steps": {str(k): t.updates for k, t in trainers.items()}, "ms_per_micro_batch": {}}
    base, _ = _stat(times[1])
    for k, ts in times.items():
        med, sp = _stat(ts)
        out["ms_per_micro_batch"][str(k)] = {"ms": round(med, 4), "spread": round(sp, 4), "vs_k1": round(med / base, 4),
                                             "molecules_per_s": round(batch / med * 1e3, 1)}
    for t in trainers.values():
        t.close()
    del trainers, step
    gc.collect()
    torch.cuda.empty_cache()
    return out


def c4_times(a, dev):
    k, batch = 8, 1024
    trainers, step = _trainers("egnn_equihnns", batch, "pcqm", 4000, (1, k), dev, 256)
    _warm(trainers, step, a.warmup)
    per = k * a.c4_groups
    times = {1: [], k: []}
    for _ in range(min(a.blocks, 5)):
        for kk in (1, k):
            for _ in range(kk):
                step(kk)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                step(kk)
            torch.cuda.synchronize()
            times[kk].append((time.perf_counter() - t0) / a.c4_groups * 1e3)      # ms per eight micro-batches
    out = {"molecules_per_micro_batch": batch, "flavour": "pcqm", "hidden": 256, "accum_steps": k, "index_form": "built_ahead (pinned)",
           "molecules_per_optimizer_step": batch * k, "groups_per_block": a.c4_groups}
    for kk, ts in times.items():
        med, sp = _stat(ts)
        out["k8" if kk == k else "k1_eight_steps"] = {"ms_per_group": round(med, 3), "spread": round(sp, 4),
                                                       "molecules_per_s": round(batch * k / med * 1e3, 1)}
    for t in trainers.values():
        t.close()
    del trainers, step
    gc.collect()
    torch.cuda.empty_cache()
    return out


def closing_launch_times(sizes, zero_n, a, dev):
    """eqh_copy_many, eqh_add_many and eqh_add_many with the scratch clear over one list of ``sizes`` floats"""
    from equihgnn_amd import ops
    pad = lambda n: (n + 63) // 64 * 64
    flat = torch.zeros(sum(pad(n) for n in sizes), device=dev)
    dsts, off = [], 0
    for n in sizes:
        dsts.append(flat[off:off + n])
        off += pad(n)
    srcs = [torch.randn(n, device=dev) * 1e-3 for n in sizes]
    scratch = torch.zeros(zero_n, device=dev)
    runs = {"copy_many": lambda: ops.copy_many(dsts, srcs), "add_many": lambda: ops.add_many(dsts, srcs),
            "add_many_clearing": lambda: ops.add_many(dsts, srcs, zero_also=scratch)}
    graphs, side = {}, torch.cuda.Stream()
    for name, run in runs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(4):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(REPS):
                run()
        graphs[name] = gr
    for gr in graphs.values():
        for _ in range(3):
            gr.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(a.blocks):
        for name, gr in graphs.items():
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.inner):
                gr.replay()
            t.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(t) * 1e3 / (a.inner * REPS))
    out = {"entries": len(sizes), "floats": int(sum(sizes)), "largest_entry": int(max(sizes)), "cleared_floats": int(zero_n)}
    for name, ts in times.items():
        med, sp = _stat(ts)
        out[name] = {"us": round(med, 2), "spread": round(sp, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS launches) per timed block of the lone launch")
    ap.add_argument("--steps", type=int, default=16, help="micro-batches per timed block (a multiple of 8)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--c4-groups", type=int, default=2)
    ap.add_argument("--skip-c4", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_bench.json"))
    a = ap.parse_args()
    if a.steps % 8:
        raise SystemExit("bench_grad_accum: --steps must be a multiple of 8 (whole groups at every k)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_accum: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "grad_accum", "device": torch.cuda.get_device_name(0),
              "timing": f"steps: {a.blocks} interleaved blocks of {a.steps} replayed micro-batches on a host clock around a device "
                        f"synchronise; c4: up to 5 interleaved blocks of {a.c4_groups} groups of 8; lone launch: hipGraphs of {REPS} "
                        f"launches, {a.blocks} interleaved blocks of {a.inner} replays between device events (consecutive launches over "
                        "one list of buffers: they are read from cache where they fit); median block, spread = (max - min) / median",
              "steps": {}}
    result["steps"]["egnn_equihnns_b256_h256"] = step_times("egnn_equihnns", 256, 1000, a, dev)
    result["steps"]["mhnnm_b256"] = step_times("mhnnm", 256, 2000, a, dev)
    if not a.skip_c4:
        result["c4_egnn_equihnns_pcqm_b1024_k8"] = c4_times(a, dev)
    # the closing launch over the list of the BASELINE step and of the mhnnm step: sizes from a trainer of each (a step whose
    # gradients all have accumulators has an empty list: its k = 1 graph has no closing copy at all)
    result["closing_launch"] = {}
    for label, method, seed0 in (("egnn_equihnns_b256_h256", "egnn_equihnns", 1000), ("mhnnm_b256", "mhnnm", 2000),
                                 ("gin_b768_w300", "gin", 3000)):
        if method == "gin":     # (run_pcqm.sh size: the 2-D baselines' gradients are almost all autograd-allocated)
            from equihgnn_amd.baseline_2d import GNN_2D
            from equihgnn_amd.batch import graph_bucket_sizes, pad_graph_batch, synth_graph_batch
            from equihgnn_amd.trainer import GraphedTrainStep
            b = synth_graph_batch(768, seed0, "pcqm")
            b = pad_graph_batch(b, *graph_bucket_sizes(b.num_nodes, b.num_edges)).to(dev)
            torch.manual_seed(0)
            tr = GraphedTrainStep(GNN_2D(1, num_layer=5, emb_dim=300, gnn_type="gin").to(dev).train(), accum_steps=2)
            tr.step(b)
        else:
            trainers, step = _trainers(method, 256, "qm9", seed0, (2,), dev, 256)
            step(2)
            tr = trainers[2]
            del trainers, step
        sizes = [p.numel() for p in tr.others]
        zero_n = 0 if tr.scratch.buf is None else tr.scratch.buf.numel()
        tr.close()
        del tr
        gc.collect()
        result["closing_launch"][label] = (closing_launch_times(sizes, max(zero_n, 1 << 18), a, dev) if sizes else
                                           {"entries": 0, "merged_scratch_floats": zero_n})
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
