#!/usr/bin/env python3
"""What training on L1 / Huber instead of the MSE costs (not part of bench.py).  Prints ONE JSON line and writes it to ``--out``
(default profiles/loss_bench.json).  One process:

* the replayed training step (GraphedTrainStep) of ``egnn_equihnns`` (QM9-like, batch 256, hidden 256: the single fused head),
  of ``mhnn`` (batch 256, hidden 256, output_hidden 128: the paired fused head) and of ``gin`` (PCQM-like, batch 768, the
  reference's defaults: the lone loss launch) with ``loss="mse"``, ``"l1"`` and ``"huber"`` (delta 1).  One model and one
  trainer per variant, fed copies of the same resident batches; after a warm-up the variants run in interleaved blocks of
  ``--steps`` steps on a host clock around a device synchronise;
* the lone launches, forward + backward as the trainer calls them: the single head (C 256, H 128), the paired head (C 256,
  H 256) and the lone loss kernel (768 values) with each loss -- hipGraphs of ``REPS`` launches, interleaved blocks of
  ``--inner`` replays between device events.

Per variant: the median block, ``spread`` = (max - min) / median of its blocks; each other loss is compared with "mse" and the
difference is called "within the spread" unless it exceeds the larger of the two spreads.

    python tools/bench_loss.py [--blocks 7] [--steps 10] [--warmup 5] [--inner 3] [--skip-steps] [--skip-kernels]
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
VARIANTS = (("mse", dict()), ("l1", dict(loss="l1")), ("huber", dict(loss="huber", loss_beta=1.0)))


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def _compare(other, base):
    key = "ms" if "ms" in base else "us"
    diff = (other[key] - base[key]) / base[key]
    sp = max(other["spread"], base["spread"])
    return {"vs_mse": round(other[key] / base[key], 4), "larger_spread": round(sp, 4),
            "verdict": "slower beyond the spread" if diff > sp else ("faster beyond the spread" if -diff > sp else "within the spread")}


def _summary(times, key):
    out = {}
    for name, ts in times.items():
        med, sp = _stat(ts)
        out[name] = {key: round(med, 4 if key == "ms" else 2), "spread": round(sp, 4)}
    for name in times:
        if name != "mse":
            out[name].update(_compare(out[name], out["mse"]))
    return out


def _hyper_setup(method, batch, seed0, dev, **model_kw):
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    pool = 4
    host = [synth_batch(batch, seed0 + i, "qm9") for i in range(pool)]
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))

    def batches():
        out = [pad_batch(b, *tgt).packed().to(dev) for b in host]     # (a trainer caches its index on its batches)
        for b in out:
            b.num_real_graphs = batch
        return out

    def model():
        ns = default_args(method=method, batch_size=batch, **model_kw)
        torch.manual_seed(0)
        return MODELS[method](1, ns).to(dev).train(), dict(lr=ns.lr, weight_decay=ns.wd)
    return batches, model


def _gin_setup(batch, seed0, dev):
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import graph_bucket_sizes, pad_graph_batch, synth_graph_batch
    pool = 4
    host = [synth_graph_batch(batch, seed0 + i, "pcqm") for i in range(pool)]
    ext = [graph_bucket_sizes(b.num_nodes, b.num_edges) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(2))

    def batches():
        out = [pad_graph_batch(b, *tgt).to(dev) for b in host]
        for b in out:
            b.num_real_graphs = batch
        return out

    def model():
        torch.manual_seed(0)
        return GNN_2D(1, gnn_type="gin").to(dev).train(), dict(lr=1e-4)
    return batches, model


def step_times(setup, a):
    from equihgnn_amd.trainer import GraphedTrainStep
    make_batches, make_model = setup
    batches, trainers, counters = {}, {}, {}
    for name, kw in VARIANTS:
        batches[name] = make_batches()
        model, opt_kw = make_model()
        trainers[name] = GraphedTrainStep(model, **opt_kw, **kw)
        counters[name] = 0
    pool = len(batches["mse"])

    def step(name):
        n = counters[name]
        loss = trainers[name].step(batches[name][n % pool], batches[name][(n + 1) % pool])
        counters[name] = n + 1
        return loss

    for name, _ in VARIANTS:                  # bootstrap, calibration, capture and warm-up of each variant
        for _ in range(2):
            step(name)
        while getattr(trainers[name], "calibrating", False):
            step(name)
        for _ in range(1 + a.warmup):
            step(name)
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(a.blocks):
        for name, _ in VARIANTS:
            step(name)                                # (the first step after a switch of trainers is not timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"graphs": {n: len(t.slots) for n, t in trainers.items()},
           "index_form": {n: (t.calibration or {}).get("chosen") for n, t in trainers.items()},
           "last_loss": {n: float(step(n)) for n, _ in VARIANTS}}
    out.update(_summary(times, "ms"))
    for t in trainers.values():
        t.close()
    del trainers, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def _graph_times(runs, a):
    """us per call of each of ``runs`` (label -> callable): hipGraphs of REPS calls, interleaved blocks between device events"""
    graphs, side = {}, torch.cuda.Stream()
    for name, run in runs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
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
        for k, gr in graphs.items():
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.inner):
                gr.replay()
            t.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(t) * 1e3 / (a.inner * REPS))
    return _summary(times, "us")


def kernel_times(a, dev, batch=256, C=256):
    from equihgnn_amd import ops
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import MLP
    data = synth_batch(batch, 1000, "qm9").to(dev)
    ix = HyperIndex.from_batch(data)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(ix.N, C, generator=g).to(dev).requires_grad_(True)
    e = torch.randn(ix.M, C, generator=g).to(dev).requires_grad_(True)
    y = data.y.view(-1).float()
    specs = {name: ops.loss_spec(kw.get("loss", "mse"), kw.get("loss_beta", 1.0)) for name, kw in VARIANTS}
    torch.manual_seed(0)
    single = MLP(C, 128, 1, 3, dropout=0.0, Normalization="ln", InputNorm=False).to(dev).train()
    paired = MLP(2 * C, 256, 1, 3, dropout=0.0, Normalization="ln", InputNorm=False).to(dev).train()
    ps, pp = list(single.parameters()), list(paired.parameters())
    pred = torch.randn(768, generator=g).to(dev).requires_grad_(True)
    tgt = torch.randn(768, generator=g).to(dev)

    def run_single(spec):
        loss, _ = ops.readout_mse(x, ix.pool.rowptr, single, y, None, unit_grad=True, loss=spec)
        return torch.autograd.grad(loss, (x, *ps))

    def run_paired(spec):
        loss, _ = ops.readout_pair_mse(x, e, ix, data.n_e, data.e_order, paired, y, None, unit_grad=True, loss=spec)
        return torch.autograd.grad(loss, (x, e, *pp))

    def run_lone(spec):
        return torch.autograd.grad(ops.regression_loss(pred, tgt, spec), (pred,))

    out = {"unit": "us per forward + backward", "molecules": batch, "node_rows": ix.N, "hyperedge_rows": ix.M}
    for label, fn in (("single_head_c256_h128", run_single), ("paired_head_c256_h256", run_paired), ("lone_loss_n768", run_lone)):
        out[label] = _graph_times({name: (lambda s=spec, f=fn: f(s)) for name, spec in specs.items()}, a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS launches) per timed block of a lone launch")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "loss", "device": torch.cuda.get_device_name(0),
              "timing": f"steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock around a device synchronise; "
                        f"lone launches: hipGraphs of {REPS} launches, {a.blocks} interleaved blocks of {a.inner} replays between "
                        "device events; median block, spread = (max - min) / median",
              "variants": "mse: the default; l1: loss='l1'; huber: loss='huber', loss_beta=1.0", "steps": {}}
    if not a.skip_steps:
        result["steps"]["egnn_equihnns_b256_h256"] = step_times(_hyper_setup("egnn_equihnns", 256, 1000, dev, MLP_hidden=256), a)
        result["steps"]["mhnn_b256_h256_o128"] = step_times(_hyper_setup("mhnn", 256, 2000, dev, MLP_hidden=256, output_hidden=128), a)
        result["steps"]["gin_b768"] = step_times(_gin_setup(768, 1234, dev), a)
    if not a.skip_kernels:
        result["launches"] = kernel_times(a, dev)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
