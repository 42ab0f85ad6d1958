#!/usr/bin/env python3
"""Measurement of ``faformer_equihnn`` and ``faformer_equihnnm`` and of the paired pool (not part of bench.py).  Prints ONE
JSON line and writes it to ``--out`` (default profiles/faformer_paired_bench.json):

* the training step of both methods -- and of ``faformer_equihnns`` as the anchor measured in the same process -- at the
  size of BASELINE config 4 (PCQM-like molecules, batch 512, hidden 256, FAFormer's training dropouts): replayed
  (GraphedTrainStep over a pool of padded batches, the next batch's index built beside the step, as bench.py's
  ``timed_run``) and eager (TrainStep, the index rebuilt every step).  Each figure is the median of ``--blocks`` blocks of
  ``--steps`` steps, every block between device synchronisations on a host clock; ``spread`` is (max - min) / median of
  the blocks;
* ``hg_pool_pair`` next to the read-out it replaces (models._PairedBase._pool with ``fused_pool`` False: mask, [M, C]
  product, two segment reduces, concatenation and their four backward launches) on that batch's rows at hidden 256,
  forward + backward.  Both are captured as hipGraphs of ``REPS`` repetitions -- the launches of either are a few
  microseconds each, so issuing them from Python measures the host -- and replayed alternately, ``--rounds`` times
  each between device events; per variant the median per repetition and the spread of the rounds.  Their eager
  (launch-bound) times are reported too, named as such.  ``algorithmic_bytes`` are ops.pool_pair_bytes (from shapes).

    python tools/bench_faformer_paired.py [--steps 10] [--blocks 5] [--warmup 5] [--rounds 15]
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

REPS = 20          # forward + backward repetitions inside one captured graph
POOL = 4           # batches a trainer cycles through


def _blocks(step, n_blocks, n_steps, start):
    els = []
    for k in range(n_blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            step(start + k * n_steps + i)
        torch.cuda.synchronize()
        els.append((time.perf_counter() - t0) / n_steps * 1e3)
    med = statistics.median(els)
    return {"ms": round(med, 4), "spread": round((max(els) - min(els)) / med, 4), "blocks_ms": [round(v, 4) for v in els]}


def step_times(method, batch, a, dev):
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep, TrainStep
    ns = default_args(method=method, batch_size=batch)
    host = [synth_batch(batch, 4000 + i, "pcqm") for i in range(POOL)]
    out = {"molecules": batch, "hidden": ns.MLP_hidden, "atoms": [int(b.num_nodes) for b in host]}
    # replayed
    torch.manual_seed(0)
    model = MODELS[method](1, ns).to(dev).train()
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    batches = [pad_batch(b, *tgt).packed().to(dev) for b in host]
    for b in batches:
        b.num_real_graphs = batch
    tr = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd)
    step = lambda j: tr.step(batches[j % POOL], batches[(j + 1) % POOL])
    base = 0
    for _ in range(2):                      # set-up: the eager bootstrap step and the capture step
        step(base)
        base += 1
    while getattr(tr, "calibrating", False):
        step(base)
        base += 1
    for _ in range(a.warmup):
        step(base)
        base += 1
    r = _blocks(step, a.blocks, a.steps, base)
    out["replayed"] = dict(r, mol_s=round(batch / r["ms"] * 1e3, 1), graphs=len(tr.slots))
    tr.close()
    del tr, model, batches
    # eager
    torch.manual_seed(0)
    model = MODELS[method](1, ns).to(dev).train()
    plain = [b.to(dev) for b in host]
    te = TrainStep(model, lr=ns.lr, weight_decay=ns.wd)
    te.on_batch = lambda b: setattr(b, "_hyper_index", None)       # every step sees a "new" batch: the index is rebuilt
    estep = lambda j: te.step(plain[j % POOL])
    for j in range(max(2, a.warmup)):
        estep(j)
    r = _blocks(estep, max(3, a.blocks // 2), max(3, a.steps // 2), 0)
    out["eager"] = dict(r, mol_s=round(batch / r["ms"] * 1e3, 1))
    del te, model, plain
    torch.cuda.empty_cache()
    return out


def pool_comparison(batch, hidden, a, dev):
    from equihgnn_amd import ops
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import pool_sum
    d = synth_batch(batch, 4000, "pcqm").to(dev)
    index = HyperIndex.from_batch(d)
    he_csr, he_key = index.hyperedge_pool(d.n_e)
    N, M, C = int(d.x.shape[0]), int(d.edge_attr.shape[0]), hidden
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    e = torch.randn(M, C, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(batch, 2 * C, generator=g).to(dev)

    def variants(x, e):
        def fused():
            return ops.pool_pair(x, e, index, d.n_e, d.e_order)

        def replaced():
            keep = (d.e_order > 2).to(e.dtype).unsqueeze(-1)
            return torch.cat((pool_sum(x, index), ops.reduce_entries(e * keep, he_csr, he_key, "sum")), -1)

        def both_ways(fn):
            out = fn()
            return out, torch.autograd.grad(out, (x, e), w)
        return (("pool_pair", fused), ("replaced_path", replaced)), both_ways

    res = {"molecules": batch, "atoms": N, "hyperedges": M, "high_order_hyperedges": int((d.e_order > 2).sum()),
           "hidden": C, "reps_per_graph": REPS}
    fb, bb = ops.pool_pair_bytes(N, M, batch, C)
    res["algorithmic_bytes"] = {"fwd": fb, "bwd": bb}
    # The captures come first, on leaves no eager pass has touched: a capture that meets an autograd node bound to another
    # stream (left by an eager pass whose results are still alive) is invalidated.
    pairs, both_ways = variants(x, e)
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in pairs:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                both_ways(fn)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gc.collect()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side, capture_error_mode="thread_local"):
            for _ in range(REPS):
                both_ways(fn)
        graphs[name] = gr
    times = {k: [] for k in graphs}
    for gr in graphs.values():
        for _ in range(5):
            gr.replay()
    torch.cuda.synchronize()
    inner = 10
    for _ in range(a.rounds):            # alternate the two variants
        for name, gr in graphs.items():
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                gr.replay()
            t.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(t) * 1e3 / (inner * REPS))
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"fwd_bwd_us": round(med, 3), "spread": round((max(ts) - min(ts)) / med, 4)}
    res["pool_pair"]["fraction_of_hbm_8tb_s"] = round((fb + bb) / (res["pool_pair"]["fwd_bwd_us"] * 1e-6) / 8.0e12, 4)
    res["replaced_over_pool_pair"] = round(res["replaced_path"]["fwd_bwd_us"] / res["pool_pair"]["fwd_bwd_us"], 3)
    del graphs
    # eager, on leaves of their own: same inputs, same results (values and both gradients), and the launch-bound times
    pairs, both_ways = variants(x.detach().clone().requires_grad_(True), e.detach().clone().requires_grad_(True))
    (o1, (gx1, ge1)), (o2, (gx2, ge2)) = both_ways(pairs[0][1]), both_ways(pairs[1][1])
    res["max_abs_difference"] = {"out": float((o1 - o2).detach().abs().max()), "dx": float((gx1 - gx2).abs().max()),
                                 "de": float((ge1 - ge2).abs().max())}
    del o1, o2, gx1, gx2, ge1, ge2
    for name, fn in pairs:       # launch-bound: issued from Python
        for _ in range(5):
            both_ways(fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            both_ways(fn)
        torch.cuda.synchronize()
        res[name]["eager_launch_bound_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--methods", default="faformer_equihnns,faformer_equihnn,faformer_equihnnm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faformer_paired_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_faformer_paired: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "faformer_paired", "device": torch.cuda.get_device_name(0),
              "workload": f"PCQM-like synthetic molecules, batch {a.batch}, hidden 256, training mode (FAFormer's 0.1 dropouts on)",
              "timing": f"median of {a.blocks} blocks of {a.steps} steps after {a.warmup} warm-up steps; spread = (max - min) / median",
              "pool": pool_comparison(a.batch, 256, a, dev), "steps": {}}
    for method in a.methods.split(","):
        result["steps"][method] = step_times(method, a.batch, a, dev)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
