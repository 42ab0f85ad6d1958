#!/usr/bin/env python3
"""What ``--dropout`` costs on the conv tails, with and without the dropout forms of the fused row kernels (not part of
bench.py).  Prints ONE JSON line and writes it to ``--out`` (default profiles/conv_dropout_bench.json).  One process:

* the replayed training step (GraphedTrainStep; QM9-like, batch 256, hidden 256) of ``egnn_equihnns``, ``mhnns``,
  ``faformer_equihnns``, ``mhnnm`` and ``egnn_equihnnm`` in up to five variants -- ``p0`` (dropout 0: the headline's path),
  ``p0.1_fused`` (dropout 0.1, ``ops.FUSED_DROPOUT = True``: the hidden layers' dropout inside the kernels -- the row kernels
  of csrc/incidence.hip, for the MHNNConv methods the DROP forms of the panel kernels, ``ops.PANEL_DROPOUT = True``, and for
  the S-tail methods the dropout forms of the conv stack's stages, ``ops.STACK_DROPOUT = True``), ``p0.1_rows`` (the MHNNConv
  methods only: dropout 0.1 with ``ops.PANEL_DROPOUT = False`` -- an MHNNConv with an active dropout leaves the panels for the
  row kernels, the path before that switch existed), ``p0.1_stack_off`` (the S-tail methods only: dropout 0.1 with
  ``ops.STACK_DROPOUT = False`` -- the conv stack leaves the panels for the loop over the row kernels, the path before that
  switch existed and its yardstick), ``p0.1_readout_off`` (``egnn_equihnns``, ``mhnns`` and ``mhnnm``: dropout 0.1 with
  ``ops.READOUT_DROPOUT = False`` -- the read-out head leaves its one launch for dropout_add, pool, three Linears, two
  bias_relu_ln and the loss, the path before that switch existed and its yardstick) and ``p0.1_aten`` (dropout 0.1 with
  ``ops.FUSED_DROPOUT`` off: ReLU,
  LayerNorm and F.dropout as ATen launches on materialised rows, the path before either switch existed).  One model and one
  trainer per variant, fed copies of the same resident batches; after a warm-up the variants run in interleaved blocks of
  ``--steps`` steps on a host clock around a device synchronise.  The switches are set ahead of every block, so a capture
  that happens late still sees its variant's values;
* the lone ``ops.incidence_ln_reduce``, forward plus backward, on the incidences of one such batch (nnz ~ 10 k, C = 256,
  rows keyed by the nodes) with p = 0 and p = 0.1: hipGraphs of ``REPS`` forward + backward pairs, interleaved blocks of
  ``--inner`` replays between device events.

Per variant: the median block, ``spread`` = (max - min) / median of its blocks.  ``verdict`` says per method whether the fused
step is faster than the ATen step by more than both spreads -- the condition for ``FUSED_DROPOUT`` to be on by default --
and ``panel_verdict`` whether the panel step beats the row-kernel step by more than the larger of the two spreads -- the
condition for ``PANEL_DROPOUT``, decided by ``mhnnm``; ``stack_verdict`` the same for ``STACK_DROPOUT``, decided by
``egnn_equihnns``; ``readout_verdict`` the same for ``READOUT_DROPOUT``, decided by ``egnn_equihnns``.

    python tools/bench_conv_dropout.py [--blocks 7] [--steps 10] [--warmup 5] [--inner 3] [--skip-steps] [--skip-kernel]
                                       [--methods mhnnm,egnn_equihnnm] [--variants p0,p0.1_fused,p0.1_rows]
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

REPS = 10
# (name, dropout, ops.FUSED_DROPOUT, ops.PANEL_DROPOUT, ops.STACK_DROPOUT, ops.READOUT_DROPOUT)
VARIANTS = (("p0", 0.0, True, True, True, True), ("p0.1_fused", 0.1, True, True, True, True),
            ("p0.1_rows", 0.1, True, False, True, True), ("p0.1_stack_off", 0.1, True, True, False, True),
            ("p0.1_readout_off", 0.1, True, True, True, False), ("p0.1_aten", 0.1, False, True, True, True))
STEPS = {"egnn_equihnns": 1000, "mhnnm": 2000, "egnn_equihnnm": 3000, "mhnns": 4000, "faformer_equihnns": 5000}   # method -> seed of its batches
MHNN_CONV = ("mhnnm", "egnn_equihnnm")                                      # methods whose conv is MHNNConv: the panel switch matters
S_TAIL = ("egnn_equihnns", "mhnns", "faformer_equihnns")                    # methods on the S tail: the stack switch matters
READOUT = ("egnn_equihnns", "mhnns", "mhnnm")                               # methods the read-out switch is measured on


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def step_times(method, batch, seed0, a, dev, hidden=256):
    from equihgnn_amd import ops
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    pool = 4
    host = [synth_batch(batch, seed0 + i, "qm9") for i in range(pool)]
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    batches, trainers, counters = {}, {}, {}
    variants = [v for v in VARIANTS if v[0] in a.variants and (v[0] != "p0.1_rows" or method in MHNN_CONV)
                and (v[0] != "p0.1_stack_off" or method in S_TAIL) and (v[0] != "p0.1_readout_off" or method in READOUT)]
    stack_default, readout_default = ops.STACK_DROPOUT, ops.READOUT_DROPOUT

    def switches(fused, panel, stack, readout):
        ops.FUSED_DROPOUT, ops.PANEL_DROPOUT, ops.STACK_DROPOUT, ops.READOUT_DROPOUT = fused, panel, stack, readout

    for name, p, *_ in variants:
        batches[name] = [pad_batch(b, *tgt).packed().to(dev) for b in host]     # (a trainer caches its index on its batches)
        for b in batches[name]:
            b.num_real_graphs = batch
        ns = default_args(method=method, batch_size=batch, MLP_hidden=hidden, dropout=p)
        torch.manual_seed(0)
        model = MODELS[method](1, ns).to(dev).train()
        trainers[name] = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd)
        counters[name] = 0

    def step(name):
        n = counters[name]
        trainers[name].step(batches[name][n % pool], batches[name][(n + 1) % pool])
        counters[name] = n + 1

    try:
        for name, _, *sw in variants:     # bootstrap, calibration, capture and warm-up of each variant
            switches(*sw)
            for _ in range(2):
                step(name)
            while getattr(trainers[name], "calibrating", False):
                step(name)
            for _ in range(1 + a.warmup):
                step(name)
        times = {v[0]: [] for v in variants}
        for _ in range(a.blocks):
            for name, _, *sw in variants:
                switches(*sw)
                step(name)                                # (the first step after a switch of trainers is not timed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    finally:
        switches(True, True, stack_default, readout_default)
    out = {"molecules": batch, "flavour": "qm9", "hidden": hidden, "graphs": {n: len(t.slots) for n, t in trainers.items()}}
    base, _ = _stat(times["p0"])
    for name, ts in times.items():
        med, sp = _stat(ts)
        out[name] = {"ms": round(med, 4), "spread": round(sp, 4), "vs_p0": round(med / base, 4)}
    f, t, r, k = out.get("p0.1_fused"), out.get("p0.1_aten"), out.get("p0.1_rows"), out.get("p0.1_stack_off")
    if f and t:
        out["fused_vs_aten"] = round(f["ms"] / t["ms"], 4)
        out["fused_faster_beyond_both_spreads"] = bool(f["ms"] * (1 + f["spread"]) < t["ms"] * (1 - t["spread"]))
    if f and r:     # the panel path of MHNNConv against the row kernels it left the panels for
        out["panel_vs_rows"] = round(f["ms"] / r["ms"], 4)
        out["panel_faster_beyond_the_larger_spread"] = bool((r["ms"] - f["ms"]) / r["ms"] > max(f["spread"], r["spread"]))
    if f and k:     # the conv stack under dropout against the loop over the row kernels it left the panels for
        out["stack_vs_stack_off"] = round(f["ms"] / k["ms"], 4)
        out["stack_faster_beyond_the_larger_spread"] = bool((k["ms"] - f["ms"]) / k["ms"] > max(f["spread"], k["spread"]))
    o = out.get("p0.1_readout_off")
    if f and o:     # the fused read-out head under dropout against the separate launches it left its one launch for
        out["readout_vs_readout_off"] = round(f["ms"] / o["ms"], 4)
        out["readout_faster_beyond_the_larger_spread"] = bool((o["ms"] - f["ms"]) / o["ms"] > max(f["spread"], o["spread"]))
    for tr in trainers.values():
        tr.close()
    del trainers, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def kernel_times(a, dev, batch=256, C=256):
    """the lone incidence_ln_reduce (rows keyed by the nodes: the (rowptr, col) forward), forward + backward, p = 0 | 0.1"""
    from equihgnn_amd import ops
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.index import HyperIndex
    data = synth_batch(batch, 1000, "qm9").to(dev)
    ix = HyperIndex.from_batch(data)
    g = torch.Generator().manual_seed(0)
    pa = torch.randn(ix.N, C, generator=g).to(dev).requires_grad_(True)
    qb = torch.randn(ix.M, C, generator=g).to(dev).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(dev).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g)).to(dev).requires_grad_(True)
    w = torch.randn(ix.N, C, generator=g).to(dev)
    seed = torch.tensor([12345], dtype=torch.int64, device=dev)

    def run(p):
        out = ops.incidence_ln_reduce(pa, qb, gamma, beta, ix.v32, ix.e32, ix.by_v, ix.by_e, ix.by_v, ix.v32, "mean", p=p, seed=seed)
        return torch.autograd.grad(out, (pa, qb, gamma, beta), w)

    graphs = {}
    side = torch.cuda.Stream()
    for name, p in (("p0", 0.0), ("p0.1", 0.1)):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                run(p)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(REPS):
                run(p)
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
    entry = {"nnz": ix.nnz, "node_rows": ix.N, "hyperedge_rows": ix.M, "C": C,
             "launches_per_pair": "forward + backward (both sides in one launch) + the slab reduction; p = 0 adds the column sum for d beta"}
    base, base_sp = _stat(times["p0"])
    for k, ts in times.items():
        med, sp = _stat(ts)
        entry[k] = {"us_forward_plus_backward": round(med, 2), "spread": round(sp, 4), "vs_p0": round(med / base, 4)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS forward + backward pairs) per timed block of the kernel")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--methods", default=",".join(STEPS), help="comma-separated, of " + ", ".join(STEPS))
    ap.add_argument("--variants", default=",".join(v[0] for v in VARIANTS), help="comma-separated; p0 is always run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_dropout_bench.json"))
    a = ap.parse_args()
    a.methods = [m for m in a.methods.split(",") if m]
    a.variants = set(a.variants.split(",")) | {"p0"}
    if any(m not in STEPS for m in a.methods):
        raise SystemExit(f"bench_conv_dropout: --methods takes {', '.join(STEPS)}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_dropout: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "conv_dropout", "device": torch.cuda.get_device_name(0),
              "timing": f"steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock around a device synchronise; "
                        f"kernel: hipGraphs of {REPS} forward + backward pairs, {a.blocks} interleaved blocks of {a.inner} replays between "
                        "device events; median block, spread = (max - min) / median",
              "variants": "p0: dropout 0; p0.1_fused: dropout 0.1 with ops.FUSED_DROPOUT and ops.PANEL_DROPOUT on; p0.1_rows (MHNNConv "
                          "methods): dropout 0.1 with ops.PANEL_DROPOUT off; p0.1_stack_off (S-tail methods): dropout 0.1 with "
                          "ops.STACK_DROPOUT off; p0.1_readout_off (egnn_equihnns, mhnns, mhnnm): dropout 0.1 with "
                          "ops.READOUT_DROPOUT off; p0.1_aten: dropout 0.1 with ops.FUSED_DROPOUT off",
              "steps": {}}
    if not a.skip_kernel:
        result["incidence_ln_reduce"] = kernel_times(a, dev)
    if not a.skip_steps:
        for method in a.methods:
            result["steps"][f"{method}_b256_h256"] = step_times(method, 256, STEPS[method], a, dev)
        fused = {k: e for k, e in result["steps"].items() if "fused_faster_beyond_both_spreads" in e}
        if fused:
            result["verdict"] = {k: ("fused faster than ATen beyond both spreads" if e["fused_faster_beyond_both_spreads"]
                                     else "not faster beyond the spreads") for k, e in fused.items()}
            result["switch_on_by_default_is_justified"] = all(e["fused_faster_beyond_both_spreads"] for e in fused.values())
        panel = {k: e for k, e in result["steps"].items() if "panel_faster_beyond_the_larger_spread" in e}
        if panel:
            result["panel_verdict"] = {k: ("panels faster than the row kernels beyond the larger spread"
                                           if e["panel_faster_beyond_the_larger_spread"] else "not faster beyond the spreads")
                                       for k, e in panel.items()}
            if "mhnnm_b256_h256" in panel:
                result["panel_switch_on_by_default_is_justified"] = panel["mhnnm_b256_h256"]["panel_faster_beyond_the_larger_spread"]
        stack = {k: e for k, e in result["steps"].items() if "stack_faster_beyond_the_larger_spread" in e}
        if stack:
            result["stack_verdict"] = {k: ("stack faster than the row kernels beyond the larger spread"
                                           if e["stack_faster_beyond_the_larger_spread"] else "not faster beyond the spreads")
                                       for k, e in stack.items()}
            if "egnn_equihnns_b256_h256" in stack:
                result["stack_switch_on_by_default_is_justified"] = stack["egnn_equihnns_b256_h256"]["stack_faster_beyond_the_larger_spread"]
        ro = {k: e for k, e in result["steps"].items() if "readout_faster_beyond_the_larger_spread" in e}
        if ro:
            result["readout_verdict"] = {k: ("fused read-out faster than the separate launches beyond the larger spread"
                                             if e["readout_faster_beyond_the_larger_spread"] else "not faster beyond the spreads")
                                         for k, e in ro.items()}
            if "egnn_equihnns_b256_h256" in ro:
                result["readout_switch_on_by_default_is_justified"] = ro["egnn_equihnns_b256_h256"]["readout_faster_beyond_the_larger_spread"]
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
