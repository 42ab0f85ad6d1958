#!/usr/bin/env python3
"""What the paired tail's one-launch read-out head (csrc/readout_pair.hip, ``ops.PAIRED_READOUT``) buys (not part of bench.py).
Prints ONE JSON line and writes it to ``--out`` (default profiles/paired_readout_bench.json).  One process:

* the lone head, forward + backward, on the rows of one QM9-like batch of 256 molecules at hidden 256, output_hidden 128 (the
  head is 512 -> 256 -> 256 -> 1), with p = 0 and p = 0.1: ``ops.readout_pair_mse`` against the launches it replaces on the
  same inputs -- the two dropout_add passes (p > 0), the pool as ``mhnn`` / ``egnn_equihnn`` run it (two segment reduces, a
  mask product and a cat) and as ``faformer_equihnn`` runs it (ops.pool_pair), three Linears, two bias_relu_ln, mse_loss and
  all their backward launches.  hipGraphs of ``REPS`` forward + backward pairs, interleaved blocks of ``--inner`` replays
  between device events;
* the replayed training step (GraphedTrainStep) of ``mhnn`` and ``egnn_equihnn`` at batch 256, hidden 256, output_hidden 128,
  with dropout 0 and 0.1, switch on and off: one model and one trainer per variant, fed copies of the same resident batches;
  after a warm-up the variants run in interleaved blocks of ``--steps`` steps on a host clock around a device synchronise.  The
  switch is set ahead of every block, so a capture that happens late still sees its variant's value.

The switch-off path is the code as it was before the switch existed and is the reference of every ratio.  Per variant: the
median block, ``spread`` = (max - min) / median of its blocks; a gain is reported only where it exceeds the larger of the two
spreads.  ``switch_on_by_default_is_justified``: the step is faster beyond that spread for at least one of the two
probabilities on both methods and slower beyond it for none.  Every GPU phase runs under a time limit (``--limit`` seconds: the
process dumps its stacks and exits when a phase overruns it).

    python tools/bench_paired_readout.py [--blocks 7] [--steps 10] [--warmup 5] [--inner 3] [--skip-steps] [--skip-head]
"""
from __future__ import annotations

import argparse
import contextlib
import faulthandler
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
METHODS = {"mhnn": 6000, "egnn_equihnn": 7000}       # method -> seed of its batches
PROBS = (0.0, 0.1)


@contextlib.contextmanager
def limited(seconds):
    """a GPU phase that may not outlast ``seconds``: past it the stacks are dumped and the process exits"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def _compare(on, off):
    """on / off of two {"x": median, "spread": ...} entries and whether the difference exceeds the larger spread"""
    key = "ms" if "ms" in on else "us"
    gain = (off[key] - on[key]) / off[key]
    sp = max(on["spread"], off["spread"])
    return {"on_vs_off": round(on[key] / off[key], 4), "larger_spread": round(sp, 4),
            "verdict": "faster beyond the spread" if gain > sp else ("slower beyond the spread" if -gain > sp else "within the spread")}


def _model(method, p, dev, batch=256):
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    ns = default_args(method=method, batch_size=batch, MLP_hidden=256, output_hidden=128, dropout=p)
    torch.manual_seed(0)
    return MODELS[method](1, ns).to(dev).train(), ns


def head_times(a, dev, batch=256, C=256):
    """the lone head, forward + backward: one launch | the separate launches with either pool"""
    from equihgnn_amd import ops
    from equihgnn_amd.batch import synth_batch
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.layers import head_loss
    data = synth_batch(batch, 1000, "qm9").to(dev)
    ix = HyperIndex.from_batch(data)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(ix.N, C, generator=g).to(dev).requires_grad_(True)
    e = torch.randn(ix.M, C, generator=g).to(dev).requires_grad_(True)
    y = data.y.view(-1).float()
    entry = {"molecules": batch, "node_rows": ix.N, "hyperedge_rows": ix.M, "rows_of_order_above_2": int((data.e_order > 2).sum()),
             "C": C, "head": "512 -> 256 -> 256 -> 1",
             "unit": "us per forward + backward of the head (the gradients of x, e and the ten parameters)"}
    for p in PROBS:
        m, _ = _model("mhnn", p, dev, batch)
        params = list(m.mlp_out.parameters())

        def fused():
            # (unit_grad: the incoming gradient is the implicit 1, as the trainer calls it -- no scaling passes over the gradients)
            loss, _ = ops.readout_pair_mse(x, e, ix, data.n_e, data.e_order, m.mlp_out, y, None, unit_grad=True, p_x=p)
            return torch.autograd.grad(loss, (x, e, *params))

        def separate(fused_pool):
            m.fused_pool = fused_pool
            both = m._pool(m._drop(x), m._drop(e), ix, data)
            loss = head_loss(m.mlp_out(both, mask=ix.pad_masks()[3]).view(-1), (y, None))
            return torch.autograd.grad(loss, (x, e, *params))

        runs = {"one_launch": fused, "separate": lambda: separate(False), "separate_pool_pair": lambda: separate(True)}
        graphs, side = {}, torch.cuda.Stream()
        with limited(a.limit):
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
        with limited(a.limit):
            for _ in range(a.blocks):
                for k, gr in graphs.items():
                    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(a.inner):
                        gr.replay()
                    t.record()
                    torch.cuda.synchronize()
                    times[k].append(s.elapsed_time(t) * 1e3 / (a.inner * REPS))
        sub = {}
        for k, ts in times.items():
            med, sp = _stat(ts)
            sub[k] = {"us": round(med, 2), "spread": round(sp, 4)}
        sub["vs_separate"] = _compare(sub["one_launch"], sub["separate"])
        sub["vs_separate_pool_pair"] = _compare(sub["one_launch"], sub["separate_pool_pair"])
        entry[f"p{p:g}"] = sub
        del graphs, m
        gc.collect()
    return entry


def step_times(method, seed0, a, dev, batch=256):
    from equihgnn_amd import ops
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.trainer import GraphedTrainStep
    pool = 4
    host = [synth_batch(batch, seed0 + i, "qm9") for i in range(pool)]
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    variants = [(f"p{p:g}_{'on' if sw else 'off'}", p, sw) for p in PROBS for sw in (True, False)]
    batches, trainers, counters = {}, {}, {}
    default = ops.PAIRED_READOUT
    for name, p, _ in variants:
        batches[name] = [pad_batch(b, *tgt).packed().to(dev) for b in host]     # (a trainer caches its index on its batches)
        for b in batches[name]:
            b.num_real_graphs = batch
        model, ns = _model(method, p, dev, batch)
        trainers[name] = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd)
        counters[name] = 0

    def step(name):
        n = counters[name]
        trainers[name].step(batches[name][n % pool], batches[name][(n + 1) % pool])
        counters[name] = n + 1

    try:
        for name, _, sw in variants:     # bootstrap, calibration, capture and warm-up of each variant
            ops.PAIRED_READOUT = sw
            with limited(a.limit):
                for _ in range(2):
                    step(name)
                while getattr(trainers[name], "calibrating", False):
                    step(name)
                for _ in range(1 + a.warmup):
                    step(name)
                torch.cuda.synchronize()
        times = {v[0]: [] for v in variants}
        for _ in range(a.blocks):
            for name, _, sw in variants:
                ops.PAIRED_READOUT = sw
                with limited(a.limit):
                    step(name)                                # (the first step after a switch of trainers is not timed)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        step(name)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    finally:
        ops.PAIRED_READOUT = default
    out = {"molecules": batch, "flavour": "qm9", "hidden": 256, "output_hidden": 128,
           "graphs": {n: len(t.slots) for n, t in trainers.items()}}
    for name, ts in times.items():
        med, sp = _stat(ts)
        out[name] = {"ms": round(med, 4), "spread": round(sp, 4)}
    for p in PROBS:
        on, off = out[f"p{p:g}_on"], out[f"p{p:g}_off"]
        out[f"p{p:g}"] = dict(_compare(on, off), gain_ms=round(off["ms"] - on["ms"], 4))
    for tr in trainers.values():
        tr.close()
    del trainers, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS forward + backward pairs) per timed block of the head")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU phase may take before the process gives up")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paired_readout_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paired_readout: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "paired_readout", "device": torch.cuda.get_device_name(0),
              "timing": f"head: hipGraphs of {REPS} forward + backward pairs, {a.blocks} interleaved blocks of {a.inner} replays between "
                        f"device events; steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock around a "
                        "device synchronise; median block, spread = (max - min) / median; a verdict compares the difference with "
                        "the larger of the two spreads",
              "reference": "switch off: the separate launches, the path before ops.PAIRED_READOUT existed",
              "steps": {}}
    if not a.skip_head:
        result["head"] = head_times(a, dev)
    if not a.skip_steps:
        for method, seed0 in METHODS.items():
            result["steps"][f"{method}_b256_h256_o128"] = step_times(method, seed0, a, dev)
        verdicts = [e[f"p{p:g}"]["verdict"] for e in result["steps"].values() for p in PROBS]
        per_method = [any(e[f"p{p:g}"]["verdict"] == "faster beyond the spread" for p in PROBS) for e in result["steps"].values()]
        result["switch_on_by_default_is_justified"] = bool(all(per_method) and "slower beyond the spread" not in verdicts)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
