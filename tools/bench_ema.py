#!/usr/bin/env python3
"""What keeping an exponential moving average (EMA) of the weights costs inside the replayed training step, and what the
exchange around an evaluation costs (not part of bench.py).  Prints ONE JSON line and writes it to ``--out`` (default
profiles/ema_bench.json).  One process:

* the replayed training step (GraphedTrainStep; QM9-like, hidden 256) of ``egnn_equihnns`` at batch 256 and of
  ``equiformer_equihnns`` at batch 128 in two variants -- ``none`` (``ema_decay=None``: the headline's launch list) and
  ``ema999`` (``ema_decay=0.999``: the same launch list, the update kernel in its EMA form -- a fifth stream, 36 bytes per
  parameter instead of 28).  One model and one trainer per variant, fed copies of the same resident batches; after a
  warm-up the variants run in interleaved blocks of ``--steps`` steps on a host clock around a device synchronise;
* the lone exchange (eqh_swap_f32) of two buffers of each step's flat parameter size: a hipGraph of ``REPS`` launches,
  interleaved blocks of ``--inner`` replays between device events.

Per variant: the median block, ``spread`` = (max - min) / median of its blocks.  The cost is reported, not judged.

    python tools/bench_ema.py [--blocks 7] [--steps 10] [--warmup 5] [--inner 3] [--skip-steps] [--skip-kernel]
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
VARIANTS = (("none", None), ("ema999", 0.999))
# flat parameter sizes (floats) of the two steps at hidden 256, used for the lone launch when the steps are skipped
DEFAULT_SIZES = {"egnn_equihnns_b256_h256": 1_375_000, "equiformer_equihnns_b128_h256": 13_500_000}


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def step_times(method, batch, seed0, a, dev, hidden=256):
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    pool = 4
    host = [synth_batch(batch, seed0 + i, "qm9") for i in range(pool)]
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    batches, trainers, counters = {}, {}, {}
    for name, decay in VARIANTS:
        batches[name] = [pad_batch(b, *tgt).packed().to(dev) for b in host]     # (a trainer caches its index on its batches)
        for b in batches[name]:
            b.num_real_graphs = batch
        ns = default_args(method=method, batch_size=batch, MLP_hidden=hidden)
        torch.manual_seed(0)
        model = MODELS[method](1, ns).to(dev).train()
        trainers[name] = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd, ema_decay=decay)
        counters[name] = 0

    def step(name):
        n = counters[name]
        trainers[name].step(batches[name][n % pool], batches[name][(n + 1) % pool])
        counters[name] = n + 1

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
    tr = trainers["ema999"]
    n_par = tr.pflat.numel()
    drift = float((tr.ema_flat - tr.pflat.detach()).abs().max())
    out = {"molecules": batch, "flavour": "qm9", "hidden": hidden, "parameter_floats": n_par,
           "parameter_mbytes": round(n_par * 4 / 1e6, 2), "update_mbytes": {"none": round(n_par * 28 / 1e6, 2),
                                                                            "ema999": round(n_par * 36 / 1e6, 2)},
           "graphs": {n: len(t.slots) for n, t in trainers.items()},
           "index_form": {n: (t.calibration or {}).get("chosen") for n, t in trainers.items()},
           "ema999_steps": counters["ema999"], "ema999_max_abs_live_minus_average": drift}
    base, _ = _stat(times["none"])
    for name, ts in times.items():
        med, sp = _stat(ts)
        out[name] = {"ms": round(med, 4), "spread": round(sp, 4), "vs_none": round(med / base, 4)}
    out["ema_costs_us"] = round((out["ema999"]["ms"] - out["none"]["ms"]) * 1e3, 2)
    for t in trainers.values():
        t.close()
    del trainers, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def kernel_times(sizes, a, dev):
    """the lone eqh_swap_f32 launch over two buffers of ``sizes`` (label -> floats) each"""
    from equihgnn_amd import hip, ops
    L = hip.lib()
    graphs, bufs = {}, {}
    side = torch.cuda.Stream()
    for label, n in sizes.items():
        x, y = torch.randn(n, device=dev), torch.randn(n, device=dev)
        bufs[label] = (x, y, x.clone(), y.clone())

        def run(x=x, y=y, n=n):
            hip.check(L.eqh_swap_f32(ops._ptr(x), ops._ptr(y), n, ops._stream(x.device)), "eqh_swap_f32")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(4):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(REPS):       # (an even count: every replay leaves both buffers as it found them)
                run()
        graphs[label] = gr
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
    out = {}
    for k, ts in times.items():
        med, sp = _stat(ts)
        n = sizes[k]
        x, y, x0, y0 = bufs[k]
        out[k] = {"floats": n, "mbytes_moved": round(n * 16 / 1e6, 2), "us": round(med, 2), "spread": round(sp, 4),
                  "tbytes_per_s": round(n * 16 / (med * 1e-6) / 1e12, 3),
                  "restored": bool(torch.equal(x, x0) and torch.equal(y, y0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS launches) per timed block of the lone launch")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "ema", "device": torch.cuda.get_device_name(0),
              "timing": f"steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock around a device synchronise; "
                        f"lone launch: hipGraphs of {REPS} launches, {a.blocks} interleaved blocks of {a.inner} replays between device "
                        "events (consecutive launches over one pair of buffers: they are read from cache where they fit); median "
                        "block, spread = (max - min) / median",
              "variants": "none: ema_decay=None; ema999: ema_decay=0.999", "steps": {}}
    sizes = dict(DEFAULT_SIZES)
    if not a.skip_steps:
        result["steps"]["egnn_equihnns_b256_h256"] = step_times("egnn_equihnns", 256, 1000, a, dev)
        result["steps"]["equiformer_equihnns_b128_h256"] = step_times("equiformer_equihnns", 128, 3000, a, dev)
        sizes = {k: e["parameter_floats"] for k, e in result["steps"].items()}
    if not a.skip_kernel:
        result["swap"] = kernel_times(sizes, a, dev)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
