#!/usr/bin/env python3
"""What reading an epoch's loss and bootstrap metrics once per epoch, instead of once per batch, is worth (not part of
bench.py).  Prints ONE JSON line and writes it to ``--out`` (default profiles/epoch_readout_bench.json).  One process:

``egnn_equihnns`` and ``gin`` at hidden 256 over a synthetic store of ``--train`` training and ``--valid`` validation
molecules (QM9-like / PCQM-like), fed through fit.BucketedLoader + trainer.GraphedTrainStep + fit.Fitter at batch
``--batch``, in two settings -- ``off`` (``Fitter(device_metrics=False)``: one blocking read of the loss per training step,
two of predictions and targets per validation batch, the bootstrap sums on the host) and ``on`` (``device_metrics=True``:
the sums stay on the device and are read once per epoch).  One model, one Fitter and one pair of loaders per setting; after
``--warmup`` epochs of each (bootstrap, captures, the trainer's calibration) the settings run in interleaved blocks of one
epoch: off, on, off, on, ...  The wall time of an epoch's training pass (up to the evaluation) and of its validation pass
are taken separately, on a host clock with a device synchronise at each boundary.

Per setting: the median block and ``spread`` = (max - min) / median of its blocks, and ``host_reads`` per epoch.  The ratio
is reported, not judged.

    python tools/bench_epoch_readout.py [--blocks 5] [--warmup 2] [--train 8192] [--valid 1024] [--batch 256]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETTINGS = (("off", False), ("on", True))
UNIQUE = 1024            # distinct synthetic molecules; the stores repeat them (a shuffled epoch still draws every batch anew)


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def _stores(method, n_train, n_valid):
    from equihgnn_amd.batch import GraphStore, MolStore, synth_graph, synth_molecule
    rng = np.random.default_rng(1234)
    if method == "gin":
        mols = [synth_graph(rng, "pcqm") for _ in range(UNIQUE)]
        make = GraphStore
    else:
        mols = [synth_molecule(rng, "qm9") for _ in range(UNIQUE)]
        make = MolStore
    k = np.array([m.x.shape[0] for m in mols], dtype=np.float64)
    for m, v in zip(mols, (k - k.mean()) / k.std()):          # a learnable, standardised target
        m.y = float(np.float32(v))
    take = lambda n, first: make([mols[(first + i) % UNIQUE] for i in range(n)])
    return take(n_train, 0), take(n_valid, 517)


def _model(method, hidden, batch, dev):
    torch.manual_seed(0)
    if method == "gin":
        from equihgnn_amd.baseline_2d import GNN_2D
        return GNN_2D(1, emb_dim=hidden, gnn_type="gin").to(dev).train(), 1e-4, 0.0
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    ns = default_args(method=method, batch_size=batch, MLP_hidden=hidden)
    return MODELS[method](1, ns).to(dev).train(), ns.lr, ns.wd


def epoch_times(method, a, dev, hidden=256):
    from equihgnn_amd.fit import BucketedLoader, Fitter
    from equihgnn_amd.trainer import GraphedTrainStep
    train_store, valid_store = _stores(method, a.train, a.valid)
    runs = {}
    for name, on in SETTINGS:
        model, lr, wd = _model(method, hidden, a.batch, dev)
        fitter = Fitter(model, lr=lr, weight_decay=wd, std=1.5, step_factory=GraphedTrainStep, device_metrics=on)
        run = {"fitter": fitter, "mark": {},
               "train": BucketedLoader(train_store, a.batch, True, seed=5, device=dev),
               "valid": BucketedLoader(valid_store, a.batch, False, device=dev)}
        evaluate = fitter._evaluate

        def timed_evaluate(loader, run=run, evaluate=evaluate):
            torch.cuda.synchronize()
            run["mark"]["eval_in"] = time.perf_counter()
            val = evaluate(loader)
            torch.cuda.synchronize()
            run["mark"]["eval_out"] = time.perf_counter()
            return val
        fitter._evaluate = timed_evaluate
        runs[name] = run

    def epoch(name):
        """one epoch of one setting: (training pass ms, validation pass ms, host reads)"""
        run = runs[name]
        before = run["fitter"].host_reads
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run["fitter"].fit(run["train"], run["valid"], epochs=1)
        m = run["mark"]
        return (m["eval_in"] - t0) * 1e3, (m["eval_out"] - m["eval_in"]) * 1e3, run["fitter"].host_reads - before

    for name, _ in SETTINGS:                      # bootstrap, captures, the trainer's calibration, the eval graphs
        n = 0
        while n < a.warmup or getattr(runs[name]["fitter"].step, "calibrating", False):
            epoch(name)
            n += 1
            assert n < 20, "the trainer's calibration did not end"
    graphs = {name: len(run["fitter"].step.slots) for name, run in runs.items()}
    times = {name: {"train": [], "valid": [], "epoch": [], "reads": []} for name, _ in SETTINGS}
    for _ in range(a.blocks):
        for name, _ in SETTINGS:
            tr, va, reads = epoch(name)
            t = times[name]
            t["train"].append(tr)
            t["valid"].append(va)
            t["epoch"].append(tr + va)
            t["reads"].append(reads)
    n_train_batches, n_valid_batches = -(-a.train // a.batch), -(-a.valid // a.batch)
    out = {"train_molecules": a.train, "valid_molecules": a.valid, "batch": a.batch, "hidden": hidden,
           "train_batches": n_train_batches, "valid_batches": n_valid_batches,
           "graphs_captured_while_timed": {n: len(r["fitter"].step.slots) - graphs[n] for n, r in runs.items()},
           "index_form": {n: (r["fitter"].step.calibration or {}).get("chosen") for n, r in runs.items()}}
    for name, t in times.items():
        entry = {"host_reads_per_epoch": sorted(set(t["reads"]))}
        for part, per in (("train", n_train_batches), ("valid", n_valid_batches), ("epoch", None)):
            med, sp = _stat(t[part])
            entry[part] = {"ms": round(med, 3), "spread": round(sp, 4), "blocks_ms": [round(v, 3) for v in t[part]]}
            if per:
                entry[part]["ms_per_batch"] = round(med / per, 4)
        out[name] = entry
    for part in ("train", "valid", "epoch"):
        out[f"on_over_off_{part}"] = round(out["on"][part]["ms"] / out["off"][part]["ms"], 4)
    for run in runs.values():
        run["train"].close()
        run["valid"].close()
        run["fitter"].step.close()
    del runs
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train", type=int, default=8192)
    ap.add_argument("--valid", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--methods", default="egnn_equihnns,gin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_readout_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch_readout: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"bench": "epoch_readout", "device": torch.cuda.get_device_name(0),
              "timing": f"{a.warmup}+ warm-up epochs per setting, then {a.blocks} interleaved blocks (off, on, off, on, ...) of one "
                        "epoch each; host clock with a device synchronise before the training pass and around the validation "
                        "pass; median block, spread = (max - min) / median",
              "settings": "off: Fitter(device_metrics=False), the per-batch reads; on: device_metrics=True, one read per epoch",
              "models": {}}
    for method in a.methods.split(","):
        result["models"][f"{method}_b{a.batch}_h256"] = epoch_times(method, a, dev)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
