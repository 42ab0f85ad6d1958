#!/usr/bin/env python3
"""What a device-resident dataset costs and saves (not part of bench.py).  Needs a GPU.  Writes ONE JSON line to --out
(profiles/device_loader_bench.json) and prints it.

Two workloads, each fed three ways by ONE trainer in ONE process, in interleaved blocks after the buckets are warm:

    egnn_equihnns   batch 256, hidden 256, 8192 QM9-like molecules
    gin             batch 768, width 300, 5 layers, PCQM-like molecules

    resident   the epoch's padded batches already in device memory (nothing is assembled)
    host       fit.BucketedLoader over the host store: producer thread, hb_collate / gb_collate into pinned staging, one
               host-to-device copy per batch on a side stream -- the baseline
    device     fit.BucketedLoader over store.to_device(): two collate launches per batch on the side stream, no thread

Per feed: ms/step (median over the blocks and (max - min) / median), the fraction of the resident step,
time.process_time() per epoch (the CPU seconds of the WHOLE process: launches included, so the data path's cost is the
difference from `resident`), threads alive while it iterates (counted in the warm-up epoch, before the host loader ran).
Beside them: the collate pair alone in a replayed hipGraph at B = 256 QM9-like and B = 1024 PCQM-like against the algorithmic
bytes it moves, and hb_collate + the host-to-device copy of the same batches, for scale.

    python tools/bench_device_loader.py [--blocks 5] [--epochs-per-block 8] [--out profiles/device_loader_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8.0e12


def _spread(v):
    med = sorted(v)[len(v) // 2]
    return {"median": round(med, 4), "spread": round((max(v) - min(v)) / med, 4), "blocks": [round(x, 4) for x in v]}


def workload(name, make_model, store, B, blocks, epochs_per_block, dev):
    from equihgnn_amd.fit import BucketedLoader
    from equihgnn_amd.trainer import GraphedTrainStep, with_next

    dstore = store.to_device(dev)
    twin = BucketedLoader(store, B, True, seed=5, device=None)
    batches, tgts = twin.plan()
    twin.close()
    assert len(set(tgts)) == 1 and len(batches[-1]) == B, "one bucket, full batches: every feed replays the same graph"
    resident = [store.collate(b, pad_to=tgts[0]).packed().to(dev) for b in batches]
    for r in resident:
        r.num_real_graphs = B
    torch.manual_seed(0)
    tr = GraphedTrainStep(make_model().to(dev).train(), lr=1e-4)
    loaders = {"host": BucketedLoader(store, B, True, seed=5, device=dev),
               "device": BucketedLoader(dstore, B, True, seed=5)}
    alive, sample = {}, True

    def epoch(feed):
        if feed == "resident":
            for data, nxt in with_next(resident):
                tr.step(data, nxt)
            if sample:
                alive[feed] = threading.active_count()
            return len(resident)
        k = 0
        for data, nxt in with_next(loaders[feed]):
            tr.step(data, nxt)
            k += 1
            if k == 2 and sample:
                alive[feed] = threading.active_count()
        return k

    n = 0
    while n < 48 or tr.calibrating:                  # the capture and the trainer's calibration windows
        tr.step(resident[n % len(resident)])
        n += 1
        assert n < 400, "the trainer's calibration did not end"
    # every ring allocated, every bucket captured.  Threads are counted HERE, the host loader last: once it has run, the
    # producer thread of the epoch it started ahead stays alive through the other feeds' blocks too
    for feed in ("resident", "device", "host"):
        epoch(feed)
    sample = False
    torch.cuda.synchronize()
    graphs = len(tr.slots)
    ms = {f: [] for f in ("resident", "host", "device")}
    cpu = {f: [] for f in ms}
    for _ in range(blocks):
        for feed in ms:
            torch.cuda.synchronize()
            t0, c0, k = time.perf_counter(), time.process_time(), 0
            for _ in range(epochs_per_block):
                k += epoch(feed)
            torch.cuda.synchronize()
            ms[feed].append((time.perf_counter() - t0) * 1e3 / k)
            cpu[feed].append((time.process_time() - c0) / epochs_per_block)
    for ld in loaders.values():
        ld.close()
    res = {"molecules": len(store), "batch": B, "batches_per_epoch": len(batches), "bucket": list(tgts[0]),
           "steps_per_block": epochs_per_block * len(batches), "blocks": blocks,
           "graphs": len(tr.slots), "graphs_captured_while_timed": len(tr.slots) - graphs}
    base = _spread(ms["resident"])["median"]
    for feed in ms:
        s = _spread(ms[feed])
        res[feed] = {"ms_per_step": s["median"], "spread": s["spread"], "ms_per_step_blocks": s["blocks"],
                     "fraction_of_resident": round(base / s["median"], 4),
                     "cpu_seconds_per_epoch": _spread(cpu[feed])["median"],
                     "cpu_seconds_per_epoch_spread": _spread(cpu[feed])["spread"], "threads_alive": alive[feed]}
    res["device_over_host_ms"] = round(res["device"]["ms_per_step"] / res["host"]["ms_per_step"], 4)
    res["device_collate_enqueue_us_per_batch"] = round(loaders["device"].collate_seconds * 1e6 * B
                                                       / max(loaders["device"].collated, 1), 2)
    res["host_collate_us_per_batch"] = round(loaders["host"].collate_seconds * 1e6 * B / max(loaders["host"].collated, 1), 2)
    return res


def lone_collate(store, B, dev, replays=200):
    """The two launches alone in a replayed hipGraph, against the bytes they must move; the host collate and the copy of the
    same batch for scale."""
    dstore = store.to_device(dev)
    idx = np.random.default_rng(3).permutation(len(store))[:B].astype(np.int64)
    ext = store.extents(idx)
    tgt = store.bucket(ext, 128)
    out = dstore.empty_staging(tgt, B + 1)
    didx = torch.from_numpy(idx).to(dev)
    dstore.collate(didx, pad_to=tgt, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dstore.collate(didx, pad_to=tgt, out=out)
    for _ in range(10):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / replays
    host = store.empty_staging(tgt, B + 1, pin=True)
    layout_bytes = sum(int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size() for _, _, shape, dt in host._layout)
    # written: every output element once; read: the real rows' sources once, idx, two offsets per column and molecule, and
    # the prefix the fill searches (counted once: it stays in cache)
    real = store.collate(idx)
    read = sum(getattr(real, n).numel() * getattr(real, n).element_size() for n, *_ in host._layout) + B * 8 * (1 + 4 * len(ext))
    ts = []
    for _ in range(9):
        t0 = time.perf_counter()
        store.collate(idx, pad_to=tgt, out=host)
        ts.append((time.perf_counter() - t0) * 1e6)
    devb = host.to(dev)
    torch.cuda.synchronize()
    a.record()
    for _ in range(50):
        devb._flat.copy_(host._flat, non_blocking=True)
    b.record()
    torch.cuda.synchronize()
    return {"B": B, "extents": list(ext), "bucket": list(tgt), "pair_in_graph_us": round(us, 2),
            "bytes_written": layout_bytes, "bytes_read": int(read),
            "GBps": round((layout_bytes + read) / us * 1e-3, 1), "fraction_of_8TBps": round((layout_bytes + read) / (us * 1e-6) / HBM, 4),
            "host_collate_us": round(sorted(ts)[len(ts) // 2], 2), "h2d_us": round(a.elapsed_time(b) * 1e3 / 50, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--epochs-per-block", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_loader_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_loader: needs a GPU (a device store has no CPU fallback)")
    from equihgnn_amd import hip
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import GraphStore, MolStore, synth_graph, synth_molecule
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    hip.lib()
    dev = torch.device("cuda:0")
    t0 = time.time()
    rng = np.random.default_rng(1234)
    qm9 = MolStore([synth_molecule(rng, "qm9") for _ in range(8192)])
    unique = [synth_graph(rng, "pcqm") for _ in range(768 * 4)]
    pcqm_g = GraphStore(unique * 6)                                  # 24 batches of 768 (a shuffled epoch draws each differently)
    pcqm_h = MolStore([synth_molecule(rng, "pcqm") for _ in range(2048)])
    ns = default_args(method="egnn_equihnns", batch_size=256)
    line = {"tool": "bench_device_loader",
            "timing": "host clock between device synchronisations; one process, interleaved blocks (resident, host, device) "
                      "after one warm epoch per feed; median over blocks, spread = (max - min) / median",
            "cpu_seconds": "time.process_time() of the whole process per epoch (launches included; all threads)"}
    line["egnn_equihnns"] = workload("egnn_equihnns", lambda: MODELS["egnn_equihnns"](1, ns), qm9, 256, a.blocks,
                                     a.epochs_per_block, dev)
    line["gin"] = workload("gin", lambda: GNN_2D(1, gnn_type="gin"), pcqm_g, 768, a.blocks, a.epochs_per_block, dev)
    line["collate_pair_qm9_256"] = lone_collate(qm9, 256, dev)
    line["collate_pair_pcqm_1024"] = lone_collate(pcqm_h, 1024, dev)
    line["wall_s"] = round(time.time() - t0, 1)
    text = json.dumps(line)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
