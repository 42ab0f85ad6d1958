#!/usr/bin/env python3
"""Measurement of the 2-D baselines gin / gcn (not part of bench.py).  Prints ONE JSON line:

* the training step at scripts/run_pcqm.sh's size (768 PCQM-like molecules, width 300, 5 layers): replayed
  (GraphedTrainStep on a padded batch) and eager (model(data) -> F.mse_loss -> backward -> torch.optim.Adam), in ms/step and
  molecules/s;
* hg_edge_msg_fwd / hg_edge_msg_bwd stand-alone at that size and at a cache-exceeding one (2^20 atoms, C = 300: a 1.26 GB
  feature matrix), as a fraction of 8 TB/s in algorithmic bytes, in two forms:
    per-edge    SURVEY.md §8d's segment-reduce count (ops.gnn2d.edge_msg_bytes): every message gathers its source row,
                bond-table reads counted as zero bytes (LDS in the forward, cache-resident in the backward);
    compulsory  every [N, C] matrix read or written once (fwd: x, out; bwd: x, dout, dx) plus the index arrays.

    python tools/bench_gnn2d.py [--steps 20] [--warmup 5] [--big-atoms 1048576]

With --pipeline it measures the data path instead (and writes the line to --out, profiles/gnn2d_pipeline.json): gin and gcn
at the same size, the replayed step on RESIDENT padded batches against the same trainer FED by fit.BucketedLoader over a
batch.GraphStore (one batch of look-ahead, as Fitter.fit drives it), in alternating blocks of one epoch each; plus the host
time per batch of the native collate (gb_collate) and of its restatement collate_graphs + pad_graph_batch.

    python tools/bench_gnn2d.py --pipeline [--blocks 8] [--epoch-batches 24] [--out profiles/gnn2d_pipeline.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM = 8.0e12


def _time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def model_steps(gnn_type, B, steps, warmup, dev):
    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import graph_bucket_sizes, pad_graph_batch, synth_graph_batch
    from equihgnn_amd.trainer import GraphedTrainStep

    b = synth_graph_batch(B, 1234, "pcqm")
    torch.manual_seed(0)
    eager_model = GNN_2D(1, gnn_type=gnn_type).to(dev).train()
    d = b.to(dev)
    opt = torch.optim.Adam(eager_model.parameters(), lr=1e-4)

    def eager():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(eager_model(d), d.y)
        loss.backward()
        opt.step()

    t_eager = _time_ms(eager, steps, warmup)
    torch.manual_seed(0)
    model = GNN_2D(1, gnn_type=gnn_type).to(dev).train()
    p = pad_graph_batch(b, *graph_bucket_sizes(b.num_nodes, b.num_edges)).to(dev)
    tr = GraphedTrainStep(model, lr=1e-4)
    # (warm-up past the trainer's set-up: the capture and its ~32-step calibration of the index-build placement)
    t_graph = _time_ms(lambda: tr.step(p), steps, max(warmup, 48))
    return {"atoms": b.num_nodes, "edges": b.num_edges,
            "replayed_ms": round(t_graph, 4), "replayed_mol_s": round(B / t_graph * 1e3, 1),
            "eager_ms": round(t_eager, 4), "eager_mol_s": round(B / t_eager * 1e3, 1)}


def kernels(N, E_per_atom, C, steps, warmup, dev):
    from equihgnn_amd.ops.gnn2d import GCN, GIN, GraphIndex, edge_msg_bytes
    from equihgnn_amd import hip
    from equihgnn_amd.ops._base import _ptr, _stream

    g = torch.Generator(device=dev).manual_seed(0)
    E = int(N * E_per_atom)
    src = torch.randint(0, N, (E,), device=dev, generator=g)
    # local molecules of ~30 atoms: the target is near the source, as in a batch of molecules
    dst = (src + torch.randint(-15, 16, (E,), device=dev, generator=g)).clamp(0, N - 1)
    attr = torch.stack([torch.randint(0, d, (E,), device=dev, generator=g) for d in (5, 6, 2)], 1)
    gi = GraphIndex(torch.stack((src, dst)), attr, torch.zeros(N, dtype=torch.int64, device=dev), N, 1)
    x = torch.randn(N, C, device=dev, generator=g)
    tabs = torch.randn(gi.T, C, device=dev, generator=g)
    eps = torch.full((1,), 0.1, device=dev)
    root = torch.randn(1, C, device=dev, generator=g)
    out = torch.empty_like(x)
    dout = torch.randn(N, C, device=dev, generator=g)
    dx = torch.empty_like(x)
    dtab = torch.empty_like(tabs)
    dextra = torch.empty(C, device=dev)
    L = hip.lib()
    ws_bytes = L.hg_edge_msg_bwd_workspace_bytes(N, C, gi.T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = _stream(dev)
    res = {"atoms": N, "edges": E, "C": C}
    comp_idx = 4 * (N + 1) + 8 * E
    for name, mode, param in (("gin", GIN, eps), ("gcn", GCN, root)):
        e_, r_ = (param, None) if mode == GIN else (None, param)

        def fwd():
            hip.check(L.hg_edge_msg_fwd(mode, _ptr(x), _ptr(tabs), gi.T, gi.F, _ptr(gi.by_dst.rowptr), _ptr(gi.src_of_dst),
                                        _ptr(gi.code_dst), _ptr(gi.by_src.rowptr), _ptr(e_), _ptr(r_), N, C, _ptr(out), st),
                      "fwd")

        def bwd():
            hip.check(L.hg_edge_msg_bwd(mode, _ptr(x), _ptr(tabs), gi.T, gi.F, _ptr(gi.by_src.rowptr), _ptr(gi.dst_of_src),
                                        _ptr(gi.code_src), _ptr(e_), _ptr(r_), _ptr(dout), N, C, _ptr(dx), _ptr(dtab),
                                        _ptr(dextra), 0, _ptr(ws), ws_bytes, st), "bwd")

        for kname, fn, per_edge, compulsory in (
                ("fwd", fwd, edge_msg_bytes(E, N, C, False), 8 * C * N + comp_idx),
                ("bwd", bwd, edge_msg_bytes(E, N, C, True), 12 * C * N + comp_idx)):
            ms = _time_ms(fn, steps, warmup)
            res[f"{name}_{kname}_us"] = round(ms * 1e3, 2)
            res[f"{name}_{kname}_frac_per_edge"] = round(per_edge / (ms * 1e-3) / HBM, 3)
            res[f"{name}_{kname}_frac_compulsory"] = round(compulsory / (ms * 1e-3) / HBM, 3)
    return res


def _median_ms(fn, runs=7):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def pipeline(B, blocks, epoch_batches, dev):
    """Resident against loader-fed steps of ONE trainer per model, in alternating blocks of one epoch (host clock between two
    device synchronisations: the loader's copies run on a stream of their own, so no single stream's events see a step)."""
    import numpy as np

    from equihgnn_amd.baseline_2d import GNN_2D
    from equihgnn_amd.batch import GBatch, GraphStore, collate_graphs, pad_graph_batch, synth_graph
    from equihgnn_amd.fit import BucketedLoader
    from equihgnn_amd.trainer import GraphedTrainStep, with_next

    rng = np.random.default_rng(1234)
    unique = [synth_graph(rng, "pcqm") for _ in range(B * 4)]
    reps = -(-epoch_batches // 4)
    mols = unique * reps                                         # (a shuffled epoch still draws every batch differently)
    store = GraphStore(mols)
    twin = BucketedLoader(store, B, True, seed=5, device=None)
    batches, tgts = twin.plan()
    twin.close()
    tgt = tgts[0]
    assert len(set(tgts)) == 1, "one bucket per run is what the loader's default plans"
    # host: the native collate into a pinned packed buffer against the restatement, one thread, same batch
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    host = GBatch.empty_packed(tgt[0], tgt[1], store.F, B + 1, pin=True)
    idx = batches[0]
    res = {"molecules": len(store), "batches_per_epoch": len(batches), "bucket_atoms": tgt[0], "bucket_edges": tgt[1],
           "batch_bytes": int(host._flat.numel()),
           "real_atoms_mean": round(float(np.mean([store.extents(b)[0] for b in batches])), 1),
           "real_edges_mean": round(float(np.mean([store.extents(b)[1] for b in batches])), 1),
           "gb_collate_ms": round(_median_ms(lambda: store.collate(idx, pad_to=tgt, out=host)), 4),
           "collate_graphs_ms": round(_median_ms(lambda: collate_graphs([mols[int(i)] for i in idx])), 4)}
    plain = collate_graphs([mols[int(i)] for i in idx])
    res["pad_graph_batch_ms"] = round(_median_ms(lambda: pad_graph_batch(plain, *tgt)), 4)
    torch.set_num_threads(threads)
    # the host-to-device copy of one packed batch, alone on the device
    devb = host.to(dev)
    res["h2d_ms"] = round(_time_ms(lambda: devb._flat.copy_(host._flat, non_blocking=True), 20, 5), 4)
    resident = [store.collate(b, pad_to=tgt).to(dev) for b in batches]
    for gnn_type in ("gin", "gcn"):
        torch.manual_seed(0)
        model = GNN_2D(1, gnn_type=gnn_type).to(dev).train()
        tr = GraphedTrainStep(model, lr=1e-4)
        loader = BucketedLoader(store, B, True, seed=5, device=dev, prefetch=3)
        n = 0
        while n < 48 or tr.calibrating:                          # the capture and the trainer's calibration windows
            tr.step(resident[n % len(resident)])
            n += 1
            assert n < 400, "the trainer's calibration did not end"
        for data, nxt in with_next(loader):                      # one epoch through the loader: pinned ring, side stream
            tr.step(data, nxt)
        torch.cuda.synchronize()
        graphs = len(tr.slots)
        t_res, t_fed, t_load = [], [], []
        for _ in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for data in resident:
                tr.step(data)
            torch.cuda.synchronize()
            t_res.append((time.perf_counter() - t0) * 1e3 / len(resident))
            t0 = time.perf_counter()
            k = 0
            for data, nxt in with_next(loader):
                tr.step(data, nxt)
                k += 1
            torch.cuda.synchronize()
            t_fed.append((time.perf_counter() - t0) * 1e3 / k)
            assert k == len(resident)
        for _ in range(3):                                       # the loader alone: collate + copy per batch, nothing to feed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = sum(1 for _ in loader)
            torch.cuda.synchronize()
            t_load.append((time.perf_counter() - t0) * 1e3 / k)
        loader.close()
        med = lambda v: sorted(v)[len(v) // 2]
        res[gnn_type] = {
            "resident": {"ms_per_step": round(med(t_res), 4), "min": round(min(t_res), 4), "max": round(max(t_res), 4)},
            "loader_fed": {"ms_per_step": round(med(t_fed), 4), "min": round(min(t_fed), 4), "max": round(max(t_fed), 4)},
            "fraction_of_resident": round(med(t_res) / med(t_fed), 4),
            "fraction_per_block": [round(a / b, 4) for a, b in zip(t_res, t_fed)],
            "loader_alone_ms_per_batch": round(med(t_load), 4),
            "loader_collate_ms_per_batch": round(loader.collate_seconds * 1e3 / max(loader.collated, 1) * B, 4),
            "graphs_captured_while_timed": len(tr.slots) - graphs, "graphs": len(tr.slots),
            "warmup_steps": n + len(resident), "timed_steps_per_form": blocks * len(resident),
            "mol_s_loader_fed": round(B / med(t_fed) * 1e3, 1)}
        del tr, model, loader
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=768)
    ap.add_argument("--big-atoms", type=int, default=1 << 20)
    ap.add_argument("--pipeline", action="store_true", help="measure the loader-fed step instead (see the module docstring)")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--epoch-batches", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn2d_pipeline.json"))
    a = ap.parse_args()
    from equihgnn_amd import hip
    hip.lib()
    dev = torch.device("cuda:0")
    t0 = time.time()
    if a.pipeline:
        line = {"tool": "bench_gnn2d --pipeline", "batch": a.batch, "width": 300, "layers": 5, "blocks": a.blocks,
                "timing": "host clock between device synchronisations, alternating blocks of one epoch; medians, min, max",
                **pipeline(a.batch, a.blocks, a.epoch_batches, dev)}
        line["wall_s"] = round(time.time() - t0, 1)
        text = json.dumps(line)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        print(text)
        return
    line = {"tool": "bench_gnn2d", "batch": a.batch, "width": 300, "layers": 5, "steps": a.steps,
            "bytes_formula": {"per_edge": "fwd 4C*E + 8E + 4(N+1) + 8C*N; bwd + 4C*N (bond-table reads: 0)",
                              "compulsory": "fwd 8C*N, bwd 12C*N, + 4(N+1) + 8E"},
            "hbm_peak_Bps": HBM}
    for t in ("gin", "gcn"):
        line[t] = model_steps(t, a.batch, a.steps, a.warmup, dev)
    n_run = line["gin"]["atoms"]
    line["kernels_run_pcqm"] = kernels(n_run, line["gin"]["edges"] / n_run, 300, a.steps, a.warmup, dev)
    line["kernels_cache_exceeding"] = kernels(a.big_atoms, line["gin"]["edges"] / n_run, 300, max(a.steps // 4, 3),
                                              2, dev)
    line["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
