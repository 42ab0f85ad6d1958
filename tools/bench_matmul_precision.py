#!/usr/bin/env python3
"""What the matmul precision modes give back (not part of bench.py).  Prints ONE JSON line and writes it to ``--out`` (default
profiles/matmul_precision_bench.json).  Everything is timed in ONE process, "highest" beside the reduced modes:

* three dense products through ``ops.gemm`` -- FAFormer's [246 k x 256].[256 x 256] (x W^T), the Equiformer's
  [2432 x 256].[256 x 16384] (x W^T) and a K = 2052 input gradient dY W, [36864 x 2052].[2052 x 256] -- per mode and, for the
  reduced modes, per ring depth (EQH_BF16_RING=deep: the LDS that fewer planes free spent on a deeper ring).  Each variant is
  captured as a hipGraph of ``REPS`` launches; after a warm-up the graphs are replayed in interleaved blocks (variant 1, 2, ..,
  1, 2, ..) between device events.  Per variant: the median block in microseconds per launch, ``spread`` = (max - min) / median
  of its blocks, and ``vs_highest`` = its median / the median of "highest";
* the replayed training step (GraphedTrainStep) of ``equiformer_equihnns`` (QM9-like, batch 128) and ``faformer_equihnns``
  (PCQM-like, batch 512) per mode: one trainer, the mode switched between interleaved blocks (the trainer keys its graphs by
  the mode, so each mode replays its own capture).

``verdict`` says, per shape and mode, whether the mode is faster than "highest" by more than the two spreads.

    python tools/bench_matmul_precision.py [--blocks 7] [--steps 10] [--warmup 5] [--skip-steps]

``--panels`` times what ``set_float32_matmul_precision(mode, panels=True)`` gives instead (default output
profiles/panel_precision_bench.json), in the same way: a lone [4864 x 256].[256 x 256] row-panel product (ops.panel_gemm) with
6 / 3 / 1 products, each with an image of exactly its planes and with the three-plane image, and the replayed training step of
``egnn_equihnns`` and ``mhnnm`` (batch 256, hidden 256) under the ``--variants`` (default "highest", "medium" without the flag,
"high+panels", "medium+panels"), interleaved in one process.  ``--merge [NAME=]FILE`` (repeatable) adds the result of another
run of this tool on the same box under NAME (default ``other_build``): the same script run from a checkout of an earlier
commit, with the variants that commit knows; a run with ``--full-images``, under which the operators pack three-plane images
in every mode (the A/B of the reduced-plane images at step level); or a run against another build of the library
(EQH_LIB_PATH).  ``--rows`` lists the row counts of the lone product.

    python tools/bench_matmul_precision.py --panels [--variants highest,medium] [--rows 4864,16384] [--skip-products]
                                           [--full-images] [--merge [NAME=]FILE]

``--wgrads`` times what ``set_float32_matmul_precision(mode, wgrads=True)`` gives (default output
profiles/wgrad_precision_bench.json), again in one process on replayed graphs: the lone batched weight-gradient launch
(ops.wgrad_batch between defer_begin and defer_flush: the launch and its one slab reduction) at the two shapes of the BASELINE
batch -- 21 products of [4736 x 256]^T [4736 x 256], which take the 128 x 128 form, and 30, which take the 128 x 256 form -- with
6 / 3 / 1 products; and the replayed training step of ``egnn_equihnns`` and ``mhnnm`` (batch 256, hidden 256) under
highest / high / medium with ``panels=True`` alone and with ``panels=True, wgrads=True`` (``--variants`` replaces the list; the
first is the ratios' base).  ``pairs`` compares each ``mode+panels+wgrads`` with its ``mode+panels`` -- the arithmetic of the
commit before the flag -- beyond both spreads; ``--merge`` adds that commit's own build timed by its own copy of this tool.

    python tools/bench_matmul_precision.py --wgrads [--variants ...] [--skip-products] [--skip-steps] [--merge [NAME=]FILE]

``--edges`` times what ``set_float32_matmul_precision(mode, edges=True)`` gives (default output
profiles/edge_precision_bench.json), in one process on replayed graphs: the lone forward launch of the fused EGNN edge update
(egnn_edge_fwd_p) and its lone backward (egnn_edge_bwd_p: prep + receiver pass + sender pass + the slab reductions) at
N = 4608 / Hp = 1088 (the BASELINE batch) and N = 29696 / Hp = 1088 (batch 1024), the neighbours a kNN over one cloud of the whole
batch as in the model, with 6 / 3 / 1 products; and the replayed training step of ``egnn_equihnns`` (batch 256, hidden 256)
under highest, medium, medium+edges and medium+panels+wgrads+edges.  ``pairs`` compares each variant with ``+edges`` with the
same variant without it, where that was timed, beyond both spreads; ``--merge`` adds the flag-off rows of the commit before the
flag, timed by its own copy of this tool (``--wgrads --variants highest,medium --skip-products``).

    python tools/bench_matmul_precision.py --edges [--variants ...] [--skip-products] [--skip-steps] [--merge [NAME=]FILE]
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
MODES = ("highest", "high", "medium")
SHAPES = {"faformer_246k_256_256": (245760, 256, 256, True), "equiformer_2432_256_16384": (2432, 16384, 256, True),
          "dyW_36864_2052_256": (36864, 256, 2052, False)}


def _stat(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def gemm_times(a, dev):
    import equihgnn_amd
    from equihgnn_amd import hip, ops
    res = {}
    for name, (M, N, K, tb) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        x = torch.randn(M, K, generator=g).to(dev)
        w = torch.randn((N, K) if tb else (K, N), generator=g).to(dev)
        out = torch.empty(M, N, device=dev)
        graphs = {}
        for mode in MODES:
            for ring in (("base",) if mode == "highest" else ("base", "deep")):
                equihgnn_amd.set_float32_matmul_precision(mode)
                os.environ["EQH_BF16_RING"] = ring
                for _ in range(3):
                    ops.gemm(x, w, trans_b=tb, out=out)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(REPS):
                        ops.gemm(x, w, trans_b=tb, out=out)
                graphs[mode if ring == "base" else mode + "_deep_ring"] = gr
        equihgnn_amd.set_float32_matmul_precision("highest")
        os.environ.pop("EQH_BF16_RING", None)
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
        pr = (hip.HgGemmProblem * 1)()
        pr[0].m, pr[0].n, pr[0].k, pr[0].trans_b = M, N, K, int(tb)
        entry = {"m": M, "n": N, "k": K, "b_is_n_by_k": tb, "tile": int(hip.lib().hg_gemm_x6_choose_tile(1, pr, 1))}
        base, base_sp = _stat(times["highest"])
        for k, ts in times.items():
            med, sp = _stat(ts)
            entry[k] = {"us": round(med, 2), "spread": round(sp, 4), "vs_highest": round(med / base, 4),
                        "tflops_fp32_equivalent": round(2.0 * M * N * K / med / 1e6, 1),
                        "faster_than_highest_beyond_spread": bool(med * (1 + sp) < base * (1 - base_sp))}
        res[name] = entry
        del graphs, x, w, out
        gc.collect()
        torch.cuda.empty_cache()
    return res


def _set_mode(variant):
    import equihgnn_amd
    mode, *flags = variant.split("+")
    unknown = set(flags) - {"panels", "wgrads", "edges"}
    if unknown:
        raise SystemExit(f"unknown flag(s) {sorted(unknown)} in variant {variant!r}")
    equihgnn_amd.set_float32_matmul_precision(mode, **{f: True for f in flags})


def panel_product_times(a, dev, rows=4864, C=256):
    """a lone row-panel product under 6 / 3 / 1 products: hipGraphs of REPS launches, interleaved blocks between device events"""
    from equihgnn_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, C, generator=g).to(dev)
    w = (torch.randn(C, C, generator=g) * C ** -0.5).to(dev)
    out = torch.empty(rows, C, device=dev)
    graphs, keep = {}, []
    for products, planes in ((6, 3), (3, 2), (3, 3), (1, 1), (1, 3)):
        (img,) = ops.panel_pack([(w, True)], planes=planes)
        keep.append(img)
        for _ in range(3):
            ops.panel_gemm(x, img, C, out=out, products=products)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(REPS):
                ops.panel_gemm(x, img, C, out=out, products=products)
        graphs[f"products_{products}_image_planes_{planes}"] = gr
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
    entry = {"rows": rows, "C": C, "panels": (rows + 31) // 32}
    base, base_sp = _stat(times["products_6_image_planes_3"])
    for k, ts in times.items():
        med, sp = _stat(ts)
        entry[k] = {"us": round(med, 2), "spread": round(sp, 4), "vs_six_products": round(med / base, 4),
                    "faster_than_six_products_beyond_spread": bool(med * (1 + sp) < base * (1 - base_sp))}
    return entry


def step_times(method, batch, flavour, seed0, a, dev, variants=MODES, hidden=None):
    import equihgnn_amd
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.models import MODELS
    from equihgnn_amd.registry import default_args
    from equihgnn_amd.trainer import GraphedTrainStep
    pool = 4
    ns = default_args(method=method, batch_size=batch, **({} if hidden is None else {"MLP_hidden": hidden}))
    host = [synth_batch(batch, seed0 + i, flavour) for i in range(pool)]
    torch.manual_seed(0)
    model = MODELS[method](1, ns).to(dev).train()
    ext = [bucket_sizes(b.num_nodes, b.num_hyperedges, b.nnz) for b in host]
    tgt = tuple(max(e[i] for e in ext) for i in range(3))
    batches = [pad_batch(b, *tgt).packed().to(dev) for b in host]
    for b in batches:
        b.num_real_graphs = batch
    tr = GraphedTrainStep(model, lr=ns.lr, weight_decay=ns.wd)
    n = [0]

    def step():
        tr.step(batches[n[0] % pool], batches[(n[0] + 1) % pool])
        n[0] += 1

    for _ in range(2):
        step()
    while getattr(tr, "calibrating", False):          # the trainer settles the form of its index build under "highest"
        step()
    for mode in variants:                             # each mode's capture and warm-up
        _set_mode(mode)
        for _ in range(1 + a.warmup):
            step()
    times = {m: [] for m in variants}
    for _ in range(a.blocks):
        for mode in variants:
            _set_mode(mode)
            step()                                    # (the first step after a switch is not timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
    equihgnn_amd.set_float32_matmul_precision("highest")
    out = {"molecules": batch, "flavour": flavour, "hidden": ns.MLP_hidden, "graphs": len(tr.slots)}
    base, base_sp = _stat(times["highest" if "highest" in times else variants[0]])
    for mode, ts in times.items():
        med, sp = _stat(ts)
        out[mode] = {"ms": round(med, 4), "spread": round(sp, 4), "vs_highest": round(med / base, 4),
                     "faster_than_highest_beyond_spread": bool(med * (1 + sp) < base * (1 - base_sp))}
    tr.close()
    del tr, model, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def wgrad_launch_times(a, dev, count, K=4736, C=256):
    """`count` products of [K x C]^T [K x C] in one batched launch (+ its one deferred slab reduction) under 6 / 3 / 1 products:
    hipGraphs of REPS launches, interleaved blocks between device events"""
    import equihgnn_amd
    from equihgnn_amd import hip, ops
    g = torch.Generator().manual_seed(0)
    dys = [torch.randn(K, C, generator=g).to(dev) for _ in range(count)]
    xs = [torch.randn(K, C, generator=g).to(dev) for _ in range(count)]
    outs = [torch.zeros(C, C, device=dev) for _ in range(count)]
    entries = [(dy, x, 1e-3, o) for dy, x, o in zip(dys, xs, outs)]

    def launch():
        ops.defer_begin(dev)
        ops.wgrad_batch(entries)
        ops.defer_flush(dev)

    graphs = {}
    for mode in MODES:
        equihgnn_amd.set_float32_matmul_precision(mode, wgrads=True)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(REPS):
                launch()
        graphs[mode] = gr
    equihgnn_amd.set_float32_matmul_precision("highest")
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
    ws = int(hip.lib().hg_wgrad_batch_workspace_bytes(count, C, C))
    entry = {"count": count, "K": K, "O": C, "I": C, "chunks_of_K": ws // (count * C * C * 4),
             "form_by_the_dispatch_rule": "128 x 256" if C % 256 == 0 and (C // 128) * (C // 256) * min(count, 64) * 5 >= 256 else "128 x 128"}
    base, base_sp = _stat(times["highest"])
    for k, ts in times.items():
        med, sp = _stat(ts)
        entry[k] = {"us": round(med, 2), "spread": round(sp, 4), "vs_highest": round(med / base, 4),
                    "tflops_fp32_equivalent": round(2.0 * count * K * C * C / med / 1e6, 1),
                    "faster_than_highest_beyond_spread": bool(med * (1 + sp) < base * (1 - base_sp))}
    del graphs, dys, xs, outs, entries
    gc.collect()
    torch.cuda.empty_cache()
    return entry


def edge_launch_times(a, dev, N, Hp=1088):
    """the lone forward launch and the lone backward of the fused EGNN edge update under 6 / 3 / 1 products: hipGraphs of REPS
    launches, interleaved blocks between device events"""
    import ctypes
    from equihgnn_amd import hip, ops
    L = hip.lib()
    g = torch.Generator().manual_seed(0)
    ab = torch.randn(N, 2 * Hp, generator=g).to(dev)
    wd = (torch.randn(Hp, generator=g) * 0.3).to(dev)
    w2 = (torch.randn(16, Hp, generator=g) / Hp ** 0.5).to(dev)
    b2 = (torch.randn(16, generator=g) * 0.1).to(dev)
    dm = torch.randn(N, 16, generator=g).to(dev)
    nbr, d2 = ops.knn((torch.randn(N, 3, generator=g) * 2).to(dev), 16, 0)      # one cloud: the kNN ignores molecule boundaries
    nbr, d2 = nbr.int().contiguous(), d2.contiguous()
    csr_t = ops.csr_build(nbr.reshape(-1).long(), None, N)
    m, pre2 = torch.empty(N, 16, device=dev), torch.empty(N, 16, 16, device=dev)
    dab, dwd, dw2 = torch.empty(N, 2 * Hp, device=dev), torch.empty(Hp, device=dev), torch.empty(16, Hp, device=dev)
    dpre2, db2 = torch.empty(N, 16, 16, device=dev), torch.empty(16, device=dev)
    ws_bytes = L.egnn_edge_bwd_workspace_bytes(N, Hp)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def forward(products):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        hip.check(L.egnn_edge_fwd_p(p(ab), p(wd), p(w2), p(b2), p(nbr), p(d2), N, Hp, p(m), p(pre2), st, products), "egnn_edge_fwd_p")

    def backward(products):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        hip.check(L.egnn_edge_bwd_p(p(ab), p(wd), p(w2), p(nbr), p(d2), p(pre2), p(dm), 16, p(csr_t.rowptr), p(csr_t.perm), N, Hp,
                                    p(dab), p(dwd), p(dw2), p(dpre2), p(db2), 0, 0, p(ws), ws_bytes, st, products), "egnn_edge_bwd_p")

    forward(6)
    graphs = {}
    for what, fn in (("forward", forward), ("backward", backward)):
        for products in (6, 3, 1):
            for _ in range(3):
                fn(products)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(REPS):
                    fn(products)
            graphs[what, products] = gr
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
    entry = {"N": N, "Hp": Hp, "forward": {}, "backward": {}}
    for what in ("forward", "backward"):
        base, base_sp = _stat(times[what, 6])
        for products in (6, 3, 1):
            med, sp = _stat(times[what, products])
            entry[what][f"products_{products}"] = {"us": round(med, 2), "spread": round(sp, 4), "vs_six_products": round(med / base, 4),
                                                   "faster_than_six_products_beyond_spread": bool(med * (1 + sp) < base * (1 - base_sp))}
    del graphs, ab, dab, ws
    gc.collect()
    torch.cuda.empty_cache()
    return entry


def main_edges(a, dev):
    variants = tuple(v for v in a.variants.split(",") if v)
    result = {"bench": "edge_precision", "device": torch.cuda.get_device_name(0),
              "timing": f"launches: hipGraphs of {REPS} x (the forward launch | prep + receiver + sender pass + slab reductions), {a.blocks} "
                        f"interleaved blocks of {a.inner} replays between device events; steps: {a.blocks} interleaved blocks of {a.steps} "
                        "replayed steps on a host clock; median block, spread = (max - min) / median",
              "variants": "mode[+panels][+wgrads][+edges]: set_float32_matmul_precision(mode, panels=..., wgrads=..., edges=...); without "
                          "+edges the edge kernels keep six products (the arithmetic of the commit before the flag)",
              "steps": {}}
    if not a.skip_products:
        result["edge_4608_1088"] = edge_launch_times(a, dev, 4608)
        result["edge_29696_1088"] = edge_launch_times(a, dev, 29696)
    if not a.skip_steps:
        result["steps"]["egnn_equihnns_b256_h256"] = step_times("egnn_equihnns", 256, "qm9", 1000, a, dev, variants, hidden=256)
        pairs = {}
        for name, e in result["steps"].items():
            for v in variants:
                off = v.replace("+edges", "")
                if v != off and off in e:
                    pairs[f"{name}/{v}"] = {"vs": off, "ratio": round(e[v]["ms"] / e[off]["ms"], 4),
                                            "faster_beyond_both_spreads": bool(e[v]["ms"] * (1 + e[v]["spread"]) <
                                                                               e[off]["ms"] * (1 - e[off]["spread"]))}
        result["pairs"] = pairs
    for item in a.merge:
        name, _, path = item.rpartition("=")
        with open(path) as f:
            result[name or "other_build"] = json.loads(f.readline())
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


def main_wgrads(a, dev):
    variants = tuple(v for v in a.variants.split(",") if v)
    result = {"bench": "wgrad_precision", "device": torch.cuda.get_device_name(0),
              "timing": f"launch: hipGraphs of {REPS} x (batched launch + its slab reduction), {a.blocks} interleaved blocks of {a.inner} "
                        f"replays between device events; steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host "
                        "clock; median block, spread = (max - min) / median",
              "variants": "mode[+panels][+wgrads]: set_float32_matmul_precision(mode, panels=..., wgrads=...); without +wgrads the "
                          "batched weight gradients keep six products (the arithmetic of the commit before the flag)",
              "steps": {}}
    if not a.skip_products:
        result["wgrad_batch_21_x_4736_256_256"] = wgrad_launch_times(a, dev, 21)
        result["wgrad_batch_30_x_4736_256_256"] = wgrad_launch_times(a, dev, 30)
    if not a.skip_steps:
        result["steps"]["egnn_equihnns_b256_h256"] = step_times("egnn_equihnns", 256, "qm9", 1000, a, dev, variants, hidden=256)
        result["steps"]["mhnnm_b256_h256"] = step_times("mhnnm", 256, "qm9", 2000, a, dev, variants, hidden=256)
        pairs = {}
        for name, e in result["steps"].items():
            for v in variants:
                off = v.replace("+wgrads", "")
                if v != off and off in e:
                    pairs[f"{name}/{v}"] = {"vs": off, "ratio": round(e[v]["ms"] / e[off]["ms"], 4),
                                            "faster_beyond_both_spreads": bool(e[v]["ms"] * (1 + e[v]["spread"]) <
                                                                               e[off]["ms"] * (1 - e[off]["spread"]))}
        result["pairs"] = pairs
    for item in a.merge:
        name, _, path = item.rpartition("=")
        with open(path) as f:
            result[name or "other_build"] = json.loads(f.readline())
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


def main_panels(a, dev):
    variants = tuple(v for v in a.variants.split(",") if v)
    if variants[0] != "highest":
        raise SystemExit("--variants must start with highest (the ratios' base)")
    result = {"bench": "panel_precision", "device": torch.cuda.get_device_name(0),
              "timing": f"product: hipGraphs of {REPS} launches, {a.blocks} interleaved blocks of {a.inner} replays between device events; "
                        f"steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock; median block, "
                        "spread = (max - min) / median",
              "variants": "mode[+panels]: set_float32_matmul_precision(mode, panels=...); without +panels the panel kernels keep six products",
              "steps": {}}
    if a.full_images:
        from equihgnn_amd.ops import panel
        panel.FULL_IMAGES = True
        result["images"] = "three planes in every mode (--full-images)"
    if os.environ.get("EQH_LIB_PATH"):
        result["library"] = os.path.basename(os.environ["EQH_LIB_PATH"])
    if not a.skip_products:
        for rows in (int(r) for r in a.rows.split(",")):
            result[f"panel_product_{rows}_256_256"] = panel_product_times(a, dev, rows=rows)
    if not a.skip_steps:
        result["steps"]["egnn_equihnns_b256_h256"] = step_times("egnn_equihnns", 256, "qm9", 1000, a, dev, variants, hidden=256)
        result["steps"]["mhnnm_b256_h256"] = step_times("mhnnm", 256, "qm9", 2000, a, dev, variants, hidden=256)
    for item in a.merge:
        name, _, path = item.rpartition("=")
        with open(path) as f:
            result[name or "other_build"] = json.loads(f.readline())
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="graph replays (of REPS launches) per timed block of a product")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--panels", action="store_true", help="time the panel kernels' modes instead (see the module docstring)")
    ap.add_argument("--wgrads", action="store_true", help="time the batched weight gradients' modes instead (see the module docstring)")
    ap.add_argument("--edges", action="store_true", help="time the EGNN edge kernels' modes instead (see the module docstring)")
    ap.add_argument("--variants", default=None)
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--rows", default="4864", help="row counts of the lone panel product (--panels)")
    ap.add_argument("--full-images", action="store_true", help="the operators pack three-plane images in every mode (--panels)")
    ap.add_argument("--merge", action="append", default=[], metavar="[NAME=]FILE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.variants is None:
        a.variants = ("highest,medium,medium+edges,medium+panels+wgrads+edges" if a.edges else
                      "highest+panels,high+panels,medium+panels,highest+panels+wgrads,high+panels+wgrads,medium+panels+wgrads"
                      if a.wgrads else "highest,medium,high+panels,medium+panels")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "edge_precision_bench.json" if a.edges else "wgrad_precision_bench.json" if a.wgrads else
                             "panel_precision_bench.json" if a.panels else "matmul_precision_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_matmul_precision: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    if a.edges:
        return main_edges(a, dev)
    if a.wgrads:
        return main_wgrads(a, dev)
    if a.panels:
        return main_panels(a, dev)
    result = {"bench": "matmul_precision", "device": torch.cuda.get_device_name(0),
              "timing": f"products: hipGraphs of {REPS} launches, {a.blocks} interleaved blocks of {a.inner} replays between device events; "
                        f"steps: {a.blocks} interleaved blocks of {a.steps} replayed steps on a host clock; median block, "
                        "spread = (max - min) / median",
              "products": gemm_times(a, dev), "steps": {}}
    if not a.skip_steps:
        result["steps"]["c3_equiformer_equihnns_b128"] = step_times("equiformer_equihnns", 128, "qm9", 3000, a, dev)
        result["steps"]["c5_faformer_equihnns_b512"] = step_times("faformer_equihnns", 512, "pcqm", 5000, a, dev)
    result["verdict"] = {
        **{f"{s}/{m}": ("faster" if e[m]["faster_than_highest_beyond_spread"] else "not faster beyond the spread: six products would do")
           for s, e in result["products"].items() for m in e if isinstance(e[m], dict) and m != "highest"},
        **{f"{s}/{m}": ("faster" if e[m]["faster_than_highest_beyond_spread"] else "not faster beyond the spread")
           for s, e in result["steps"].items() for m in ("high", "medium")}}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
