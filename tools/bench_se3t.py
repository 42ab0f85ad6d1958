#!/usr/bin/env python3
"""Measurement of ``se3_transformer_equihnns`` (not part of bench.py).  Prints ONE JSON line and writes it to
profiles/se3t_bench.json:

* the training step at default_args() (256 QM9-like molecules, hidden 256): replayed (GraphedTrainStep on a padded batch) and
  eager (model(data) -> F.mse_loss -> backward -> torch.optim.Adam), in ms/step and molecules/s;
* the lone se3t_pair_fwd / se3t_pair_bwd launches at the shapes of ``conv_in`` ((0,0): I = O = hidden, pooled) and of ``to_v``
  (1,1) (I = hidden, O = 64, unpooled) on that batch's neighbour graph, with their FLOPs (2 E MO Q 128 O forward, twice that
  backward) and the bytes of the node matrices they stream.

    python tools/bench_se3t.py [--steps 10] [--warmup 3] [--molecules 256] [--hidden 256]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def _pair_launches(model, d, hidden, steps, warmup):
    from equihgnn_amd import ops
    from equihgnn_amd.index import HyperIndex
    from equihgnn_amd.ops.se3t import SE3T_PAIRS
    from equihgnn_amd.se3_transformer import EdgeBasis
    layer = model.se3_transformer_layer
    geo = EdgeBasis(d.pos, HyperIndex.from_batch(d), layer.k, layer.radius, layer._qtab)
    n, e = geo.N, geo.N * geo.K
    out = {}
    for label, pair, o, pooled in (("conv_in_00", (0, 0), hidden, True), ("to_v_11", (1, 1), 64, False)):
        _, mo, q = SE3T_PAIRS[pair]
        h = torch.randn(e, 128, device=d.pos.device, requires_grad=True)
        g = torch.randn(n, q * 128 * o, device=d.pos.device, requires_grad=True)
        gb = torch.randn(n, q * o, device=d.pos.device, requires_grad=True)
        meanw = geo.meanw if pooled else None
        fwd = lambda: ops.se3t_pair(h, g, gb, geo.basis, pair, o, geo.csr_t.rowptr, geo.csr_t.perm, meanw)
        y = fwd()
        up = torch.randn_like(y)
        t_f = _time_ms(lambda: fwd(), steps, warmup)
        t_fb = _time_ms(lambda: torch.autograd.grad(fwd(), (h, g, gb), up), steps, warmup)
        flops = 2 * e * mo * q * 128 * o
        out[label] = {"pair": list(pair), "O": o, "pooled": pooled, "fwd_us": round(t_f * 1e3, 1),
                      "bwd_us": round((t_fb - t_f) * 1e3, 1), "fwd_tflop_s": round(flops / (t_f * 1e-3) / 1e12, 2),
                      "node_matrix_bytes": 4 * n * q * 128 * o}
    return out, n, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--molecules", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256)
    a = ap.parse_args()
    import equihgnn_amd.models  # noqa: F401
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.registry import default_args, registry
    from equihgnn_amd.trainer import GraphedTrainStep

    dev = torch.device("cuda:0")
    args = default_args(method="se3_transformer_equihnns", MLP_hidden=a.hidden, output_hidden=a.hidden // 2)
    b = synth_batch(a.molecules, 1234, "qm9")
    cls = registry.get_model_class("se3_transformer_equihnns")
    torch.manual_seed(0)
    eager_model = cls(1, args).to(dev).train()
    d = b.to(dev)
    opt = torch.optim.Adam(eager_model.parameters(), lr=1e-4)

    def eager():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(eager_model(d), d.y)
        loss.backward()
        opt.step()

    t_eager = _time_ms(eager, a.steps, a.warmup)
    pairs, n, e = _pair_launches(eager_model, d, a.hidden, a.steps, a.warmup)
    del opt
    torch.manual_seed(0)
    model = cls(1, args).to(dev).train()
    p = pad_batch(b, *bucket_sizes(b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0])).to(dev)
    tr = GraphedTrainStep(model, lr=1e-4)
    t_graph = _time_ms(lambda: tr.step(p), a.steps, max(a.warmup, 4))
    line = json.dumps({"bench": "se3_transformer_equihnns", "molecules": a.molecules, "atoms": n, "edges": e, "hidden": a.hidden,
                       "replayed_ms": round(t_graph, 4), "replayed_mol_s": round(a.molecules / t_graph * 1e3, 1),
                       "eager_ms": round(t_eager, 4), "eager_mol_s": round(a.molecules / t_eager * 1e3, 1),
                       "pair_launches": pairs, "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    print(line)
    with open(os.path.join(ROOT, "profiles", "se3t_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
