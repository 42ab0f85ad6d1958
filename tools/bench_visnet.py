#!/usr/bin/env python3
"""Measurement of the ViSNet wrappers (not part of bench.py).  Prints ONE JSON line:

* the visnet_equihnns training step at default_args() (256 QM9-like molecules, hidden 256): replayed (GraphedTrainStep on
  a padded batch) and eager (model(data) -> F.mse_loss -> backward -> torch.optim.Adam), in ms/step and molecules/s;
* every vis_* launch of one EAGER forward + backward, bracketed by in-stream time stamps (ops.Timeline): its time, its
  FLOPs (counted from the kernels' arithmetic per edge slot and channel, KERNEL_COST), and two byte counts from shapes:
    gathered    ops.visnet.edge_bytes: every gathered node row counted once per edge slot that reads it.  Most of these
                reads hit in the caches, so its rate may exceed 8 TB/s; it is a traffic figure, not the bound;
    compulsory  every tensor the launch reads or writes counted once (KERNEL_COST), whose rate against 8 TB/s is the
                fraction of the HBM bound reported as ``frac_hbm_compulsory``;
* the share of that eager step spent in the bracketed dense products of ops.linear (k_gemm_x6 / k_panel_stream launches:
  the forward and input-gradient products; weight gradients run unbracketed in the deferred batch) as
  ``linear_us`` / ``linear_share_of_eager_step``.

    python tools/bench_visnet.py [--steps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM = 8.0e12
# per launch pair: (FLOPs per live edge slot and channel, [N, C]-sized tensors, [16 N, C]-sized tensors) touched once
KERNEL_COST = {
    "k_vis_nbr_fwd": (3, 2, 1), "k_vis_nbr_bwd": (6, 3, 2),
    "k_vis_edge_embed_fwd": (2, 1, 2), "k_vis_edge_embed_bwd": (5, 2, 3),
    "k_vis_attn_fwd": (14, 4, 3), "k_vis_attn_bwd": (40, 7, 5),
    "k_vis_vec_fwd": (32, 16, 2), "k_vis_vec_bwd": (60, 24, 4),
    "k_vis_edge_update_fwd": (85, 16, 2), "k_vis_edge_update_bwd": (250, 32, 3),
}
LINEAR_KERNELS = ("k_gemm_x6", "k_panel_stream")


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


def _index(d):
    from equihgnn_amd.index import HyperIndex
    return HyperIndex.from_batch(d)


def _rbf(model):
    de = model.visnet_layer.representation_model.distance_expansion
    return de.means, de.betas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import equihgnn_amd.models  # noqa: F401
    from equihgnn_amd import ops
    from equihgnn_amd.batch import bucket_sizes, pad_batch, synth_batch
    from equihgnn_amd.registry import default_args, registry
    from equihgnn_amd.trainer import GraphedTrainStep

    dev = torch.device("cuda:0")
    args = default_args(method="visnet_equihnns")
    B = args.batch_size
    b = synth_batch(B, 1234, "qm9")
    cls = registry.get_model_class("visnet_equihnns")
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
    # kernels of one eager step
    ops.TIMELINE = tl = ops.Timeline(dev)
    tl.pair()
    d._hyper_index = None
    eager()
    torch.cuda.synchronize()
    rows = tl.read_us()
    ops.TIMELINE = None
    slot = rows[0][2]
    kern, other, linear = {}, 0.0, 0.0
    N, C = int(b.x.shape[0]), args.MLP_hidden
    live = int(_index(d).radius(d.pos, 5.0, 16, *_rbf(eager_model)).cnt.sum())
    for name, work, us in rows[1:]:
        us = max(us - slot, 1e-3)
        if name.startswith("k_vis"):
            k = kern.setdefault(name, {"us": 0.0, "gathered_bytes": 0, "compulsory_bytes": 0, "flops": 0, "launches": 0})
            k["us"] += us
            k["gathered_bytes"] += work
            fl, nodes, edges = KERNEL_COST.get(name, (0, 0, 0))
            k["flops"] += fl * live * C
            k["compulsory_bytes"] += 4 * C * (nodes * N + edges * 16 * N) + 8 * 16 * N
            k["launches"] += 1
        elif name in LINEAR_KERNELS:
            linear += us
        else:
            other += us
    for k in kern.values():
        t = k["us"] * 1e-6
        k["gathered_tb_s"] = round(k["gathered_bytes"] / t / 1e12, 2)
        k["frac_hbm_compulsory"] = round(k["compulsory_bytes"] / t / HBM, 3)
        k["tflop_s"] = round(k["flops"] / t / 1e12, 2)
        k["us"] = round(k["us"], 2)
    torch.manual_seed(0)
    model = cls(1, args).to(dev).train()
    p = pad_batch(b, *bucket_sizes(b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0])).to(dev)
    tr = GraphedTrainStep(model, lr=1e-4)
    t_graph = _time_ms(lambda: tr.step(p), a.steps, max(a.warmup, 48))
    vis_us = sum(k["us"] for k in kern.values())
    print(json.dumps({"bench": "visnet_equihnns", "molecules": B, "atoms": int(b.x.shape[0]), "hidden": args.MLP_hidden,
                      "replayed_ms": round(t_graph, 4), "replayed_mol_s": round(B / t_graph * 1e3, 1),
                      "eager_ms": round(t_eager, 4), "eager_mol_s": round(B / t_eager * 1e3, 1),
                      "step_measured_for_kernels": "one eager step (stamp-bracketed), not the replayed step",
                      "vis_kernels_us": round(vis_us, 1), "linear_us": round(linear, 1),
                      "linear_share_of_eager_step": round(linear * 1e-3 / t_eager, 3),
                      "other_bracketed_us": round(other, 1), "live_edges": live, "kernels": kern}))


if __name__ == "__main__":
    main()
