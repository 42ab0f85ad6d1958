#!/usr/bin/env python3
"""Golden vectors of the ViSNet wrappers ``visnet_equihnn`` / ``visnet_equihnns`` / ``visnet_equihnnm``: the REFERENCE's
own equihgnn/models/equihnn_visnet.py and equihgnn/models/layers/visnet_layer.py (read from the reference checkout at run
time, never copied) run on small seeded batches.

    python tests/golden/make_golden_visnet.py            # (re)write tests/golden/visnet/*.npz
    python tests/golden/make_golden_visnet.py --check    # regenerate and compare bit for bit with the committed files
    python tests/golden/make_golden_visnet.py --state-dict-layouts   # (re)write reference_state_dicts_visnet.json

It reuses make_golden.py's stand-ins and import machinery and common.py's batch generator and weight filler.  The
reference needs more of torch_geometric and torch_cluster than the hypergraph models do; these STAND-INS are added here,
written from the packages' documented semantics:

* ``radius_graph`` (torch_cluster's CUDA kernel, loop=True, max_num_neighbors=16): tests/visnet_ref.py's -- for each target
  i the atoms j of i's molecule in ascending index, i included, with fp32 squared distance summed x, y, z strictly below
  r^2, the first 16 kept; edges ordered by target, then source; edge_index[0] = source.  Property-tested in
  tests/test_visnet_host.py.
* ``torch_geometric.utils.scatter`` (sum): make_golden's scatter.
* ``MessagePassing`` with the ``_i`` / ``_j`` argument suffixes (gathers at edge_index[1] / edge_index[0]), ``node_dim=0``,
  a tuple-valued ``message`` reduced by an overridden ``aggregate``, and ``edge_updater`` -> ``edge_update``.
* ``GatedEquivariantBlock`` as in PyG 2.5.3 (vec1_proj, vec2_proj, update_net = Linear(2C, C) -> SiLU -> Linear(C, 2C),
  SiLU on the scalar output, the norm of vec1_proj(v) over the 8-component axis).  It is not in the reference checkout:
  its names and arithmetic are unpinned.

Every case keeps each candidate squared distance at least MIN_D2_MARGIN from r^2 (recorded as ``d2_margin``), so the
strict < cannot flip between the float32 and float64 evaluations.  Gradients: per parameter (sum, sum |g|, norm) and the
first rows of every 2-D gradient (whole 1-D gradients), so each file stays well under 1 MB.
"""
from __future__ import annotations

import importlib
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import visnet_ref  # noqa: E402
from common import fill_state_dict, golden_args, make_batch  # noqa: E402

OUT_DIR = os.path.join(HERE, "visnet")
MIN_D2_MARGIN = 1e-3
METHODS = ("visnet_equihnn", "visnet_equihnns", "visnet_equihnnm")

# name: (method, hidden, seed, flavour, float64, extra args, rows of each 2-D gradient stored)
CASES = {
    "visnet_equihnns_c64": ("visnet_equihnns", 64, 11, "qm9", False, {}, 4),
    "visnet_equihnns_c256": ("visnet_equihnns", 256, 12, "qm9", False, {}, 1),
    "visnet_equihnns_c64_f64": ("visnet_equihnns", 64, 13, "qm9", True, {}, 4),
    "visnet_equihnns_c256_f64": ("visnet_equihnns", 256, 14, "qm9", True, {}, 1),
    "visnet_equihnn_c64": ("visnet_equihnn", 64, 15, "qm9", False, {}, 4),
    "visnet_equihnnm_c64_bn": ("visnet_equihnnm", 64, 16, "qm9", False, {"normalization": "bn"}, 4),
    "visnet_equihnns_pcqm_c64": ("visnet_equihnns", 64, 17, "pcqm", False, {}, 4),
}
N_MOLS = 6


# ------------------------------------------------------------------------------------------
# stand-ins (added to make_golden's)
# ------------------------------------------------------------------------------------------
class MessagePassing(torch.nn.Module):
    """torch_geometric.nn.MessagePassing, flow source_to_target: ``x_j`` = x[edge_index[0]], ``x_i`` = x[edge_index[1]];
    message() -> aggregate() (sum over edge_index[1] unless overridden) -> update(); edge_updater() -> edge_update()."""

    def __init__(self, aggr="add", node_dim=-2, **kw):
        super().__init__()
        assert aggr == "add", aggr
        self.aggr, self.node_dim = aggr, node_dim

    @staticmethod
    def _collect(fn, edge_index, kw):
        src, dst = edge_index[0], edge_index[1]
        args = {}
        for p in inspect.signature(fn).parameters:
            if p in kw:
                args[p] = kw[p]
            elif p.endswith("_j") and p[:-2] in kw:
                args[p] = kw[p[:-2]].index_select(0, src)
            elif p.endswith("_i") and p[:-2] in kw:
                args[p] = kw[p[:-2]].index_select(0, dst)
        return args

    def propagate(self, edge_index, size=None, **kw):
        n = next(v.shape[0] for k, v in kw.items() if k in ("x", "q", "vec"))
        msg = self.message(**self._collect(self.message, edge_index, kw))
        return self.update(self.aggregate(msg, index=edge_index[1], ptr=None, dim_size=n))

    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        out = torch.zeros((dim_size,) + tuple(inputs.shape[1:]), dtype=inputs.dtype, device=inputs.device)
        return out.index_add_(0, index, inputs)

    def update(self, aggr_out):
        return aggr_out

    def edge_updater(self, edge_index, **kw):
        return self.edge_update(**self._collect(self.edge_update, edge_index, kw))


def radius_graph(x, r, batch=None, loop=False, max_num_neighbors=32, **kw):
    assert loop and batch is not None
    return visnet_ref.radius_graph(x, batch, r=r, k=max_num_neighbors).to(x.device)


class GatedEquivariantBlock(torch.nn.Module):
    """torch_geometric.nn.models.visnet.GatedEquivariantBlock, PyG 2.5.3."""

    def __init__(self, hidden_channels, out_channels, intermediate_channels=None, scalar_activation=False):
        super().__init__()
        self.out_channels = out_channels
        if intermediate_channels is None:
            intermediate_channels = hidden_channels
        self.vec1_proj = torch.nn.Linear(hidden_channels, hidden_channels, bias=False)
        self.vec2_proj = torch.nn.Linear(hidden_channels, out_channels, bias=False)
        self.update_net = torch.nn.Sequential(torch.nn.Linear(hidden_channels * 2, intermediate_channels),
                                              torch.nn.SiLU(), torch.nn.Linear(intermediate_channels, out_channels * 2))
        self.act = torch.nn.SiLU() if scalar_activation else None

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.vec1_proj.weight)
        torch.nn.init.xavier_uniform_(self.vec2_proj.weight)
        torch.nn.init.xavier_uniform_(self.update_net[0].weight)
        self.update_net[0].bias.data.zero_()
        torch.nn.init.xavier_uniform_(self.update_net[2].weight)
        self.update_net[2].bias.data.zero_()

    def forward(self, x, v):
        vec1 = torch.norm(self.vec1_proj(v), dim=-2)
        vec2 = self.vec2_proj(v)
        x = torch.cat([x, vec1], dim=-1)
        x, v = torch.split(self.update_net(x), self.out_channels, dim=-1)
        v = v.unsqueeze(1) * vec2
        if self.act is not None:
            x = self.act(x)
        return x, v


def import_reference_visnet():
    mg.import_reference(())     # stand-ins, sys.path and the equihgnn.models package shells
    tg_nn = sys.modules["torch_geometric.nn"]
    tg_nn.MessagePassing = MessagePassing
    tg_nn.radius_graph = radius_graph
    tg_nn.models = mg._module("torch_geometric.nn.models")
    tg_nn.models.visnet = mg._module("torch_geometric.nn.models.visnet", GatedEquivariantBlock=GatedEquivariantBlock)
    sys.modules["torch_geometric.utils"].scatter = lambda src, index, dim=0, dim_size=None, reduce="sum": \
        mg._standin_scatter(src, index, dim=dim, dim_size=dim_size, reduce=reduce)
    importlib.import_module("equihgnn.models.equihnn_visnet")
    return importlib.import_module("equihgnn.common.registry").registry


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def d2_margin(pos, batch):
    p = pos.double()
    m = float("inf")
    for b in batch.unique():
        q = p[batch == b]
        d2 = (q.unsqueeze(0) - q.unsqueeze(1)).pow(2).sum(-1)
        m = min(m, float((d2 - 25.0).abs().min()))
    return m


def case_batch(name):
    """The case's batch: common.make_batch (a conjugated hyperedge in molecules 0 and -1, a one-atom molecule in the middle)
    with molecule 1 packed into a 3.4 A cube (every pair within 5 A: the 16-neighbour truncation binds) and the last atom
    of molecule 2 moved 20 A away (no neighbour in radius).  The seed is advanced until every candidate squared distance is
    at least MIN_D2_MARGIN from 25."""
    _, _, seed, flavour, _, _, _ = CASES[name]
    for s in range(seed, seed + 1000):
        b = make_batch(s, n_mols=N_MOLS, flavour=flavour, big=20)
        rng = np.random.default_rng(s)
        pos = b.pos.clone()
        bt = b.batch
        i1 = torch.nonzero(bt == 1).reshape(-1)
        pos[i1] = torch.from_numpy(rng.uniform(-1.7, 1.7, size=(i1.numel(), 3)).astype(np.float32))
        i2 = torch.nonzero(bt == 2).reshape(-1)
        pos[i2[-1]] = pos[i2[-1]] + 20.0
        b.pos = pos
        if d2_margin(b.pos, bt) >= MIN_D2_MARGIN:
            return b, s
    raise RuntimeError(name)


def build_model(registry_or_cls, name, dtype):
    method, hidden, seed, _, _, extra, _ = CASES[name]
    cls = registry_or_cls.get_model_class(method) if hasattr(registry_or_cls, "get_model_class") else registry_or_cls
    torch.manual_seed(0)
    model = cls(1, golden_args(method, hidden, **extra))
    visnet_ref.fill_visnet_model(model, seed, fill_state_dict)
    return model.to(dtype).train()


def run_case(registry, name):
    method, hidden, seed, flavour, f64, extra, rows = CASES[name]
    dtype = torch.float64 if f64 else torch.float32
    model = build_model(registry, name, dtype)
    b, used_seed = case_batch(name)
    data = b
    data.pos, data.y = b.pos.to(dtype), b.y.to(dtype)
    cnt = torch.bincount(visnet_ref.radius_graph(b.pos, b.batch)[1], minlength=b.x.shape[0])
    assert int(cnt.max()) == 16 and int(cnt.min()) == 1
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)        # (Distance builds edge_weight with the default dtype)
    try:
        out = model(data)
    finally:
        torch.set_default_dtype(prev)
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    case = {"meta_method": np.array(method), "meta_hidden": np.array(hidden), "meta_batch_seed": np.array(used_seed),
            "d2_margin": np.array(d2_margin(b.pos.float(), b.batch)), "grad_rows": np.array(rows)}
    for k in ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e", "e_order", "batch", "y"):
        v = getattr(b, k)
        case["in_" + k] = (v.float() if k in ("pos", "y") else v).numpy()
    case["out"] = out.detach().numpy()
    case["loss"] = loss.detach().numpy()
    names, present, stats = [], [], []
    for n, p in model.named_parameters():
        names.append(n)
        present.append(p.grad is not None)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        stats.append([float(g.sum()), float(g.abs().sum()), float(g.norm())])
        if p.grad is not None:
            case["grad_" + n] = (g[:rows] if g.dim() == 2 else g).numpy()
    case["grad_names"] = np.array(names)
    case["grad_present"] = np.array(present)
    case["grad_stats"] = np.array(stats, dtype=np.float64)
    for k, v in model.state_dict().items():
        if "running_" in k:
            case["buf_" + k] = v.numpy()
    return case


# ------------------------------------------------------------------------------------------
# state_dict layouts
# ------------------------------------------------------------------------------------------
def write_state_dict_layouts(path=os.path.join(HERE, "reference_state_dicts_visnet.json")):
    ref = import_reference_visnet()
    out = {}
    for m in METHODS:
        sd = ref.get_model_class(m)(1, golden_args(m, 64)).state_dict()
        out[m] = {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(t)}: {json.dumps(out[t], sort_keys=True)}" for t in sorted(out)) + "\n}\n")
    return path


def main(only=None, check=False):
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    registry = import_reference_visnet()
    os.makedirs(OUT_DIR, exist_ok=True)
    ok = True
    for name in CASES:
        if only and name not in only:
            continue
        case = run_case(registry, name)
        path = os.path.join(OUT_DIR, name + ".npz")
        if check:
            with np.load(path) as z:
                ok &= mg.compare(case, dict(z), name)
            continue
        np.savez_compressed(path, **case)
        print(f"{name}: N={case['in_x'].shape[0]} margin={float(case['d2_margin']):.2e} out[:3]={case['out'][:3]} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    return ok


if __name__ == "__main__":
    if "--state-dict-layouts" in sys.argv:
        print(write_state_dict_layouts())
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a != "--check"]
    sys.exit(0 if main(set(argv) or None, check="--check" in sys.argv) else 1)
