#!/usr/bin/env python3
"""Golden vectors of the 2-D baselines ``gin`` / ``gcn``: the REFERENCE's own equihgnn/models/baseline_2d.py (read from
the reference checkout at run time, never copied) run on small seeded batches.

    python tests/golden/make_golden_2d.py            # (re)write tests/golden/gnn2d/*.npz
    python tests/golden/make_golden_2d.py --check    # regenerate and compare bit for bit with the committed files
    python tests/golden/make_golden_2d.py --state-dict-layouts   # (re)write reference_state_dicts_2d.json

It reuses make_golden.py's stand-ins and import machinery and common.py's weight filler.  baseline_2d.py needs more of
torch_geometric and ogb than the hypergraph models do; the stand-ins added here are written from the packages'
documented semantics (PyG MessagePassing with flow source_to_target and aggregation "add": gather x[edge_index[0]],
message(), scatter-add into edge_index[1], update(); torch_geometric.utils.degree; global_mean_pool / global_max_pool;
ogb 1.3.6 BondEncoder) and are property-tested in tests/test_gnn2d_host.py.  GATConv, GATv2Conv, GlobalAttention and
Set2Set are import-only placeholders that raise when constructed: the cases never build them.
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from common import F64_MIN_MARGIN, fill_state_dict  # noqa: E402

from equihgnn_amd.batch import GMol, collate_graphs, synth_graph  # noqa: E402

BOND_FEATURE_DIMS = (5, 6, 2)   # ogb 1.3.6 get_bond_feature_dims()
OUT_DIR = os.path.join(HERE, "gnn2d")   # (a directory of their own: tests/test_golden_inputs.py owns *.npz here)
SUBSET_ROWS = 8                 # C = 300 cases: rows of every 2-D gradient stored (the full set exceeds ~1 MB)

# name: (gnn_type, hidden, layers, flavour, seed, mode, special)
#   mode: "train" (outputs, loss, gradients, running statistics after one step), "eval", "f64" (train, float64)
#   special: "holes" (a molecule without bonds and an isolated atom), "e0" (no edge in the whole batch), ""
CASES = {
    "gnn2d_gin_c64_f3": ("gin", 64, 5, "pcqm", 35, "train", "holes"),
    "gnn2d_gin_c64_f1": ("gin", 64, 5, "qm9", 21, "train", "holes"),
    "gnn2d_gcn_c64_f3": ("gcn", 64, 5, "pcqm", 28, "train", "holes"),
    "gnn2d_gcn_c64_f1": ("gcn", 64, 5, "qm9", 22, "train", "holes"),
    "gnn2d_gin_c64_e0": ("gin", 64, 5, "pcqm", 16, "train", "e0"),
    "gnn2d_gcn_c64_e0": ("gcn", 64, 5, "qm9", 16, "train", "e0"),
    "gnn2d_gin_c64_eval": ("gin", 64, 5, "pcqm", 17, "eval", "holes"),
    "gnn2d_gcn_c64_eval": ("gcn", 64, 5, "pcqm", 18, "eval", "holes"),
    "gnn2d_gin_c300_f3": ("gin", 300, 3, "pcqm", 25, "train", ""),
    "gnn2d_gcn_c300_f3": ("gcn", 300, 3, "pcqm", 20, "train", ""),
    "gnn2d_gin_c64_f64": ("gin", 64, 5, "pcqm", 46, "f64", "holes"),
    "gnn2d_gcn_c64_f64": ("gcn", 64, 5, "qm9", 31, "f64", "holes"),
    "gnn2d_gin_c300_f64": ("gin", 300, 3, "pcqm", 35, "f64", ""),
    "gnn2d_gcn_c300_f64": ("gcn", 300, 3, "pcqm", 28, "f64", ""),
}
N_MOLS = 8
# C = 300: 2 molecules and 3 layers.  Each row's seed keeps every ReLU input of the float64 reference >= F64_MIN_MARGIN rms
# from its kink (relu_margin, ``--scan``); at 8 molecules x 5 layers x 300 channels (~1e6 ReLU inputs) no seed does.
N_MOLS_WIDE = 2


# ------------------------------------------------------------------------------------------
# stand-ins (added to make_golden's)
# ------------------------------------------------------------------------------------------
class MessagePassing(torch.nn.Module):
    """torch_geometric.nn.MessagePassing, flow source_to_target, aggregation "add"."""

    def __init__(self, aggr="add", **kw):
        super().__init__()
        assert aggr == "add", aggr
        self.aggr = aggr

    def propagate(self, edge_index, size=None, **kw):
        import inspect
        x = kw["x"]
        src, dst = edge_index[0], edge_index[1]
        args = {}
        for p in inspect.signature(self.message).parameters:
            args[p] = x.index_select(0, src) if p == "x_j" else (x.index_select(0, dst) if p == "x_i" else kw[p])
        msg = self.message(**args)
        out = torch.zeros((x.shape[0],) + tuple(msg.shape[1:]), dtype=msg.dtype, device=msg.device)
        return self.update(out.index_add_(0, dst, msg))

    def message(self, x_j):
        return x_j

    def update(self, aggr_out):
        return aggr_out


def degree(index, num_nodes=None, dtype=None):
    """torch_geometric.utils.degree: occurrences of every value of ``index``."""
    n = int(index.max()) + 1 if num_nodes is None else int(num_nodes)
    out = torch.zeros(n, dtype=dtype if dtype is not None else torch.long, device=index.device)
    return out.scatter_add_(0, index, torch.ones(index.numel(), dtype=out.dtype, device=index.device))


def _n_graphs(batch, size):
    return int(batch.max()) + 1 if size is None else int(size)


def global_mean_pool(x, batch, size=None):
    """torch_geometric.nn.global_mean_pool: per-graph mean of the rows (scatter mean; an empty graph gives 0)."""
    B = _n_graphs(batch, size)
    s = torch.zeros((B, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
    n = torch.zeros(B, dtype=x.dtype, device=x.device).index_add_(0, batch, torch.ones_like(x[:, 0]))
    return s / n.clamp(min=1).unsqueeze(-1)


def global_max_pool(x, batch, size=None):
    """torch_geometric.nn.global_max_pool: per-graph elementwise maximum."""
    B = _n_graphs(batch, size)
    out = torch.full((B, x.shape[1]), float("-inf"), dtype=x.dtype, device=x.device)
    return out.scatter_reduce(0, batch.unsqueeze(-1).expand_as(x), x, "amax", include_self=True)


class BondEncoder(torch.nn.Module):
    """ogb 1.3.6 BondEncoder: one xavier-initialised table per bond feature, summed over the columns present."""

    def __init__(self, emb_dim):
        super().__init__()
        self.bond_embedding_list = torch.nn.ModuleList()
        for d in BOND_FEATURE_DIMS:
            emb = torch.nn.Embedding(d, emb_dim)
            torch.nn.init.xavier_uniform_(emb.weight.data)
            self.bond_embedding_list.append(emb)

    def forward(self, edge_attr):
        bond_embedding = 0
        for i in range(edge_attr.shape[1]):
            bond_embedding = bond_embedding + self.bond_embedding_list[i](edge_attr[:, i])
        return bond_embedding


def _placeholder(name):
    def init(self, *a, **k):
        raise RuntimeError(f"{name} stand-in must not be constructed (only imported)")
    return type(name, (torch.nn.Module,), {"__init__": init})


def install_standins_2d():
    """make_golden's stand-ins plus what baseline_2d.py imports."""
    tg_nn = sys.modules["torch_geometric.nn"]
    for k, v in dict(MessagePassing=MessagePassing, global_mean_pool=global_mean_pool, global_max_pool=global_max_pool,
                     GATConv=_placeholder("GATConv"), GATv2Conv=_placeholder("GATv2Conv"),
                     GlobalAttention=_placeholder("GlobalAttention")).items():
        setattr(tg_nn, k, v)
    tg_nn.aggr = mg._module("torch_geometric.nn.aggr", Set2Set=_placeholder("Set2Set"))
    sys.modules["torch_geometric.utils"].degree = degree
    sys.modules["ogb.graphproppred.mol_encoder"].BondEncoder = BondEncoder


def import_reference_2d():
    mg.import_reference(())          # stand-ins, sys.path and the equihgnn.models package shells
    install_standins_2d()
    importlib.import_module("equihgnn.models.baseline_2d")
    return importlib.import_module("equihgnn.common.registry").registry


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def case_mols(flavour: str, seed: int, special: str, n_mols: int = N_MOLS):
    rng = np.random.default_rng(seed)
    mols = [synth_graph(rng, flavour) for _ in range(n_mols)]
    F = mols[0].edge_attr.shape[1]
    if special == "holes":
        m = mols[2]                  # a molecule without bonds
        mols[2] = GMol(x=m.x, edge_index=np.zeros((2, 0), np.int64), edge_attr=np.zeros((0, F), np.int64), y=m.y)
        m = mols[5]                  # an isolated atom (no bond reaches it)
        mols[5] = GMol(x=np.concatenate([m.x, m.x[:1]], 0), edge_index=m.edge_index, edge_attr=m.edge_attr, y=m.y)
    elif special == "e0":
        mols = [GMol(x=m.x, edge_index=np.zeros((2, 0), np.int64), edge_attr=np.zeros((0, F), np.int64), y=m.y)
                for m in mols]
    return mols


def case_batch(name, seed=None):
    """The collated inputs of a case (also what the GPU tests rebuild from the stored arrays)."""
    _, hidden, _, flavour, row_seed, _, special = CASES[name]
    n_mols = N_MOLS_WIDE if hidden > 64 else N_MOLS
    return collate_graphs(case_mols(flavour, row_seed if seed is None else seed, special, n_mols))


class _ReluMargin(mg._ReluMargin):
    """make_golden._ReluMargin that also lets the empty message tensor of a batch without edges through."""

    def __enter__(self):
        super().__enter__()
        spy = torch.nn.functional.relu
        torch.nn.functional.relu = lambda x, inplace=False: self.orig(x, inplace) if x.numel() == 0 else spy(x, inplace)
        return self


def relu_margin(registry, name, seed=None):
    """Distance of the closest ReLU input to its kink (min |x| / rms(x), _ReluMargin) in one training-mode
    forward of the reference in FLOAT64 on the case's weights and batch.  A float32 evaluation reproduces the gradients
    only while this stays above its rounding distance (~1e-6): the train-mode rows use seeds with margin >= F64_MIN_MARGIN
    (``--scan`` prints the first such seed from the row's seed on)."""
    gnn_type, hidden, layers, _, row_seed, _, _ = CASES[name]
    seed = row_seed if seed is None else seed
    torch.manual_seed(0)
    model = registry.get_model_class(gnn_type)(1, num_layer=layers, emb_dim=hidden, gnn_type=gnn_type)
    fill_state_dict(model, seed)
    model = model.double().train()
    data = _Data(case_batch(name, seed), torch.float64)
    with _ReluMargin() as rm:
        with torch.no_grad():
            model(data)
        return rm.take()


def scan_seeds(registry, name, tries=400):
    seed0 = CASES[name][4]
    for sd in range(seed0, seed0 + tries):
        m = relu_margin(registry, name, sd)
        print(f"{name}: seed {sd} relu margin {m:.2e}", flush=True)
        if m >= F64_MIN_MARGIN:
            return sd
    return None


class _Data:
    def __init__(self, b, dtype):
        self.x, self.edge_index, self.edge_attr, self.batch = b.x, b.edge_index, b.edge_attr, b.batch
        self.y = b.y.to(dtype)
        self.num_graphs = b.num_graphs


def run_case(registry, name):
    gnn_type, hidden, layers, flavour, seed, mode, special = CASES[name]
    torch.manual_seed(0)
    klass = registry.get_model_class(gnn_type)
    model = klass(1, num_layer=layers, emb_dim=hidden, gnn_type=gnn_type)
    fill_state_dict(model, seed)
    dtype = torch.float64 if mode == "f64" else torch.float32
    model = model.to(dtype)
    b = case_batch(name)
    data = _Data(b, dtype)
    case = {"meta_name": np.array(name), "in_x": b.x.numpy(), "in_edge_index": b.edge_index.numpy(),
            "in_edge_attr": b.edge_attr.numpy(), "in_batch": b.batch.numpy(), "in_y": b.y.numpy()}
    if mode == "eval":
        model.eval()
        with torch.no_grad():
            case["out"] = model(data).numpy()
        return case
    case["relu_margin"] = np.array(relu_margin(registry, name), dtype=np.float64)
    model.train()
    out = model(data)
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    case["out"] = out.detach().numpy()
    case["loss"] = np.array(loss.item())
    names, present = [], []
    for k, p in model.named_parameters():
        names.append(k)
        present.append(p.grad is not None)
        if p.grad is None:
            continue
        g = p.grad.numpy()
        if hidden > 64 and g.ndim == 2:
            g = g[:SUBSET_ROWS]
        case["g:" + k] = g
    case["grad_names"] = np.array(names)
    case["grad_present"] = np.array(present)
    for k, v in model.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            case["rs:" + k] = v.numpy()
    return case


# ------------------------------------------------------------------------------------------
# state_dict layouts
# ------------------------------------------------------------------------------------------
def state_dict_layout_2d(klass, gnn_type, emb_dim=32):
    sd = klass(1, num_layer=5, emb_dim=emb_dim, gnn_type=gnn_type).state_dict()
    return {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}


def write_state_dict_layouts(path=os.path.join(HERE, "reference_state_dicts_2d.json")):
    ref = import_reference_2d()
    out = {t: state_dict_layout_2d(ref.get_model_class(t), t) for t in ("gin", "gcn")}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(t)}: {json.dumps(out[t], sort_keys=True)}" for t in sorted(out)) + "\n}\n")
    return path


def main(only=None, check=False):
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    registry = import_reference_2d()
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
        if "relu_margin" in case:
            assert float(case["relu_margin"]) >= F64_MIN_MARGIN, (name, float(case["relu_margin"]), "run --scan")
        np.savez_compressed(path, **case)
        print(f"{name}: N={case['in_x'].shape[0]} E={case['in_edge_index'].shape[1]} out[:3]={case['out'][:3]} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    return ok


if __name__ == "__main__":
    if "--state-dict-layouts" in sys.argv:
        print(write_state_dict_layouts())
        sys.exit(0)
    if "--scan" in sys.argv:
        torch.set_num_threads(1)
        reg = import_reference_2d()
        for nm in [a for a in sys.argv[1:] if a in CASES] or [n for n in CASES if CASES[n][5] != "eval"]:
            print(f"{nm}: first seed with margin >= {F64_MIN_MARGIN:g}: {scan_seeds(reg, nm)}", flush=True)
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a != "--check"]
    sys.exit(0 if main(set(argv) or None, check="--check" in sys.argv) else 1)
