#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE's own model
files (read from /root/reference at run time, never copied) on seeded synthetic batches.

Run in the build container only:   python tests/golden/make_golden.py
(the GPU box has no /root/reference; it consumes the committed .npz files).

The reference's third-party dependencies are absent from this image.  The
stand-ins below are this repo's own code, written from the packages' documented semantics;
they exist only so that the reference's files import.  What is pinned by the vectors is the
reference's own arithmetic in equihgnn/models/** (wrappers, MHNN(S)Conv, MLP, EGNN,
Equiformer); the stand-ins are cross-checked by property tests in tests/test_standins.py.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("EQUIHGNN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from common import (CASE_TABLE, F64_FULL_LIMIT, F64_MIN_MARGIN, F64_TABLE, LAYER_TABLE, TRAJECTORY_TABLE, layer_inputs, case_spec,  # noqa: E402
                    f64_sample_indices, f64_spec, trajectory_batches, fill_state_dict, golden_args, load_case, make_batch, zero_dropouts)

from equihgnn_amd.batch import ATOM_FEATURE_DIMS  # noqa: E402


# ------------------------------------------------------------------------------------------
# stand-ins for absent third-party packages
# ------------------------------------------------------------------------------------------
def _standin_scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    """torch_scatter.scatter for the call pattern of conv.py (1-D index along ``dim``)."""
    assert out is None and index.dim() == 1
    dim = dim if dim >= 0 else src.dim() + dim
    if dim_size is None:
        dim_size = int(index.max()) + 1
    view = [1] * src.dim()
    view[dim] = -1
    idx = index.view(view).expand_as(src)
    shape = list(src.shape)
    shape[dim] = dim_size
    res = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(dim, idx, src)
    if reduce in ("sum", "add"):
        return res
    if reduce == "mean":
        cnt = torch.bincount(index, minlength=dim_size).clamp(min=1).to(src.dtype)
        return res / cnt.view(view)
    raise ValueError(reduce)


def _standin_global_add_pool(x, batch, size=None):
    size = int(batch.max()) + 1 if size is None else size
    return _standin_scatter(x, batch, dim=-2, dim_size=size, reduce="sum")


class _StandinAtomEncoder(torch.nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.atom_embedding_list = torch.nn.ModuleList()
        for d in ATOM_FEATURE_DIMS:
            emb = torch.nn.Embedding(d, emb_dim)
            torch.nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)

    def forward(self, x):
        acc = 0
        for i in range(x.shape[1]):
            acc += self.atom_embedding_list[i](x[:, i])
        return acc


def _standin_get_at(pattern, tensor, indices):
    """einx.get_at for the three patterns the Equiformer uses
    (equiformer_layer.py:356,1331-1335): gather along the bracketed axis."""
    pat = pattern.replace(" ", "")
    if pat == "b[i]dm,bjk->bjkdm":
        b = torch.arange(tensor.shape[0], device=tensor.device)[:, None, None]
        return tensor[b, indices]
    if pat == "bi[j]c,bik->bikc":
        return tensor.gather(2, indices[..., None].expand(*indices.shape, tensor.shape[-1]))
    if pat == "bi[j],bik->bik":
        return tensor.gather(2, indices)
    raise NotImplementedError(pattern)


def _standin_to_dense_batch(x, batch=None, fill_value=0.0, max_num_nodes=None, batch_size=None):
    """torch_geometric.utils.to_dense_batch: [N, ...] + sorted batch vector -> [B, Nmax, ...], mask."""
    if batch is None:
        batch = x.new_zeros(x.shape[0], dtype=torch.long)
    b = int(batch.max()) + 1 if batch_size is None else batch_size
    counts = torch.bincount(batch, minlength=b)
    nmax = int(counts.max()) if max_num_nodes is None else max_num_nodes
    start = torch.cumsum(counts, 0) - counts
    pos = torch.arange(x.shape[0]) - start[batch]
    out = x.new_full((b, nmax, *x.shape[1:]), fill_value)
    mask = torch.zeros(b, nmax, dtype=torch.bool)
    out[batch, pos] = x
    mask[batch, pos] = True
    return out, mask


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_standins():
    _module("torch_scatter", scatter=_standin_scatter)
    _module("ogb")
    _module("ogb.graphproppred")
    _module("ogb.graphproppred.mol_encoder", AtomEncoder=_StandinAtomEncoder)
    tg = _module("torch_geometric")
    tg.nn = _module("torch_geometric.nn", global_add_pool=_standin_global_add_pool)
    tg.utils = _module("torch_geometric.utils", to_dense_batch=_standin_to_dense_batch)
    import typing

    _module("beartype", beartype=lambda f: f)
    bt = _module("beartype.typing")
    for k in ("Dict", "Optional", "Tuple", "Union", "List", "Callable"):
        setattr(bt, k, getattr(typing, k))
    _module("einx", get_at=_standin_get_at)
    _module("opt_einsum", contract=lambda eq, *ops, **kw: torch.einsum(eq, *ops))

    class _Never(torch.nn.Module):  # num_linear_attn_heads=0 -> never instantiated
        def __init__(self, *a, **k):
            raise RuntimeError("TaylorSeriesLinearAttn stand-in must not be constructed")

    _module("taylor_series_linear_attention", TaylorSeriesLinearAttn=_Never)


def reconstructed_J():
    """The reference's data/J_dense.pt is a missing blob (.MISSING_LARGE_BLOBS).  J_l is the
    real-spherical-harmonic representation of the x<->y... axis swap used by the ZYZ Wigner-D
    construction (irr_repr.py:23-32).  SURVEY.md §8c documents the reconstruction and its
    checks; J2 only feeds the (1,1) basis, which is dead for the type-0 output."""
    s3 = np.sqrt(3.0) / 2.0
    J0 = torch.tensor([[1.0]], dtype=torch.float64)
    J1 = torch.tensor([[0, 1, 0], [1, 0, 0], [0, 0, -1]], dtype=torch.float64)
    J2 = torch.tensor([[0, 0, 0, -1, 0], [0, 1, 0, 0, 0], [0, 0, -0.5, 0, -s3],
                       [-1, 0, 0, 0, 0], [0, 0, -s3, 0, 0.5]], dtype=torch.float64)
    return [J0, J1, J2]


def import_reference(names=("equihnn_egnn", "mhnn")):
    """Import the reference's model files without executing equihgnn/models/__init__.py
    (which eagerly imports PyG/torch_cluster-dependent models)."""
    install_standins()
    os.environ["CLEAR_CACHE"] = "1"
    sys.path.insert(0, REF)
    for pkg, sub in (("equihgnn.models", "equihgnn/models"),
                     ("equihgnn.models.layers", "equihgnn/models/layers"),
                     ("equihgnn.models.layers.equiformer", "equihgnn/models/layers/equiformer")):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, sub)]
        sys.modules[pkg] = m
    if "equihnn_equiformer" in names:
        real_load = torch.load

        def patched_load(path, *a, **k):
            if str(path).endswith("J_dense.pt"):
                return reconstructed_J()
            return real_load(path, *a, **k)

        torch.load = patched_load
        try:
            importlib.import_module("equihgnn.models.layers.equiformer.irr_repr")
        finally:
            torch.load = real_load
    for n in names:
        importlib.import_module("equihgnn.models." + n)
    return importlib.import_module("equihgnn.common.registry").registry


# ------------------------------------------------------------------------------------------
# cases (the table, the batch generator and its options live in common.py: the tests re-derive the inputs)
# ------------------------------------------------------------------------------------------
def run_case(registry, spec):
    method, hidden, seed, train_mode, store_grads = (spec["method"], spec["hidden"], spec["seed"], spec["train"],
                                                     spec["store_grads"])
    torch.manual_seed(0)
    args = golden_args(method, hidden, **spec.get("args", {}))
    model = registry.get_model_class(method)(1, args)
    fill_state_dict(model, seed)
    model.train(train_mode)
    if spec["dropout0"]:
        zero_dropouts(model)
    data = make_batch(spec)

    taps = {}
    hooks = []

    def tap(name, pick=lambda o: o):
        counter = {"n": 0}

        def fn(_m, _i, o):
            key = name if name != "conv" else f"conv{counter['n']}"
            counter["n"] += 1
            taps[key] = pick(o).detach().clone()
        return fn

    hooks.append(model.atom_encoder.register_forward_hook(tap("atom_encoder")))
    if hasattr(model, "egnn_layer"):
        hooks.append(model.egnn_layer.register_forward_hook(tap("front_end", lambda o: o[0][0])))
    if hasattr(model, "fa_former"):
        hooks.append(model.fa_former.register_forward_hook(tap("front_end", lambda o: o[0][0])))
    if hasattr(model, "equiformer_layer"):
        hooks.append(model.equiformer_layer.register_forward_hook(
            tap("front_end", lambda o: o.type0[0])))
    if hasattr(model, "conv"):
        # the wrapper applies act() after conv; tap the conv output itself
        # MHNNSConv returns X; MHNNConv returns (X, E): tap the node features
        hooks.append(model.conv.register_forward_hook(
            tap("conv", lambda o: (o[0] if isinstance(o, tuple) else o).reshape(-1, (o[0] if isinstance(o, tuple) else o).shape[-1]))))
    if hasattr(model, "batch_norms"):
        for i, bn in enumerate(model.batch_norms):
            hooks.append(bn.register_forward_hook(tap(f"bn{i}")))
    hooks.append(model.mlp_out.register_forward_pre_hook(
        lambda _m, i: taps.__setitem__("pool", i[0].detach().reshape(-1, i[0].shape[-1]).clone())))

    # record the neighbour lists the reference's own topk call produces
    real_topk = torch.Tensor.topk
    rec = {}

    def spy_topk(self, *a, **k):
        r = real_topk(self, *a, **k)
        rec.setdefault("idx", r.indices.detach().clone())
        rec.setdefault("val", r.values.detach().clone())
        return r

    torch.Tensor.topk = spy_topk
    try:
        out = model(data)
    finally:
        torch.Tensor.topk = real_topk
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    for h in hooks:
        h.remove()

    case = {"meta_method": np.array(method), "meta_hidden": np.array(hidden),
            "meta_seed": np.array(seed), "meta_train": np.array(int(train_mode))}
    for k in ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e", "e_order", "batch", "y"):
        case["in_" + k] = getattr(data, k).numpy()
    for k, v in taps.items():
        case["tap_" + k] = v.numpy()
    if "idx" in rec:
        case["knn_idx"] = rec["idx"].reshape(-1, rec["idx"].shape[-1]).numpy()
        case["knn_val"] = rec["val"].reshape(-1, rec["val"].shape[-1]).numpy()
    case["out"] = out.detach().numpy()
    case["loss"] = loss.detach().numpy()
    if train_mode and any(isinstance(m_, torch.nn.BatchNorm1d) for m_ in model.modules()):
        # train-mode BatchNorm over ~100 atoms amplifies fp32 rounding: the reference's OWN float32 output sits 3e-6 .. 7e-6 from
        # its float64 evaluation (and moves by 2e-6 .. 4e-6 with the thread count), so these cases also carry the float64 output --
        # the rounding-free value of the reference's algorithm -- for the forward bound
        torch.manual_seed(0)
        m64 = registry.get_model_class(method)(1, args)
        fill_state_dict(m64, seed)
        m64.train(True)
        m64 = m64.double()
        d64 = make_batch(spec)
        d64.pos, d64.y = d64.pos.double(), d64.y.double()
        with torch.no_grad():
            case["out_f64"] = m64(d64).numpy()
    names, has_grad, stats = [], [], []
    for n, p in model.named_parameters():
        names.append(n)
        has_grad.append(p.grad is not None)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        stats.append([float(g.sum()), float(g.abs().sum()), float(g.norm())])
        if store_grads and p.grad is not None and p.numel() <= 20000:
            case["grad_" + n] = g.numpy()
        elif p.grad is not None:
            flat = g.reshape(-1)
            case["gradhead_" + n] = flat[: min(64, flat.numel())].numpy()
    case["grad_names"] = np.array(names)
    case["grad_present"] = np.array(has_grad)
    case["grad_stats"] = np.array(stats, dtype=np.float64)
    if any(k.endswith("running_mean") for k in model.state_dict()):
        for k, v in model.state_dict().items():
            if "running_" in k:
                case["buf_" + k] = v.numpy()
    return case


def run_case_f64(registry, spec, return_margin_only=False):
    """The reference's own model in FLOAT64 (`.double()`, float64 coordinates and targets) on a case's batch: output, loss and
    every parameter gradient (whole up to F64_FULL_LIMIT entries, an evenly spread sample above), plus the distance of the
    closest ReLU input to its kink (rms units)."""
    method, hidden, seed, train_mode = spec["method"], spec["hidden"], spec["seed"], spec["train"]
    torch.manual_seed(0)
    model = registry.get_model_class(method)(1, golden_args(method, hidden))
    fill_state_dict(model, seed)               # float32 values, exactly what the float32 side loads
    model.train(train_mode)
    if spec["dropout0"]:
        zero_dropouts(model)
    model = model.double()
    data = make_batch(spec)
    inputs = {k: getattr(data, k).numpy().copy() for k in ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e",
                                                            "e_order", "batch", "y")}
    data.pos, data.y = data.pos.double(), data.y.double()
    with _ReluMargin() as rm:
        out = model(data)
        margin = rm.take()
    if return_margin_only:
        return margin
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    assert out.dtype == torch.float64
    case = {"meta_method": np.array(method), "meta_hidden": np.array(hidden), "meta_seed": np.array(seed),
            "meta_train": np.array(int(train_mode)), "relu_margin": np.array(margin, dtype=np.float64),
            "out64": out.detach().numpy(), "loss64": loss.detach().numpy()}
    for k, v in inputs.items():
        case["in_" + k] = v
    names, has, absmax = [], [], []
    for n, p in model.named_parameters():
        names.append(n)
        has.append(p.grad is not None)
        if p.grad is None:
            absmax.append(0.0)
            continue
        g = p.grad.detach().numpy()
        absmax.append(float(np.abs(g).max()))
        # (stored as float32: the values are the float64 evaluation's, rounded once -- 6e-8 relative against the 5e-5 bound)
        if g.size <= F64_FULL_LIMIT:
            case["g64_" + n] = g.astype(np.float32)
        else:
            case["g64s_" + n] = g.reshape(-1)[f64_sample_indices(g.size)].astype(np.float32)
    case["grad_names"], case["grad_present"] = np.array(names), np.array(has)
    case["grad_absmax"] = np.array(absmax, dtype=np.float64)
    return case


def scan_f64_seeds(registry, name, tries=200):
    """First seed from the row's seed on whose closest ReLU input is >= F64_MIN_MARGIN rms from zero on the float64
    reference (`python make_golden.py --scan-f64 [names]`)."""
    spec = f64_spec(name)
    for sd in range(spec["seed"], spec["seed"] + tries):
        m = run_case_f64(registry, dict(spec, seed=sd), return_margin_only=True)
        print(f"{name}: seed {sd} relu margin {m:.2e}", flush=True)
        if m >= F64_MIN_MARGIN:
            return sd
    return None


def d_fixture():
    """Known-answer vectors for the D construction alone (equiformer/basis.py:194-215): crafted rel_pos rows --
    generic directions, the axes, exactly -y, rows inside the |x_hat + y_hat|^2 < 1e-6 clamp on a log scale of
    deviations, a zero vector, tiny and huge norms -- and the reference's D[1] for them."""
    basis = importlib.import_module("equihgnn.models.layers.equiformer.basis")
    g = np.random.default_rng(77)
    rows = [g.standard_normal(3) for _ in range(24)]
    rows += [np.array(v, float) for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1],
                                          [0, -2.5, 0], [0, 0, 0], [1e-12, -3e-12, 2e-12], [3e3, -1e3, 2e3])]
    for dev in (1e-5, 3e-5, 1e-4, 2e-4, 3e-4, 4e-4, 5e-4, 5.8e-4, 7e-4, 9e-4, 9.9e-4, 1.01e-3, 1.2e-3, 2e-3, 1e-2):
        phi = g.uniform(0, 2 * np.pi)
        rows.append(np.array([dev * np.cos(phi), -1.0, dev * np.sin(phi)]) * g.uniform(0.8, 3.0))
    rel = torch.tensor(np.stack(rows), dtype=torch.float32)[None, :, None, :]      # [1, E, 1, 3], as at :1346
    D = basis.get_D_to_from_z_axis(rel, 1)[1]
    return {"rel_pos": rel.reshape(-1, 3).numpy(), "D1": D.reshape(-1, 3, 3).numpy()}


class _ReluMargin:
    """While active, every ReLU the reference evaluates (F.relu in mlp.py:93-97, nn.ReLU in the wrappers) reports how close
    its closest input lies to the kink: min |x| / rms(x).  A training trajectory is reproducible to 1e-4 by another fp32
    implementation only while no input sits within that implementation's rounding distance (~1e-6 rms) of zero: past such
    a point the two sides differ by a finite jump of the gradient, not by rounding."""

    def __enter__(self):
        self.orig = torch.nn.functional.relu
        self.values = []

        def spy(x, inplace=False):
            with torch.no_grad():
                xd = x.detach()
                self.values.append(float(xd.abs().min() / xd.pow(2).mean().sqrt().clamp_min(1e-30)))
            return self.orig(x, inplace)

        torch.nn.functional.relu = spy
        return self

    def __exit__(self, *exc):
        torch.nn.functional.relu = self.orig

    def take(self):
        v, self.values = (min(self.values) if self.values else float("inf")), []
        return v


def run_trajectory(registry, name, spec=None):
    """`steps` optimiser steps of the reference model as LitModel runs them (main.py:49-63,137-140)."""
    method, hidden, seed, n_mols, steps, lr = spec or TRAJECTORY_TABLE[name]
    torch.manual_seed(0)
    model = registry.get_model_class(method)(1, golden_args(method, hidden))
    fill_state_dict(model, seed)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    losses, outs, margins = [], [], []
    batches = trajectory_batches(name) if spec is None else [make_batch(seed + t, n_mols) for t in range(steps)]
    with _ReluMargin() as rm:
        for data in batches:
            opt.zero_grad(set_to_none=True)
            out = model(data)
            margins.append(rm.take())
            loss = torch.nn.MSELoss()(out, data.y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            outs.append(out.detach().numpy().copy())
    case = {"meta_method": np.array(method), "meta_hidden": np.array(hidden), "meta_seed": np.array(seed),
            "meta_lr": np.array(lr), "loss": np.array(losses, dtype=np.float64),
            "relu_margin": np.array(margins, dtype=np.float64),     # per step: the closest ReLU input to its kink, in rms units
            "out": np.stack([np.pad(o, (0, max(len(x) for x in outs) - len(o))) for o in outs]),
            "out_len": np.array([len(o) for o in outs])}
    names, norms = [], []
    for n, p in model.named_parameters():
        names.append(n)
        norms.append(float(p.detach().norm()))
        if p.numel() <= 5000:
            case["param_" + n] = p.detach().numpy().copy()
    case["param_names"] = np.array(names)
    case["param_norms"] = np.array(norms, dtype=np.float64)
    for k, v in model.state_dict().items():
        if "running_" in k:
            case["buf_" + k] = v.numpy().copy()
    return case


def run_layer(name):
    """The reference's Equiformer layer (equiformer_layer.py:961-1398) built as equihnn_equiformer.py:37-49 builds it,
    except for the depth."""
    hidden, depth, seed, n = LAYER_TABLE[name]
    eq = importlib.import_module("equihgnn.models.layers.equiformer_layer")
    torch.manual_seed(0)
    layer = eq.Equiformer(dim=hidden, heads=1, depth=depth, dim_head=48, num_degrees=2, valid_radius=5, num_neighbors=16,
                          l2_dist_attention=False, reduce_dim_out=False, attend_self=True, linear_out=True)
    fill_state_dict(layer, seed)
    feats, coors, w0, w1 = layer_inputs(name)
    feats.requires_grad_(True)
    out = layer(feats[None], coors[None], torch.ones(1, n, dtype=torch.bool))
    t0, t1 = out.type0[0], out.type1[0]
    ((t0 * w0).sum() + (t1 * w1).sum()).backward()
    case = {"meta_hidden": np.array(hidden), "meta_depth": np.array(depth), "meta_seed": np.array(seed),
            "in_feats": feats.detach().numpy(), "in_coors": coors.numpy(), "in_w0": w0.numpy(), "in_w1": w1.numpy(),
            "type0": t0.detach().numpy(), "type1": t1.detach().numpy(), "grad_feats": feats.grad.numpy()}
    names, has, stats = [], [], []
    for n_, p in layer.named_parameters():
        names.append(n_)
        has.append(p.grad is not None)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        stats.append([float(g.sum()), float(g.abs().sum()), float(g.norm())])
        if p.grad is not None and p.numel() <= 6000:
            case["grad_" + n_] = g.numpy()
    case["grad_names"], case["grad_present"] = np.array(names), np.array(has)
    case["grad_stats"] = np.array(stats, dtype=np.float64)
    # the (1,1) basis is an SVD null-space vector per J whose SIGN is LAPACK's choice (equiformer/basis.py:41-53); it is
    # a buffer of the state_dict, i.e. data: the fixture carries the one this run of the reference computed
    case["buf_basis11"] = getattr(layer, "basis:(1,1)").numpy().copy()
    return case


def compare(case, stored, name):
    bad = []
    for k in sorted((set(case) | set(stored)) - {"meta_name"}):
        if k not in case or k not in stored:
            bad.append(f"{k}: only on one side")
        elif np.asarray(case[k]).dtype.kind in "US":
            if str(case[k]) != str(stored[k]) and not np.array_equal(case[k], stored[k]):
                bad.append(f"{k}: differs")
        elif np.asarray(case[k]).shape != stored[k].shape or not np.array_equal(np.asarray(case[k]), stored[k]):
            bad.append(f"{k}: differs (max |d| = "
                       f"{np.abs(np.asarray(case[k], float) - stored[k].astype(float)).max() if np.asarray(case[k]).shape == stored[k].shape else 'shape'})")
    print(f"{name}: " + ("identical to the committed file" if not bad else "DIFFERS: " + "; ".join(bad[:6])))
    return not bad


def main(only=None, check=False):
    # one thread and deterministic kernels: the multi-threaded CPU backward sums gradient contributions in a
    # run-dependent order (differences of 1e-8), and `--check` compares the regenerated arrays bit for bit
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    names = [n for n in CASE_TABLE if only is None or n in only]
    f64 = [n for n in F64_TABLE if only is None or n in only]
    traj = [n for n in TRAJECTORY_TABLE if only is None or n in only]
    layers = [n for n in LAYER_TABLE if only is None or n in only]
    methods = {CASE_TABLE[n][0] for n in names} | {TRAJECTORY_TABLE[n][0] for n in traj} | {F64_TABLE[n][0] for n in f64}
    mods = []
    if methods & {"mhnnm", "mhnn", "mhnns"}:
        mods.append("mhnn")
    if methods & {"egnn_equihnns", "egnn_equihnn", "egnn_equihnnm"}:
        mods.append("equihnn_egnn")
    if "equiformer_equihnns" in methods or (only is None or "equiformer_D" in only) or layers:
        mods.append("equihnn_equiformer")
    if "faformer_equihnns" in methods:
        mods.append("equihnn_fa_former")
    registry = import_reference(tuple(mods))
    ok = True
    for name in names:
        case = run_case(registry, case_spec(name))
        path = os.path.join(HERE, name + ".npz")
        if check:
            ok &= compare(case, load_case(name), name)
            continue
        np.savez_compressed(path, **case)
        print(f"{name}: N={case['in_x'].shape[0]} M={case['in_edge_attr'].shape[0]} "
              f"nnz={case['in_edge_index0'].shape[0]} out[:3]={case['out'][:3]} "
              f"loss={float(case['loss']):.6f} -> {os.path.getsize(path)/1024:.0f} KiB")
    for name in f64:
        case = run_case_f64(registry, f64_spec(name))
        if check:
            ok &= compare(case, load_case(name), name)
            continue
        assert float(case["relu_margin"]) >= F64_MIN_MARGIN, (name, float(case["relu_margin"]), "re-run --scan-f64 and update the seed")
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **case)
        print(f"{name}: N={case['in_x'].shape[0]} out64[:3]={case['out64'][:3]} loss64={float(case['loss64']):.9f} "
              f"relu margin {float(case['relu_margin']):.2e} -> {os.path.getsize(path)/1024:.0f} KiB")
    for name in traj:
        case = run_trajectory(registry, name)
        if check:
            ok &= compare(case, load_case(name), name)
        else:
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **case)
            print(f"{name}: losses {case['loss']}")
    for name in layers:
        case = run_layer(name)
        if check:
            ok &= compare(case, load_case(name), name)
        else:
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **case)
            print(f"{name}: type0 {case['type0'].shape} |type1| {np.abs(case['type1']).max():.3f} "
                  f"live grads {int(case['grad_present'].sum())}/{len(case['grad_present'])}")
    if only is None or "equiformer_D" in only:
        case = d_fixture()
        if check:
            ok &= compare(case, load_case("equiformer_D"), "equiformer_D")
        else:
            np.savez_compressed(os.path.join(HERE, "equiformer_D.npz"), **case)
            print(f"equiformer_D: {case['rel_pos'].shape[0]} rows")
    return ok


def scan_trajectory_seeds(name, seeds):
    """Kink margins of the trajectory `name` re-seeded: `python make_golden.py --scan trajectory_egnn_equihnns_c64 81 82 ...`
    (how the seeds of TRAJECTORY_TABLE were chosen: the closest ReLU input of every step at least 1e-5 rms from zero)."""
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    method, hidden, _, n_mols, steps, lr = TRAJECTORY_TABLE[name]
    registry = import_reference(("mhnn",) if method.startswith("mhnn") else ("equihnn_egnn",))
    for seed in seeds:
        case = run_trajectory(registry, name, (method, hidden, seed, n_mols, steps, lr))
        print(f"seed {seed}: relu margins per step {case['relu_margin']}  losses {case['loss']}")


INSTALL_METHODS = ("egnn_equihnns", "mhnnm", "mhnn", "mhnns", "egnn_equihnn", "egnn_equihnnm")


def state_dict_layout(klass, method):
    """{key: [shape, dtype]} of ``klass(1, args)``'s state_dict at the small size tests/test_install.py builds."""
    from equihgnn_amd.registry import default_args
    sd = klass(1, default_args(method=method, MLP_hidden=32, output_hidden=16)).state_dict()
    return {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}


def write_state_dict_layouts(path=os.path.join(HERE, "reference_state_dicts.json")):
    """The state_dict layout of the reference's own class for every method of INSTALL_METHODS: what
    tests/test_install.py holds the drop-in classes to where the reference checkout is absent."""
    import json
    ref = import_reference(("equihnn_egnn", "mhnn"))
    out = {m: state_dict_layout(ref.get_model_class(m), m) for m in INSTALL_METHODS}
    with open(path, "w") as f:        # one line per method
        f.write("{\n" + ",\n".join(f"{json.dumps(m)}: {json.dumps(out[m], sort_keys=True)}" for m in sorted(out)) + "\n}\n")
    return path


if __name__ == "__main__":
    if "--state-dict-layouts" in sys.argv:
        print(write_state_dict_layouts())
        sys.exit(0)
    if "--scan-f64" in sys.argv:
        torch.set_num_threads(1)
        torch.use_deterministic_algorithms(True)
        wanted = [a for a in sys.argv[1:] if a in F64_TABLE] or list(F64_TABLE)
        reg = import_reference(("mhnn", "equihnn_egnn", "equihnn_equiformer", "equihnn_fa_former"))
        for nm in wanted:
            print(f"{nm}: first seed with margin >= {F64_MIN_MARGIN:g}: {scan_f64_seeds(reg, nm)}", flush=True)
        sys.exit(0)
    if "--scan" in sys.argv:
        i = sys.argv.index("--scan")
        scan_trajectory_seeds(sys.argv[i + 1], [int(x) for x in sys.argv[i + 2:]])
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a != "--check"]
    sys.exit(0 if main(set(argv) or None, check="--check" in sys.argv) else 1)
