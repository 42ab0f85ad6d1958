#!/usr/bin/env python3
"""Golden vectors of ``se3_transformer_equihnns``: the REFERENCE's own equihgnn/models/equihnn_se3_transformer.py and
equihgnn/models/layers/se3_transformer_layer.py (read from the reference checkout at run time, never copied) on small seeded
batches, in float32 and in float64.

    python tests/golden/make_golden_se3t.py            # (re)write the four fixtures and the state-dict layouts
    python tests/golden/make_golden_se3t.py --check    # regenerate and compare with the committed files

It reuses make_golden.py's stand-ins and import recipe.  se3_transformer/irr_repr.py:20-26 loads data/J_dense.pt, a blob the
reference checkout lacks (as the Equiformer's is): the reconstructed J_0, J_1, J_2 of SURVEY.md section 8c are supplied through
the same patched ``torch.load``.  The basis cache on disk is switched off (CLEAR_CACHE).

Written:
  reference_state_dicts_se3t.json         names and shapes of the stock class at C = 32 and C = 256
  se3t/se3t_Q.npz                         the Q_J the reference's SVD produced here, and Y_J / basis values for fixed unit vectors
  se3t/se3_transformer_equihnns_c32.npz     float32 run: 6 molecules + a one-atom molecule, one atom moved beyond every radius
  se3t/se3_transformer_equihnns_c32_f64.npz    the same batch and weights in float64
  se3t/se3_transformer_equihnns_tiny.npz     N = 5 (k = 4 < 16), float32, with the float64 output beside it

Weights are not stored: both sides derive them from the seed (common.fill_state_dict).  The reference zero-initialises no layer
of this model (checked here: every parameter of a freshly built stock model but the LayerNorm biases is non-zero).  Gradients:
(sum, sum |g|, norm) of every parameter, whole gradients up to 1024 entries and an evenly spread sample of 128 entries
(grad_sample_indices) above, so each file stays within the size of the other fixtures.

Every case keeps each selected neighbour's distance at least 1e-3 from the radius and has no tie at the 16th neighbour, so the
graph is the same in float32 and float64.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "se3t")     # (tests/golden itself holds the case-table files only: tests/test_golden_inputs.py)
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from common import _kth_neighbour_ties, fill_state_dict, golden_args, make_batch  # noqa: E402

METHOD = "se3_transformer_equihnns"
# name: (hidden, seed, float64, tiny)
CASES = {
    "se3_transformer_equihnns_c32": (32, 131, False, False),
    "se3_transformer_equihnns_c32_f64": (32, 131, True, False),
    "se3_transformer_equihnns_tiny": (32, 132, False, True),
}
GRAD_FULL_LIMIT, GRAD_SAMPLE = 1024, 128     # gradients of at most 1024 entries are stored whole, larger ones as a sample


def grad_sample_indices(numel: int) -> np.ndarray:
    """Flat indices of the stored sample of a large gradient: GRAD_SAMPLE entries evenly spread over the tensor."""
    return np.unique(np.linspace(0, numel - 1, GRAD_SAMPLE).astype(np.int64))


UNIT_VECTORS = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0.6, 0.8, 0], [0.3, -0.5, 0.8],
                         [-0.7, 0.1, -0.2], [1e-4, 1.0, -1e-4]], dtype=np.float64)


def import_reference_se3t():
    mg.install_standins()
    os.environ["CLEAR_CACHE"] = "1"
    sys.path.insert(0, mg.REF)
    for pkg, sub in (("equihgnn.models", "equihgnn/models"), ("equihgnn.models.layers", "equihgnn/models/layers")):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(mg.REF, sub)]
        sys.modules[pkg] = m
    real_load = torch.load

    def patched_load(path, *a, **k):
        if str(path).endswith("J_dense.pt"):
            return mg.reconstructed_J()
        return real_load(path, *a, **k)

    torch.load = patched_load
    try:
        importlib.import_module("equihgnn.models.layers.se3_transformer.irr_repr")
    finally:
        torch.load = real_load
    importlib.import_module("equihgnn.models.equihnn_se3_transformer")
    return importlib.import_module("equihgnn.common.registry").registry


def case_batch(name):
    hidden, seed, _, tiny = CASES[name]
    from equihgnn_amd.batch import collate, synth_molecule
    for s in range(seed, seed + 1000, 7):
        if tiny:
            rng = np.random.default_rng(s)
            b = collate([synth_molecule(rng, "qm9", n_atoms=5, force_conj=False)])
        else:
            b = make_batch(s, n_mols=6, last_conj=True)
            pos = b.pos.clone()
            far = int(torch.nonzero(b.batch == 2).reshape(-1)[-1])
            pos[far] = pos[far] + 30.0                     # no neighbour within the radius: every slot masked
            pos[b.batch == 4] += torch.tensor([14.0, 0.0, 0.0])       # a molecule on its own: fewer than 16 in radius
            b.pos = pos
        p = b.pos.double()
        d = (p[:, None] - p[None]).norm(dim=-1)
        d.fill_diagonal_(float("inf"))
        k = min(16, p.shape[0] - 1)
        near = d.sort(dim=-1).values[:, :k]
        if _kth_neighbour_ties(b.pos.numpy()) == 0 and float((near - 5.0).abs().min()) >= 1e-3:
            return b, s, (near <= 5.0).sum(-1)
    raise RuntimeError(name)


def build_model(registry, hidden, seed, dtype):
    torch.manual_seed(0)
    model = registry.get_model_class(METHOD)(1, golden_args(METHOD, hidden))
    fill_state_dict(model, seed)
    return model.to(dtype).train()


def run(model, b, dtype):
    data = b
    data.pos, data.y = b.pos.to(dtype), b.y.to(dtype)
    taps = {}
    se3 = model.se3_transformer_layer
    hooks = [model.atom_encoder.register_forward_hook(lambda _m, _i, o: taps.__setitem__("atom_encoder", o.detach().clone())),
             se3.conv_in.register_forward_hook(lambda _m, _i, o: taps.update(conv_in0=o["0"][0].detach().clone(),
                                                                             conv_in1=o["1"][0].detach().clone())),
             se3.register_forward_hook(lambda _m, _i, o: taps.__setitem__("front_end", o[0].detach().clone()))]
    for i, blk in enumerate(se3.net.blocks):
        hooks.append(blk[1].register_forward_hook(
            lambda _m, _i, o, i=i: taps.update({f"block{i}_0": o["0"][0].detach().clone(), f"block{i}_1": o["1"][0].detach().clone()})))
    out = model(data)
    loss = torch.nn.functional.mse_loss(out, data.y)
    loss.backward()
    for h in hooks:
        h.remove()
    return out, loss, taps


def run_case(registry, name):
    hidden, seed, f64, tiny = CASES[name]
    dtype = torch.float64 if f64 else torch.float32
    b, used_seed, counts = case_batch(name)
    if not tiny:
        assert b.x.shape[0] >= 40 and int(counts.min()) == 0 and int(((counts > 0) & (counts < 16)).sum()) > 0
        assert int((b.e_order > 2).sum()) > 0
    case = {"meta_method": np.array(METHOD), "meta_hidden": np.array(hidden), "meta_seed": np.array(seed),
            "meta_batch_seed": np.array(used_seed), "valid_counts": counts.numpy()}
    for k in ("x", "pos", "edge_index0", "edge_index1", "edge_attr", "n_e", "e_order", "batch", "y"):
        v = getattr(b, k)
        case["in_" + k] = (v.float() if k in ("pos", "y") else v).numpy()
    model = build_model(registry, hidden, seed, dtype)
    out, loss, taps = run(model, b, dtype)
    for k, v in taps.items():
        case["tap_" + k] = v.numpy()
    case["out"], case["loss"] = out.detach().numpy(), loss.detach().numpy()
    names, present, stats = [], [], []
    for n, p in model.named_parameters():
        names.append(n)
        present.append(p.grad is not None)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        stats.append([float(g.double().sum()), float(g.double().abs().sum()), float(g.double().norm())])
        if p.grad is not None:
            flat = g.reshape(-1)
            case["grad_" + n] = (flat if flat.numel() <= GRAD_FULL_LIMIT else flat[torch.from_numpy(grad_sample_indices(flat.numel()))]).numpy()
    case["grad_names"], case["grad_present"] = np.array(names), np.array(present)
    case["grad_stats"] = np.array(stats, dtype=np.float64)
    if not f64:
        # the reference's own float64 run beside the float32 one: the measured float32 error is what the test bounds come from
        m64 = build_model(registry, hidden, seed, torch.float64)
        b64, _, _ = case_batch(name)
        out64, loss64, _ = run(m64, b64, torch.float64)
        case["out_f64"], case["loss_f64"] = out64.detach().numpy(), loss64.detach().numpy()
        gmax, gerr = [], []
        for (n, p), (_, p64) in zip(model.named_parameters(), m64.named_parameters()):
            gmax.append(float(p64.grad.abs().max()))
            gerr.append(float((p.grad.double() - p64.grad).abs().max()))
        case["ref_f32_grad_err"], case["ref_f64_grad_max"] = np.array(gerr), np.array(gmax)
    return case


def write_q(path=os.path.join(OUT_DIR, "se3t_Q.npz")):
    basis = importlib.import_module("equihgnn.models.layers.se3_transformer.basis")
    out = {"unit_vectors": UNIT_VECTORS / np.linalg.norm(UNIT_VECTORS, axis=1, keepdims=True)}
    for di, do in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for j in range(abs(di - do), di + do + 1):
            out[f"Q_{di}{do}_{j}"] = basis.basis_transformation_Q_J(j, di, do).double().numpy()
    v = torch.from_numpy(out["unit_vectors"])[None, None]              # [1, 1, V, 3] as neighbor_rel_pos is [b, n, k, 3]
    for key, t in basis.get_basis(v, 1).items():
        out["basis_" + key.replace(",", "")] = t[0, 0].numpy()
    sph = basis.get_spherical_from_cartesian(v)
    for j, y in basis.precompute_sh(sph, 2).items():
        out[f"Y_{j}"] = y[0, 0].numpy()
    np.savez_compressed(path, **out)
    return path


def write_state_dict_layouts(registry, path=os.path.join(HERE, "reference_state_dicts_se3t.json")):
    out = {}
    for hidden in (32, 256):
        model = registry.get_model_class(METHOD)(1, golden_args(METHOD, hidden))
        sd = model.state_dict()
        zero = [k for k, v in sd.items() if v.is_floating_point() and float(v.abs().max()) == 0.0]
        assert all(k.endswith(("rp.net.1.bias", "rp.net.4.bias")) or "normalizations" in k for k in zero), zero   # LayerNorm biases only
        out[f"{METHOD}_c{hidden}"] = {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(t)}: {json.dumps(out[t], sort_keys=True)}" for t in sorted(out)) + "\n}\n")
    return path


def main(check=False):
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    registry = import_reference_se3t()
    ok = True
    os.makedirs(OUT_DIR, exist_ok=True)
    if not check:
        print(write_state_dict_layouts(registry))
        print(write_q())
    for name in CASES:
        case = run_case(registry, name)
        path = os.path.join(OUT_DIR, name + ".npz")
        if check:
            with np.load(path) as z:
                ok &= mg.compare(case, dict(z), name)
            continue
        np.savez_compressed(path, **case)
        extra = ""
        if "out_f64" in case:
            rel = case["ref_f32_grad_err"] / np.maximum(case["ref_f64_grad_max"], 1e-300)
            extra = (f" ref fp32-vs-f64: out {np.abs(case['out'] - case['out_f64']).max():.3e} loss "
                     f"{abs(float(case['loss']) - float(case['loss_f64'])):.3e} grad/max {rel.max():.3e}")
        print(f"{name}: N={case['in_x'].shape[0]} seed={int(case['meta_batch_seed'])} counts min/max "
              f"{case['valid_counts'].min()}/{case['valid_counts'].max()} out[:3]={case['out'][:3]}{extra} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(check="--check" in sys.argv) else 1)
