#!/usr/bin/env python3
"""Golden vectors of the FAFormer wrappers ``faformer_equihnn`` and ``faformer_equihnnm``: the REFERENCE's own
equihgnn/models/equihnn_fa_former.py (read from the reference checkout at run time, never copied) run on small seeded
batches.

    python tests/golden/make_golden_faformer_paired.py            # (re)write tests/golden/faformer_paired/*.npz
    python tests/golden/make_golden_faformer_paired.py --check    # regenerate and compare bit for bit with the committed files
    python tests/golden/make_golden_faformer_paired.py --scan [names]   # first seeds of the float64 cases that meet F64_MIN_MARGIN
    python tests/golden/make_golden_faformer_paired.py --state-dict-layouts   # reference_state_dicts_faformer_paired.json

It reuses make_golden.py's stand-ins, import machinery, ``run_case`` / ``run_case_f64`` and ``compare``, and common.py's batch
generator and weight filler; no new stand-in is needed.  The tables below have the columns of common.CASE_TABLE / F64_TABLE.

Inputs.  The reference's ``faformer_equihnn`` sizes its hyperedge pool by ``he_batch.max() + 1`` and fails in ``torch.cat``
unless the LAST molecule of the batch has a hyperedge of order > 2 (equihnn_fa_former.py:99-101).  ``common.make_batch``
forces one into the last molecule and puts a one-atom molecule WITHOUT any hyperedge in the middle, so every batch here also
has an earlier molecule whose row of the hyperedge pool is zero; ``check_input_rule`` asserts both.

One correction to what ``run_case`` returns: for a training-mode case with BatchNorm it adds ``out_f64``, the float64 forward
value, from a second model whose dropouts it leaves as constructed -- FAFormer's 0.1 dropouts would be live there.  The
cases concerned run with those dropouts forced to 0 (``dropout0``), so ``out_f64`` is evaluated again here with the same
rule applied; the same float64 pass yields ``tapown_<name>``, the distance of each float32 ``tap_<name>`` from its float64
value (train-mode BatchNorm amplifies float32 rounding from layer to layer: with --normalization bn the reference's own
float32 output of the third layer lies 2.7e-5 of its scale from the float64 one).
"""
from __future__ import annotations

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
from common import F64_MIN_MARGIN, f64_sample_indices, fill_state_dict, golden_args, make_batch, zero_dropouts  # noqa: E402

OUT_DIR = os.path.join(HERE, "faformer_paired")
METHODS = ("faformer_equihnn", "faformer_equihnnm")

# name: (method, hidden, seed, n_mols, train_mode, store_grads, options) -- options as in common.CASE_TABLE.
# Per method: eval and train (FAFormer's dropouts at p = 0) at hidden 64, a PCQM-flavoured batch, and hidden 256 with the
# large gradients stored as their first rows (store_grads False: 64 leading entries and the norms, as the other *_c256 files)
CASE_TABLE = {
    "faformer_equihnn_c64": ("faformer_equihnn", 64, 151, 6, False, True, {}),
    "faformer_equihnn_c64_train_p0": ("faformer_equihnn", 64, 152, 5, True, True, dict(dropout0=True)),
    "faformer_equihnn_pcqm_c64": ("faformer_equihnn", 64, 153, 6, False, True, dict(flavour="pcqm", big=44)),
    "faformer_equihnn_c256": ("faformer_equihnn", 256, 154, 2, False, False, {}),
    "faformer_equihnnm_c64": ("faformer_equihnnm", 64, 161, 6, False, True, {}),
    "faformer_equihnnm_c64_train_p0": ("faformer_equihnnm", 64, 162, 5, True, True, dict(dropout0=True)),
    "faformer_equihnnm_pcqm_c64": ("faformer_equihnnm", 64, 163, 6, False, True, dict(flavour="pcqm", big=44)),
    "faformer_equihnnm_c256": ("faformer_equihnnm", 256, 164, 2, False, False, {}),
    # --normalization bn: BatchNorm inside every MLP as well (mlp.py:29-44), training mode
    "faformer_equihnnm_c64_bn_train_p0": ("faformer_equihnnm", 64, 165, 6, True, True,
                                          dict(dropout0=True, args=dict(normalization="bn"))),
}

# name: (method, hidden, seed, n_mols, train_mode, options) -- the reference in float64, training mode with FAFormer's dropouts
# at 0; the seeds are the first ones from 1520 / 1620 on whose closest ReLU input lies >= F64_MIN_MARGIN rms from zero (--scan)
F64_TABLE = {
    "faformer_equihnn_c64_f64": ("faformer_equihnn", 64, 1520, 5, True, dict(dropout0=True)),
    "faformer_equihnnm_c64_f64": ("faformer_equihnnm", 64, 1620, 5, True, dict(dropout0=True)),
}

# faformer_equihnnm has three unshared conv layers: with every gradient whole a hidden-64 file would pass 1 MiB.  In its files
# a gradient of more than ROW_SUBSET_ABOVE entries (the [64, 128]-shaped Linears of the conv layers, FAFormer's widest) is
# stored as a subset, in the forms the checks already read: float32 cases keep the first 64 entries next to the norm in
# grad_stats (``gradhead_``, as store_grads False does), float64 cases the evenly spread sample of common.f64_sample_indices
# (``g64s_``: every other entry of a [64, 128] matrix).
ROW_SUBSET_ABOVE = 8000


def row_subsets(case, name):
    if not name.startswith("faformer_equihnnm"):
        return case
    for k in [k for k in case if k.startswith(("grad_", "g64_")) and k not in ("grad_names", "grad_present", "grad_stats",
                                                                              "grad_absmax")]:
        if case[k].size > ROW_SUBSET_ABOVE:
            g = case.pop(k).reshape(-1)
            if k.startswith("grad_"):
                case["gradhead_" + k[5:]] = g[:64]
            else:
                case["g64s_" + k[4:]] = g[f64_sample_indices(g.size)]
    return case


_DEFAULTS = dict(flavour="qm9", last_conj=True, big=None, geometry=None, dropout0=False, depth=1, args={})


def case_spec(name: str) -> dict:
    method, hidden, seed, n_mols, train, store, opt = CASE_TABLE[name]
    return dict(_DEFAULTS, name=name, method=method, hidden=hidden, seed=seed, n_mols=n_mols, train=train, store_grads=store,
                **opt)


def f64_spec(name: str) -> dict:
    method, hidden, seed, n_mols, train, opt = F64_TABLE[name]
    return dict(_DEFAULTS, name=name, method=method, hidden=hidden, seed=seed, n_mols=n_mols, train=train, store_grads=True,
                **opt)


def build_model(cls, spec, f64: bool = False):
    """The case's model from a class with the reference's constructor: seeded weights, mode, FAFormer's dropouts."""
    torch.manual_seed(0)
    model = cls(1, golden_args(spec["method"], spec["hidden"], **({} if f64 else spec["args"])))
    fill_state_dict(model, spec["seed"])
    model.train(spec["train"])
    if spec["dropout0"]:
        zero_dropouts(model)
    return model


def check_input_rule(case, name):
    """The last molecule has a hyperedge of order > 2 (the reference runs), an earlier one has none (the zero row)."""
    n_e, order = case["in_n_e"], case["in_e_order"]
    mol = np.repeat(np.arange(n_e.shape[0]), n_e)
    high = np.bincount(mol[order > 2], minlength=n_e.shape[0])
    assert high[-1] > 0 and (high[:-1] == 0).any(), (name, high)
    assert (n_e == 0).any(), (name, n_e)             # ... and one molecule has no hyperedge at all


def run(registry, name):
    if name in F64_TABLE:
        spec = f64_spec(name)
        case = mg.run_case_f64(registry, spec)
        assert float(case["relu_margin"]) >= F64_MIN_MARGIN, (name, float(case["relu_margin"]), "re-run --scan, update the seed")
    else:
        spec = case_spec(name)
        case = mg.run_case(registry, spec)
        if "out_f64" in case:            # (see the module docstring)
            m64 = build_model(registry.get_model_class(spec["method"]), spec).double()
            d64 = make_batch(spec)
            d64.pos, d64.y = d64.pos.double(), d64.y.double()
            taps = {}
            keep = lambda key, pick=lambda o: o: (lambda _m, _i, o: taps.__setitem__(key, pick(o).detach().numpy().copy()))
            m64.atom_encoder.register_forward_hook(keep("atom_encoder"))
            m64.fa_former.register_forward_hook(keep("front_end", lambda o: o[0][0]))
            for i, bn in enumerate(m64.batch_norms):
                bn.register_forward_hook(keep(f"bn{i}"))
            m64.mlp_out.register_forward_pre_hook(lambda _m, i: taps.__setitem__("pool", i[0].detach().numpy().copy()))
            with torch.no_grad():
                case["out_f64"] = m64(d64).numpy()
            # how far the reference's OWN float32 intermediate values lie from its float64 ones, in units of the tensor's
            # scale max(1, max |value|): what a comparison with the float32 ``tap_*`` carries on top of its tolerance
            for k, v in taps.items():
                t32 = case["tap_" + k].astype(np.float64)
                case["tapown_" + k] = np.array(np.abs(t32 - v.reshape(t32.shape)).max() / max(1.0, float(np.abs(t32).max())))
    check_input_rule(case, name)
    return row_subsets(case, name)


def write_state_dict_layouts(path=os.path.join(HERE, "reference_state_dicts_faformer_paired.json")):
    ref = mg.import_reference(("equihnn_fa_former",))
    out = {}
    for m in METHODS:
        sd = ref.get_model_class(m)(1, golden_args(m, 64)).state_dict()
        out[m] = {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(t)}: {json.dumps(out[t], sort_keys=True)}" for t in sorted(out)) + "\n}\n")
    return path


def scan(names, tries=200):
    registry = mg.import_reference(("equihnn_fa_former",))
    for name in names or list(F64_TABLE):
        spec, found = f64_spec(name), None
        for sd in range(spec["seed"], spec["seed"] + tries):
            m = mg.run_case_f64(registry, dict(spec, seed=sd), return_margin_only=True)
            print(f"{name}: seed {sd} relu margin {m:.2e}", flush=True)
            if m >= F64_MIN_MARGIN:
                found = sd
                break
        print(f"{name}: first seed with margin >= {F64_MIN_MARGIN:g}: {found}", flush=True)


def main(only=None, check=False):
    # (one thread and deterministic kernels, as make_golden.main: --check compares bit for bit)
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    registry = mg.import_reference(("equihnn_fa_former",))
    os.makedirs(OUT_DIR, exist_ok=True)
    ok = True
    for name in list(CASE_TABLE) + list(F64_TABLE):
        if only and name not in only:
            continue
        case = run(registry, name)
        path = os.path.join(OUT_DIR, name + ".npz")
        if check:
            with np.load(path, allow_pickle=False) as z:
                ok &= mg.compare(case, {k: z[k] for k in z.files}, name)
            continue
        np.savez_compressed(path, **case)
        out = case["out64" if name in F64_TABLE else "out"]
        print(f"{name}: N={case['in_x'].shape[0]} M={case['in_edge_attr'].shape[0]} out[:3]={out[:3]} "
              f"-> {os.path.getsize(path) / 1024:.0f} KiB")
    return ok


if __name__ == "__main__":
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    if "--state-dict-layouts" in sys.argv:
        print(write_state_dict_layouts())
        sys.exit(0)
    if "--scan" in sys.argv:
        scan([a for a in sys.argv[1:] if a in F64_TABLE])
        sys.exit(0)
    argv = [a for a in sys.argv[1:] if a != "--check"]
    sys.exit(0 if main(set(argv) or None, check="--check" in sys.argv) else 1)
