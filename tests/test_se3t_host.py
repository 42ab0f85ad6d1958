"""Host-side checks of ``se3_transformer_equihnns`` (no GPU): the registry entry, the reference's parameter names and shapes,
the closed-form Q_J matrices and basis values against the values the reference produced (tests/golden/se3t/se3t_Q.npz, signs
included), and the float64 restatement tests/se3t_ref.py against the reference's own float64 run
(se3_transformer_equihnns_c32_f64.npz) to 1e-9 -- which makes the restatement the operand-level oracle of
tests/test_hip_se3t.py."""
import json
import os

import numpy as np
import pytest
import torch

import se3t_ref
from common import GOLDEN_DIR, fill_state_dict, golden_args, load_case

METHOD = "se3_transformer_equihnns"


def _model(hidden):
    from equihgnn_amd.registry import create_model

    torch.manual_seed(0)
    return create_model(METHOD)(1, golden_args(METHOD, hidden))


def test_registry_returns_the_class():
    from equihgnn_amd import models
    from equihgnn_amd.registry import create_model

    assert create_model(METHOD) is models.SE3TransformerEquiHNNS
    assert models.MODELS[METHOD] is models.SE3TransformerEquiHNNS


@pytest.mark.parametrize("hidden", [32, 256])
def test_state_dict_names_and_shapes_are_the_references(hidden):
    layouts = json.load(open(os.path.join(GOLDEN_DIR, "reference_state_dicts_se3t.json")))[f"{METHOD}_c{hidden}"]
    model = _model(hidden)
    mine = {k: [list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()}
    assert mine == layouts
    assert list(mine) == list(layouts) or sorted(mine) == sorted(layouts)
    ref_like = {k: torch.zeros(shape, dtype=getattr(torch, dt.split(".")[1])) for k, (shape, dt) in layouts.items()}
    model.load_state_dict(ref_like, strict=True)
    case = load_case("se3t/se3_transformer_equihnns_c32")
    if hidden == 32:
        assert sorted(n for n, _ in model.named_parameters()) == sorted(str(n) for n in case["grad_names"])


def test_other_constructor_arguments_are_refused():
    from equihgnn_amd.se3_transformer import SE3Transformer

    SE3Transformer(dim=32, heads=2, depth=2, dim_head=32, num_degrees=2, valid_radius=5, num_neighbors=16, splits=2)
    for kw in (dict(heads=4), dict(depth=1), dict(dim_head=24), dict(num_degrees=3), dict(valid_radius=4), dict(num_neighbors=8),
               dict(attend_self=False), dict(reversible=True), dict(use_null_kv=True), dict(output_degrees=2),
               dict(rotary_position=True), dict(num_conv_layers=1), dict(edge_dim=4), dict(global_feats_dim=8)):
        args = dict(dim=32, heads=2, depth=2, dim_head=32, num_degrees=2, valid_radius=5, num_neighbors=16)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            SE3Transformer(**args)


def test_q_matrices_equal_the_references_signs_included():
    from equihgnn_amd.se3_transformer import Q_SIGNS, flip_q_sign, q_matrices, q_table

    with np.load(os.path.join(GOLDEN_DIR, "se3t", "se3t_Q.npz")) as z:
        q = q_matrices(torch.float64)
        assert len(q) == 6
        for (di, do, j), mat in q.items():
            ref = z[f"Q_{di}{do}_{j}"]
            assert mat.shape == ref.shape
            assert np.abs(mat.numpy() - ref).max() <= 1e-6, (di, do, j)
    assert q_table().shape == (100,)
    before = dict(Q_SIGNS)
    flip_q_sign(1, 1, 1)
    try:
        assert torch.equal(q_matrices()[(1, 1, 1)], -q[(1, 1, 1)]) and torch.equal(q_matrices()[(1, 1, 2)], q[(1, 1, 2)])
    finally:
        flip_q_sign(1, 1, 1)
    assert Q_SIGNS == before


def test_spherical_harmonics_and_basis_equal_the_references():
    """Fixed unit vectors, +-z (where the reference's atan2 sits at its branch) and +-y (its poles) among them."""
    with np.load(os.path.join(GOLDEN_DIR, "se3t", "se3t_Q.npz")) as z:
        v = torch.from_numpy(z["unit_vectors"])
        for j, y in enumerate(se3t_ref.real_sh(v)):
            assert np.abs(y.numpy() - z[f"Y_{j}"]).max() <= 1e-6, j
        bas = se3t_ref.basis(v)
        for (di, do), b in bas.items():
            ref = z[f"basis_{di}{do}"].reshape(b.shape)          # [V, 1, mo, 1, mi, F]
            assert np.abs(b.numpy() - ref).max() <= 1e-6, (di, do)


@pytest.fixture(scope="module")
def f64_case():
    case = load_case("se3t/se3_transformer_equihnns_c32_f64")
    model = _model(32)
    fill_state_dict(model, int(case["meta_seed"]))
    sd = {k: v.double() for k, v in model.state_dict().items()}
    taps = {}
    with torch.no_grad():
        se3t_ref.front_end(sd, torch.from_numpy(case["tap_atom_encoder"]), torch.from_numpy(case["in_pos"]).double(), taps=taps)
    return case, taps


@pytest.mark.parametrize("tap", ["conv_in0", "conv_in1", "block0_0", "block0_1", "block1_0", "block1_1", "front_end"])
def test_float64_restatement_reproduces_the_reference(f64_case, tap):
    case, taps = f64_case
    ref = case["tap_" + tap]
    got = taps[tap].numpy()
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (tap, np.abs(got - ref).max())


def test_fixture_covers_the_cases_it_is_for():
    case = load_case("se3t/se3_transformer_equihnns_c32")
    cnt = case["valid_counts"]
    assert case["in_x"].shape[0] >= 40 and cnt.min() == 0 and ((cnt > 0) & (cnt < 16)).any() and (cnt == 16).any()
    assert (case["in_e_order"] > 2).any()
    assert load_case("se3t/se3_transformer_equihnns_tiny")["in_x"].shape[0] == 5
