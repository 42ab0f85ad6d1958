"""Host (no GPU): the three ViSNet wrappers are registered, keep the reference's module tree, and the radius-graph
restatement the GPU tests compare against keeps the first 16 atoms of each molecule in index order."""
import pytest
import torch

import visnet_ref

NAMES = ("visnet_equihnn", "visnet_equihnns", "visnet_equihnnm")


def _args(**kw):
    from equihgnn_amd.registry import default_args
    return default_args(MLP_hidden=64, output_hidden=32, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_registry_serves_the_visnet_names(name):
    import equihgnn_amd.models as models
    from equihgnn_amd.registry import registry
    cls = registry.get_model_class(name)
    assert cls is not None and cls is models.MODELS[name]
    assert cls.__module__ == "equihgnn_amd.models"


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_has_the_reference_layout(name):
    from equihgnn_amd.registry import registry
    m = registry.get_model_class(name)(1, _args())
    sd = m.state_dict()
    C = 64
    v = "visnet_layer."
    rm = v + "representation_model."
    assert not any(k.startswith("atom_encoder.") for k in sd)
    want = {
        rm + "embedding.atom_embedding_list.0.weight": None,
        rm + "distance_expansion.means": (32,),
        rm + "distance_expansion.betas": (32,),
        rm + "neighbor_embedding.embedding.atom_embedding_list.8.weight": None,
        rm + "neighbor_embedding.distance_proj.weight": (C, 32),
        rm + "neighbor_embedding.combine.weight": (C, 2 * C),
        rm + "edge_embedding.edge_proj.weight": (C, 32),
        rm + "vis_mp_layers.0.vec_layernorm.weight": (C,),
        rm + "vis_mp_layers.0.vec_proj.weight": (3 * C, C),
        rm + "vis_mp_layers.4.f_proj.bias": (C,),
        rm + "vis_mp_layers.4.w_src_proj.weight": (C, C),
        rm + "vis_mp_layers.5.o_proj.weight": (3 * C, C),
        rm + "vis_mp_layers.5.s_proj.weight": (2 * C, C),
        rm + "out_norm.weight": (C,),
        rm + "vec_out_norm.weight": (C,),
        v + "output_model.output_network.1.vec2_proj.weight": (C, C),
        v + "output_model.output_network.1.update_net.2.weight": (2 * C, C),
        v + "output_model.output_network.0.update_net.0.weight": (C, 2 * C),
        v + "mean": (),
        v + "std": (),
    }
    for k, shape in want.items():
        assert k in sd, k
        if shape is not None:
            assert tuple(sd[k].shape) == shape, k
    last = rm + "vis_mp_layers.5."
    assert not any(k.startswith(last + p) for k in sd for p in ("f_proj", "w_src_proj", "w_trg_proj"))
    assert len([k for k in sd if k.startswith(rm + "vis_mp_layers.")]) == 5 * 22 + 18
    with torch.no_grad():
        m.load_state_dict({k: t.clone() for k, t in sd.items()}, strict=True)


def test_channels_must_divide_into_heads():
    from equihgnn_amd.visnet import ViSNet
    with pytest.raises(ValueError, match="evenly divisible"):
        ViSNet(hidden_channels=60, lmax=2, max_num_neighbors=16)


@pytest.mark.parametrize("kw", [dict(vertex=True), dict(vecnorm_type="max_min"), dict(trainable_rbf=True),
                                dict(derivative=True)])
def test_unbuilt_variants_raise(kw):
    from equihgnn_amd.visnet import ViSNet
    with pytest.raises(NotImplementedError):
        ViSNet(hidden_channels=64, lmax=2, max_num_neighbors=16, **kw)


def test_standin_radius_graph_keeps_first_16_in_index_order():
    g = torch.Generator().manual_seed(0)
    # molecule 0: 24 atoms packed in a 3 A box (every pair within 5 A); molecule 1: 5 atoms in the same box; molecule 2:
    # one atom; molecule 3: two atoms 7 A apart
    pos = torch.cat([torch.rand(24, 3, generator=g) * 3, torch.rand(5, 3, generator=g) * 3, torch.zeros(1, 3),
                     torch.tensor([[0.0, 0.0, 0.0], [7.0, 0.0, 0.0]])])
    batch = torch.tensor([0] * 24 + [1] * 5 + [2] + [3] * 2)
    ei = visnet_ref.radius_graph(pos, batch)
    src, dst = ei
    assert torch.all(batch[src] == batch[dst])                    # no edge between molecules
    for i in range(pos.shape[0]):
        s = src[dst == i]
        mol = torch.nonzero(batch == batch[i]).reshape(-1)
        if batch[i] == 0:
            assert s.tolist() == mol[:16].tolist()                # truncation binds: the first 16, self included
        elif batch[i] == 1:
            assert s.tolist() == mol.tolist()
        else:
            assert s.tolist() == [i]                              # lone atom / no neighbour in radius: self-loop only
    assert torch.all(dst[1:] >= dst[:-1])                         # by target, then source
    keep = dst[1:] == dst[:-1]
    assert torch.all(src[1:][keep] > src[:-1][keep])
    pad = visnet_ref.radius_graph(pos, batch, n_real=29)
    assert pad[:, pad[1] >= 29].tolist() == [[29, 30, 31], [29, 30, 31]]


def test_state_dicts_equal_the_reference_layouts():
    """reference_state_dicts_visnet.json: the reference's three classes built with make_golden_visnet.py's stand-ins."""
    import json
    import os

    import equihgnn_amd.models  # noqa: F401
    from common import GOLDEN_DIR, golden_args
    from equihgnn_amd.registry import registry
    with open(os.path.join(GOLDEN_DIR, "reference_state_dicts_visnet.json")) as f:
        ref = json.load(f)
    assert sorted(ref) == sorted(NAMES)
    for name in NAMES:
        sd = registry.get_model_class(name)(1, golden_args(name, 64)).state_dict()
        assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()} == ref[name], name


def test_golden_generator_regenerates_bit_for_bit():
    import os
    import subprocess
    import sys

    from common import GOLDEN_DIR
    import make_golden
    if not os.path.isdir(os.path.join(make_golden.REF, "equihgnn", "models")):
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN_DIR, "make_golden_visnet.py"), "--check"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
