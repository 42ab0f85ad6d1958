"""Host checks of the two FAFormer wrappers ``faformer_equihnn`` / ``faformer_equihnnm`` and of the paired pool's C ABI:
registry names, the drop-in install, state_dict layouts against the reference's (tests/golden/
reference_state_dicts_faformer_paired.json, written from the reference by make_golden_faformer_paired.py
--state-dict-layouts), the header's declarations and their ctypes binding.  No GPU."""
import json
import os
import re
import subprocess
import sys
import textwrap
from ctypes import c_int32, c_int64, c_void_p

import pytest
import torch

from common import GOLDEN_DIR, golden_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("faformer_equihnn", "faformer_equihnnm")


def _layouts():
    with open(os.path.join(GOLDEN_DIR, "reference_state_dicts_faformer_paired.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("method", METHODS)
def test_names_resolve(method):
    from equihgnn_amd import models
    from equihgnn_amd.registry import create_model, registry
    cls = registry.get_model_class(method)
    assert cls is not None and create_model(method) is cls and models.MODELS[method] is cls
    assert cls.__name__ == {"faformer_equihnn": "FAFormerEquiHNN", "faformer_equihnnm": "FAFormerEquiHNNM"}[method]


@pytest.mark.parametrize("method", METHODS)
def test_state_dict_layout_is_the_reference_s(method):
    from equihgnn_amd import models
    model = models.MODELS[method](1, golden_args(method, 64))
    got = {k: [list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()}
    want = _layouts()[method]
    assert sorted(got) == sorted(want)
    assert got == want
    assert len(want) == {"faformer_equihnn": 156, "faformer_equihnnm": 219}[method]
    # strict loading both ways: a state_dict of the reference's layout into the class, and the class's own back
    blank = {k: torch.zeros(shape, dtype=getattr(torch, dt.split(".")[1])) for k, (shape, dt) in want.items()}
    model.load_state_dict(blank, strict=True)
    models.MODELS[method](1, golden_args(method, 64)).load_state_dict(model.state_dict(), strict=True)


def test_only_faformer_equihnn_takes_the_fused_pool():
    """mhnn, egnn_equihnn and visnet_equihnn keep their read-out (its sum order is under existing golden tolerances)."""
    from equihgnn_amd import models
    assert models.FAFormerEquiHNN.fused_pool is True
    for name in ("mhnn", "egnn_equihnn", "visnet_equihnn"):
        assert models.MODELS[name].fused_pool is False, name


def test_head_of_faformer_equihnn_is_twice_as_wide():
    from equihgnn_amd import models
    m = models.MODELS["faformer_equihnn"](1, golden_args("faformer_equihnn", 64))
    assert m.mlp_out.lins[0].weight.shape == (64, 128)          # output_hidden * 2 = 64 rows, MLP_hidden * 2 = 128 columns
    assert not hasattr(m, "egnn_layer") and not hasattr(m, "layers")
    mm = models.MODELS["faformer_equihnnm"](1, golden_args("faformer_equihnnm", 64))
    assert mm.mlp_out.lins[0].weight.shape == (32, 64) and len(mm.layers) == len(mm.batch_norms) == 3


CHILD = textwrap.dedent('''
    import sys, types
    sys.path[:0] = [sys.argv[1]]

    class Registry:                       # stand-in of the reference's registry interface (equihgnn/common/registry.py)
        mapping = {"model_name_mapping": {}}

        @classmethod
        def get_model_class(cls, name):
            return cls.mapping["model_name_mapping"].get(name, None)
    ref = Registry()
    stock = {n: type(n, (), {"__module__": "equihgnn.models.equihnn_fa_former"}) for n in sys.argv[2:]}
    ref.mapping["model_name_mapping"].update(stock)
    mods = {m: types.ModuleType(m) for m in ("equihgnn", "equihgnn.common", "equihgnn.common.registry")}
    mods["equihgnn.common.registry"].registry = ref
    sys.modules.update(mods)

    from equihgnn_amd import models as M
    from equihgnn_amd.registry import install_into_reference
    kept = install_into_reference(override=False)
    assert not (set(kept) & set(stock)) and all(ref.get_model_class(n) is stock[n] for n in stock)
    done = install_into_reference()
    for n in stock:
        assert n in done and ref.get_model_class(n) is M.MODELS[n], n
    print("INSTALL-OK", len(done))
''')


def test_install_into_reference_installs_both_names():
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, *METHODS], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTALL-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_header_declares_the_paired_pool_and_hip_binds_it():
    from equihgnn_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "equihgnn_hip.h")).read(), flags=re.S)
    for name in ("hg_pool_pair_fwd", "hg_pool_pair_bwd"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in hip.SIGNATURES and hip.SIGNATURES[name][0] is c_int32
    p, i64, i32 = c_void_p, c_int64, c_int32
    assert hip.SIGNATURES["hg_pool_pair_fwd"][1] == [p, p, p, i64, p, p, p, p, i64, p, i64, i32, p]
    assert hip.SIGNATURES["hg_pool_pair_bwd"][1] == [p, p, i64, p, p, i64, p, p, i64, i32, p]


def test_library_exports_the_paired_pool_and_refuses_bad_arguments():
    """The argument checks run before any launch, so they answer without a GPU."""
    from equihgnn_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    a = c_void_p(1 << 20)           # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    odd = c_void_p((1 << 20) + 4)
    fwd = lambda x=a, n_x=8, e=a, n_e=8, out=a, B=2, C=64, rp=a: L.hg_pool_pair_fwd(x, rp, None, n_x, e, a, None, a, n_e, out, B,
                                                                                   C, None)
    assert fwd(C=0) == hip.EQH_ERR_ARG and fwd(n_x=-1) == hip.EQH_ERR_ARG and fwd(B=-1) == hip.EQH_ERR_ARG
    assert fwd(out=None) == hip.EQH_ERR_ARG and fwd(x=None) == hip.EQH_ERR_ARG and fwd(rp=None) == hip.EQH_ERR_ARG
    assert fwd(e=None) == hip.EQH_ERR_ARG
    assert fwd(C=66) == hip.EQH_ERR_ALIGN and fwd(x=odd) == hip.EQH_ERR_ALIGN and fwd(e=odd) == hip.EQH_ERR_ALIGN
    assert fwd(C=1028) == hip.EQH_ERR_RANGE and fwd(n_x=1 << 31) == hip.EQH_ERR_RANGE and fwd(B=1 << 30) == hip.EQH_ERR_RANGE
    assert fwd(B=0) == hip.EQH_OK                                    # nothing to do, nothing launched
    bwd = lambda d=a, n_x=8, n_e=8, dx=a, de=a, B=2, C=64, xm=a: L.hg_pool_pair_bwd(d, xm, n_x, a, a, n_e, dx, de, B, C, None)
    assert bwd(C=-4) == hip.EQH_ERR_ARG and bwd(n_e=-1) == hip.EQH_ERR_ARG and bwd(dx=None) == hip.EQH_ERR_ARG
    assert bwd(de=None) == hip.EQH_ERR_ARG and bwd(d=None) == hip.EQH_ERR_ARG and bwd(xm=None) == hip.EQH_ERR_ARG
    assert bwd(C=6) == hip.EQH_ERR_ALIGN and bwd(dx=odd) == hip.EQH_ERR_ALIGN and bwd(de=odd) == hip.EQH_ERR_ALIGN
    assert bwd(C=2048) == hip.EQH_ERR_RANGE and bwd(n_e=1 << 31) == hip.EQH_ERR_RANGE
    assert bwd(n_x=0, n_e=0) == hip.EQH_OK


def test_pool_pair_refuses_cpu_tensors():
    from equihgnn_amd import hip, ops
    from equihgnn_amd.ops.readout import _PoolPair
    assert ops.pool_pair is ops.readout.pool_pair
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        _PoolPair.apply(torch.zeros(4, 8), torch.zeros(2, 8), None, None, None, None, torch.zeros(2, dtype=torch.int64))
