"""Device collate, the parts that need no GPU: the four symbols of csrc/collate_dev.hip are declared, exported and bound; the
argument checks return their codes before any launch (nothing here touches a device: the pointers are never followed); the
workspace query; Store.to_device on a CPU device raises."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("hb_collate_dev", "hb_collate_dev_workspace_bytes", "gb_collate_dev", "gb_collate_dev_workspace_bytes")
FAKE = 0x1000       # a non-NULL address for pointers the checks only compare with NULL


def test_the_four_symbols_are_declared_exported_and_bound():
    from equihgnn_amd import hip
    with open(hip.HEADER) as f:
        text = f.read()
    L = hip.lib()
    for name in SYMBOLS:
        assert f" {name}(" in text and name in hip.SIGNATURES
        assert getattr(L, name).argtypes == hip.SIGNATURES[name][1]
    assert hip.SIGNATURES["hb_collate_dev"] == (ctypes.c_int32, [ctypes.POINTER(hip.HbCollateDev), ctypes.c_void_p])
    assert hip.SIGNATURES["gb_collate_dev"] == (ctypes.c_int32, [ctypes.POINTER(hip.GbCollateDev), ctypes.c_void_p])
    assert hip.SIGNATURES["hb_collate_dev_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    assert hip.SIGNATURES["gb_collate_dev_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    # the host structs' fields, in order, then the workspace
    for dev, host in ((hip.HbCollateDev, hip.HbCollate), (hip.GbCollateDev, hip.GbCollate)):
        names = [n for n, _ in dev._fields_]
        assert names[:len(host._fields_)] == [n for n, _ in host._fields_]
        assert names[len(host._fields_):] == ["workspace", "workspace_bytes"]


def _full(cls, L, B=2, **kw):
    """An argument block every check accepts (fake addresses): the tests below break one thing each."""
    from equihgnn_amd import hip
    a = cls()
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p:
            setattr(a, name, FAKE)
    a.B, a.n_mols, a.padded, a.PN = B, 10, 1, 64
    if cls is hip.HbCollateDev:
        a.PM, a.PZ = 64, 128
        a.workspace_bytes = L.hb_collate_dev_workspace_bytes(B)
    else:
        a.PE, a.F = 128, 3
        a.workspace_bytes = L.gb_collate_dev_workspace_bytes(B)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("form", ["h", "g"])
def test_argument_checks_return_their_codes_without_a_device(form):
    from equihgnn_amd import hip
    L = hip.lib()
    cls, fn = (hip.HbCollateDev, L.hb_collate_dev) if form == "h" else (hip.GbCollateDev, L.gb_collate_dev)
    call = lambda **kw: fn(ctypes.byref(_full(cls, L, **kw)), None)
    assert fn(None, None) == hip.EQH_ERR_ARG                                  # no argument block
    assert call(B=-1) == hip.EQH_ERR_ARG
    assert call(out_counts=None) == hip.EQH_ERR_ARG
    assert call(idx=None) == hip.EQH_ERR_ARG                                  # B > 0 molecules and no index
    assert call(node_off=None) == hip.EQH_ERR_ARG
    assert call(y=None) == hip.EQH_ERR_ARG
    for out in ("out_x", "out_batch", "out_y") + (("out_pos", "out_edge_index0", "out_edge_index1", "out_edge_attr",
                                                   "out_e_order", "out_n_e") if form == "h" else
                                                  ("out_edge_index", "out_edge_attr")):
        assert call(**{out: None}) == hip.EQH_ERR_ARG, out                    # an output whose extent is positive
    assert call(workspace=None) == hip.EQH_ERR_ARG
    small = _full(cls, L)
    small.workspace_bytes -= 1
    assert fn(ctypes.byref(small), None) == hip.EQH_ERR_ARG                   # a workspace smaller than the query
    assert call(PN=0, out_x=None, out_batch=None, out_pos=None) == hip.EQH_ERR_RANGE      # no room for the padding atom
    if form == "h":
        assert call(PM=0, out_edge_attr=None, out_e_order=None) == hip.EQH_ERR_RANGE       # ... for its hyperedge
        assert call(PZ=-1) == hip.EQH_ERR_ARG
    else:
        assert call(F=-1) == hip.EQH_ERR_ARG
        assert call(PE=-1) == hip.EQH_ERR_ARG


def test_workspace_query_is_monotone_and_holds_the_three_prefixes():
    from equihgnn_amd import hip
    L = hip.lib()
    for fn, columns in ((L.hb_collate_dev_workspace_bytes, 3), (L.gb_collate_dev_workspace_bytes, 2)):
        sizes = [fn(B) for B in (0, 1, 2, 63, 64, 255, 256, 257, 1024, 4096, 1 << 20)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        for B, s in zip((0, 1, 2, 63, 64, 255, 256, 257, 1024, 4096, 1 << 20), sizes):
            assert s >= columns * (B + 1) * 8 and s % 8 == 0


def test_to_device_on_a_cpu_device_raises():
    from equihgnn_amd import hip
    from equihgnn_amd.batch import GraphStore, MolStore, synth_graph, synth_molecule
    rng = np.random.default_rng(0)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        MolStore([synth_molecule(rng) for _ in range(3)]).to_device("cpu")
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        GraphStore([synth_graph(rng) for _ in range(3)]).to_device(torch_cpu())


def torch_cpu():
    import torch
    return torch.device("cpu")
