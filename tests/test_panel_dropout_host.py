"""Host-side checks of the training dropout on the MHNNConv panel kernels (no GPU): hg_conv_panel_drop / HgConvDrop are
declared and exported, the entry validates its arguments before any launch, and the package switch reaches its owner."""
import ctypes


def test_header_declares_and_library_exports_the_panel_dropout_entry():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    assert "hg_conv_panel_drop" in hip.SIGNATURES, "hg_conv_panel_drop is not declared in include/equihgnn_hip.h"
    assert hasattr(handle, "hg_conv_panel_drop"), "hg_conv_panel_drop declared in the header but not exported"
    res, args = hip.SIGNATURES["hg_conv_panel_drop"]
    assert res is ctypes.c_int32
    assert args == [ctypes.c_int32, ctypes.POINTER(hip.HgConvPanel), ctypes.POINTER(hip.HgConvDrop), ctypes.c_void_p]
    assert [(n, t) for n, t in hip.HgConvDrop._fields_] == [
        ("p_inc", ctypes.c_float), ("seed_inc", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("p", ctypes.c_float),
        ("seed", ctypes.c_void_p)]
    # the sibling leaves hg_conv_panel's own signature alone
    assert hip.SIGNATURES["hg_conv_panel"] == (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(hip.HgConvPanel), ctypes.c_void_p])


def _args(hip, rows=4, C=64, **kw):
    a = hip.HgConvPanel()
    a.rows, a.C = rows, C
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _drop(hip, p_inc=0.0, p=0.0, **kw):
    d = hip.HgConvDrop()
    d.p_inc, d.p = p_inc, p
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_panel_dropout_entry_validates_before_launching():
    from equihgnn_amd import hip

    L = hip.lib()
    held = ctypes.create_string_buffer(256)
    a16 = (ctypes.addressof(held) + 15) & ~15           # a non-null, 16-byte aligned host address: never dereferenced here
    call = lambda stage, a, d: L.hg_conv_panel_drop(stage, a, d, None)
    F3, B3 = hip.HG_CONV_F3, hip.HG_CONV_B3
    # null argument blocks
    assert call(F3, None, _drop(hip)) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip), None) == hip.EQH_ERR_ARG
    # nothing to do -- but the probabilities are looked at first
    assert call(F3, _args(hip, rows=0), _drop(hip, p=0.25, seed=a16)) == hip.EQH_OK
    assert call(B3, _args(hip, rows=0), _drop(hip, p=0.25, seed=a16)) == hip.EQH_OK
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert call(F3, _args(hip, rows=0), _drop(hip, p=bad, seed=a16)) == hip.EQH_ERR_ARG, bad
        assert call(F3, _args(hip, rows=0, rowptr=a16), _drop(hip, p_inc=bad, seed_inc=a16, perm=a16)) == hip.EQH_ERR_ARG, bad
        assert call(B3, _args(hip, rows=0), _drop(hip, p=bad, seed=a16)) == hip.EQH_ERR_ARG, bad
    # only F3 and B3 have a dropout form, and neither with a tail
    for stage in (hip.HG_CONV_F1, hip.HG_CONV_F2, hip.HG_CONV_B1, hip.HG_EGNN_NODE_F, hip.HG_EGNN_NODE_B, 0, 99):
        assert call(stage, _args(hip, rows=0), _drop(hip, p=0.25, seed=a16)) == hip.EQH_ERR_ARG, stage
    assert call(F3, _args(hip, rows=0, tail=1), _drop(hip, p=0.25, seed=a16)) == hip.EQH_ERR_ARG
    # the prologue site needs the CSR, its permutation and a seed; the LayerNorm site a seed
    full = dict(seed_inc=a16, perm=a16)
    assert call(F3, _args(hip, rows=0, rowptr=a16), _drop(hip, p_inc=0.25, **full)) == hip.EQH_OK
    assert call(F3, _args(hip, rows=0), _drop(hip, p_inc=0.25, **full)) == hip.EQH_ERR_ARG                   # no rowptr
    for missing in full:
        rest = {k: v for k, v in full.items() if k != missing}
        assert call(F3, _args(hip, rows=0, rowptr=a16), _drop(hip, p_inc=0.25, **rest)) == hip.EQH_ERR_ARG, missing
    assert call(F3, _args(hip, rows=0), _drop(hip, p=0.25)) == hip.EQH_ERR_ARG
    assert call(B3, _args(hip, rows=0), _drop(hip, p=0.25)) == hip.EQH_ERR_ARG
    # B3 has no prologue
    assert call(B3, _args(hip, rows=0, rowptr=a16), _drop(hip, p_inc=0.25, p=0.25, seed=a16, **full)) == hip.EQH_ERR_ARG
    # the checks hg_conv_panel makes apply as well: width, products / planes, row range, missing operands
    ok = _drop(hip, p=0.25, seed=a16)
    assert call(F3, _args(hip, rows=0, C=96), ok) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip, rows=0, products=2), ok) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip, rows=0, products=6, planes=2), ok) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip, rows=-1), ok) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip, rows=2 ** 31), ok) == hip.EQH_ERR_RANGE
    assert call(F3, _args(hip, rows=4), ok) == hip.EQH_ERR_ARG and call(B3, _args(hip, rows=4), ok) == hip.EQH_ERR_ARG
    assert call(F3, _args(hip, rows=4, in0=a16 + 4), ok) == hip.EQH_ERR_ALIGN
    # a call with both probabilities 0 is a valid call of the dropout form (it keeps everything)
    assert call(F3, _args(hip, rows=0), _drop(hip)) == hip.EQH_OK


def test_switch_is_forwarded_to_mhnn_panel():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import mhnn_panel

    assert ops.PANEL_DROPOUT is True and mhnn_panel.PANEL_DROPOUT is True
    try:
        ops.PANEL_DROPOUT = False
        assert mhnn_panel.PANEL_DROPOUT is False and ops.PANEL_DROPOUT is False
    finally:
        ops.PANEL_DROPOUT = True
    assert mhnn_panel.PANEL_DROPOUT is True


def test_supported_follows_both_switches_and_the_probability():
    """mhnn_panel_supported on host tensors never says yes (the panels are device kernels); what is checked here is that an
    active dropout is refused through the switches, not through the layer's mode."""
    import torch

    from equihgnn_amd import ops
    from equihgnn_amd.layers import MHNNConv
    from equihgnn_amd.ops import mhnn_panel

    class _OnDevice(torch.Tensor):      # a host tensor that claims to live on the device: only is_cuda is read
        is_cuda = True

    C = 64
    x, e = torch.zeros(3, C).as_subclass(_OnDevice), torch.zeros(2, C).as_subclass(_OnDevice)
    conv = MHNNConv(C, 2, 2, 2, 2, aggr="mean", dropout=0.3, normalization="ln").train()
    assert mhnn_panel.mhnn_panel_supported(x, e, conv)
    assert mhnn_panel.mhnn_panel_supported(x, e, conv.eval())
    conv.train()
    for name in ("PANEL_DROPOUT", "FUSED_DROPOUT"):
        try:
            setattr(ops, name, False)
            assert not mhnn_panel.mhnn_panel_supported(x, e, conv), name
            assert mhnn_panel.mhnn_panel_supported(x, e, conv.eval()), name      # nothing changes without an active dropout
            conv.train()
        finally:
            setattr(ops, name, True)
    full = MHNNConv(C, 2, 2, 2, 2, aggr="mean", dropout=1.0, normalization="ln").train()
    assert not mhnn_panel.mhnn_panel_supported(x, e, full)
    assert mhnn_panel.mhnn_panel_supported(x, e, MHNNConv(C, 2, 2, 2, 2, aggr="mean", dropout=0.0, normalization="ln").train())
