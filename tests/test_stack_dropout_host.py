"""Host-side checks of the training dropout on the S-tail conv stack's panel kernels (no GPU): hg_conv_stack_drop /
HgConvStackDrop are declared and exported, the entry validates its arguments before any launch, the package switch reaches its
owner, and the predicate that decides the path follows the two switches and the probabilities."""
import ctypes


def test_header_declares_and_library_exports_the_stack_dropout_entry():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in ("hg_conv_stack_drop", "hg_conv_stack_drop_f3_launches"):
        assert name in hip.SIGNATURES, f"{name} is not declared in include/equihgnn_hip.h"
        assert hasattr(handle, name), f"{name} declared in the header but not exported"
    res, args = hip.SIGNATURES["hg_conv_stack_drop"]
    assert res is ctypes.c_int32
    assert args == [ctypes.c_int32, ctypes.POINTER(hip.HgConvPanel), ctypes.POINTER(hip.HgConvStackDrop), ctypes.c_void_p]
    assert [(n, t) for n, t in hip.HgConvStackDrop._fields_] == [
        ("p_inc", ctypes.c_float), ("seed_inc", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("p3", ctypes.c_float),
        ("seed3", ctypes.c_void_p), ("p_x", ctypes.c_float), ("seed_x", ctypes.c_void_p), ("p1", ctypes.c_float),
        ("seed1", ctypes.c_void_p)]
    # the siblings keep their signatures
    assert hip.SIGNATURES["hg_conv_panel"] == (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(hip.HgConvPanel), ctypes.c_void_p])
    assert hip.SIGNATURES["hg_conv_panel_drop"][1] == [ctypes.c_int32, ctypes.POINTER(hip.HgConvPanel), ctypes.POINTER(hip.HgConvDrop),
                                                       ctypes.c_void_p]


def _args(hip, rows=0, C=64, **kw):
    a = hip.HgConvPanel()
    a.rows, a.C = rows, C
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _drop(hip, **kw):
    d = hip.HgConvStackDrop()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_stack_dropout_entry_validates_before_launching():
    from equihgnn_amd import hip

    L = hip.lib()
    held = ctypes.create_string_buffer(256)
    a16 = (ctypes.addressof(held) + 15) & ~15           # a non-null, 16-byte aligned host address: never dereferenced here
    call = lambda stage, a, d: L.hg_conv_stack_drop(stage, a, d, None)
    F1, F3, B3, B1 = hip.HG_CONV_F1, hip.HG_CONV_F3, hip.HG_CONV_B3, hip.HG_CONV_B1
    OK, ERR = hip.EQH_OK, hip.EQH_ERR_ARG
    seeds = dict(seed_inc=a16, perm=a16, seed3=a16, seed_x=a16, seed1=a16)
    # null argument blocks
    assert call(F3, None, _drop(hip)) == ERR
    assert call(F3, _args(hip), None) == ERR
    # the four stages, with and without a tail, at rows = 0: nothing to do
    for stage, tail in ((F1, 0), (F3, 0), (F3, 1), (B1, 0), (B1, 1), (B3, 0)):
        assert call(stage, _args(hip, tail=tail), _drop(hip, p3=0.25, p1=0.25, **seeds)) == OK, (stage, tail)
        assert call(stage, _args(hip, tail=tail), _drop(hip)) == OK, (stage, tail)       # every probability 0: the plain call
    assert call(F3, _args(hip, tail=1, rowptr=a16), _drop(hip, p_inc=0.25, p3=0.25, p_x=0.25, p1=0.25, **seeds)) == OK
    # p_x on B1's tail: a scalar on the mask of the stored Xn (in3) -- no seed, but not without those rows
    b1x = _drop(hip, p3=0.25, p_x=0.25, p1=0.25, seed3=a16, seed1=a16)
    assert call(B1, _args(hip, tail=1, in3=a16), b1x) == OK
    assert call(B1, _args(hip, tail=1), b1x) == ERR
    assert call(B1, _args(hip, tail=0), b1x) == OK                                # without a tail B1 does not read p_x
    # a probability outside 0 <= p < 1 is refused before anything else is looked at -- in every field, on every stage
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        for field in ("p_inc", "p3", "p_x", "p1"):
            for stage in (F1, F3, B1, B3, 99):
                assert call(stage, _args(hip, rowptr=a16), _drop(hip, **{field: bad}, **seeds)) == ERR, (bad, field, stage)
    # a stage outside the four
    for stage in (hip.HG_CONV_F2, hip.HG_EGNN_NODE_F, hip.HG_EGNN_NODE_B, 0, 99):
        assert call(stage, _args(hip), _drop(hip, p1=0.25, **seeds)) == ERR, stage
        assert call(stage, _args(hip), _drop(hip)) == ERR, stage
    # an active site of the stage without its seed
    assert call(F1, _args(hip), _drop(hip, p1=0.25)) == ERR
    assert call(B1, _args(hip), _drop(hip, p1=0.25)) == ERR
    assert call(F3, _args(hip, tail=1), _drop(hip, p1=0.25)) == ERR
    assert call(F3, _args(hip), _drop(hip, p1=0.25)) == OK                        # without a tail F3 does not read the W1 site
    assert call(F3, _args(hip), _drop(hip, p3=0.25)) == ERR
    assert call(B3, _args(hip), _drop(hip, p3=0.25)) == ERR
    assert call(B1, _args(hip, tail=1), _drop(hip, p3=0.25, p1=0.25, seed1=a16)) == ERR
    assert call(B1, _args(hip), _drop(hip, p3=0.25, p1=0.25, seed1=a16)) == OK    # without a tail B1 does not read the W3 site
    assert call(F3, _args(hip), _drop(hip, p_x=0.25)) == ERR
    assert call(F3, _args(hip), _drop(hip, p_x=0.25, seed_x=a16)) == OK
    # the prologue site: F3 only, with the CSR, its permutation and a seed
    full = dict(seed_inc=a16, perm=a16)
    assert call(F3, _args(hip, rowptr=a16), _drop(hip, p_inc=0.25, **full)) == OK
    assert call(F3, _args(hip), _drop(hip, p_inc=0.25, **full)) == ERR                   # no rowptr
    for missing in full:
        rest = {k: v for k, v in full.items() if k != missing}
        assert call(F3, _args(hip, rowptr=a16), _drop(hip, p_inc=0.25, **rest)) == ERR, missing
    for stage in (F1, B1, B3):
        assert call(stage, _args(hip, rowptr=a16), _drop(hip, p_inc=0.25, **seeds)) == ERR, stage
    # the lone B3 stands at the last application, whose Xn is stored unmasked
    assert call(B3, _args(hip), _drop(hip, p3=0.25, p_x=0.25, **seeds)) == ERR
    # the checks hg_conv_panel makes apply as well: width, products / planes, row range, missing operands, alignment
    ok = _drop(hip, p3=0.25, p1=0.25, **seeds)
    assert call(F3, _args(hip, C=96), ok) == ERR
    assert call(F1, _args(hip, products=2), ok) == ERR
    assert call(B1, _args(hip, products=6, planes=2), ok) == ERR
    assert call(F3, _args(hip, rows=-1), ok) == ERR
    assert call(F3, _args(hip, rows=2 ** 31), ok) == hip.EQH_ERR_RANGE
    for stage in (F1, F3, B1, B3):
        assert call(stage, _args(hip, rows=4), ok) == ERR, stage
    assert call(F1, _args(hip, rows=4, in0=a16 + 4), ok) == hip.EQH_ERR_ALIGN


def test_f3_launch_count_is_one_or_two_at_every_panel_shape():
    from equihgnn_amd import hip

    L = hip.lib()
    for C in (64, 128, 256):
        for products in (0, 6, 3, 1):
            assert L.hg_conv_stack_drop_f3_launches(C, products) in (1, 2), (C, products)
    assert L.hg_conv_stack_drop_f3_launches(96, 6) == 0 and L.hg_conv_stack_drop_f3_launches(64, 2) == 0


def test_switch_is_forwarded_to_conv_stack():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import conv_stack

    before = ops.STACK_DROPOUT
    assert isinstance(before, bool) and conv_stack.STACK_DROPOUT is before
    try:
        for value in (False, True):
            ops.STACK_DROPOUT = value
            assert conv_stack.STACK_DROPOUT is value and ops.STACK_DROPOUT is value
    finally:
        ops.STACK_DROPOUT = before
    assert conv_stack.STACK_DROPOUT is before


def test_predicate_follows_both_switches_and_the_probabilities():
    from common import golden_args

    from equihgnn_amd import models, ops

    before = ops.STACK_DROPOUT
    try:
        ops.STACK_DROPOUT = True
        assert ops.stack_dropout_supported((0.3, 0.3, 0.3, 0.3)) and ops.stack_dropout_supported((0.0, 0.0, 0.0, 0.0))
        assert ops.stack_dropout_supported((0.999,))
        for bad in (1.0, 1.5, -0.1, float("nan")):
            assert not ops.stack_dropout_supported((0.3, bad, 0.3, 0.3)), bad
        for name in ("STACK_DROPOUT", "FUSED_DROPOUT"):
            try:
                setattr(ops, name, False)
                assert not ops.stack_dropout_supported((0.3, 0.3, 0.3, 0.3)), name
            finally:
                setattr(ops, name, True)
        assert ops.stack_dropout_supported((0.3, 0.3, 0.3, 0.3))
        # the dropout forms belong to the folded launch list: with a diagnostic un-folding the row kernels keep the dropout
        from equihgnn_amd.ops import conv_stack
        for name in ("FOLD_INC", "FOLD_B2"):
            assert getattr(conv_stack, name) is True       # (the defaults: the process sets neither EQH_NO_* variable)
            try:
                setattr(conv_stack, name, False)
                assert not ops.stack_dropout_supported((0.3, 0.3, 0.3, 0.3)), name
            finally:
                setattr(conv_stack, name, True)
        assert ops.stack_dropout_supported((0.3, 0.3, 0.3, 0.3))

        # the layer: an active dropout is refused through the predicate, not through the layer's mode
        import torch

        class _OnDevice(torch.Tensor):      # a host tensor that claims to live on the device: only is_cuda is read
            is_cuda = True

        m = models.MODELS["mhnns"](1, golden_args("mhnns", 64, dropout=0.3)).train()
        x = torch.zeros(4, 64).as_subclass(_OnDevice)
        res = {"any": 0}
        assert m.conv.stack_supported(x, res, 0.3) and m.conv.stack_supported(x, res)
        assert not m.conv.stack_supported(x, res, 1.0)
        assert not m.conv.stack_supported(torch.zeros(4, 64), res, 0.3)      # a host tensor: conv_stack_supported says no
        for name in ("STACK_DROPOUT", "FUSED_DROPOUT"):
            try:
                setattr(ops, name, False)
                assert not m.conv.stack_supported(x, res, 0.3), name
                assert m.conv.eval().stack_supported(x, res), name       # nothing changes without an active dropout
                m.conv.train()
            finally:
                setattr(ops, name, True)
        full = models.MODELS["mhnns"](1, golden_args("mhnns", 64, dropout=1.0)).train()
        assert not full.conv.stack_supported(x, res, 1.0)
        none = models.MODELS["mhnns"](1, golden_args("mhnns", 64, dropout=0.0)).train()
        assert none.conv.stack_supported(x, res)
    finally:
        ops.STACK_DROPOUT = before
