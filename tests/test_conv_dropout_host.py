"""Host-side checks of the conv-tail dropout (no GPU): the *_drop_* entry points of csrc/incidence.hip are declared and
exported, validate their arguments before any launch, the package switch reaches its owner, and the operators handle the
ends of the probability range before they touch a device."""
import ctypes

import pytest
import torch

ENTRY_POINTS = ("hg_bias_relu_ln_drop_fwd", "hg_bias_relu_ln_drop_bwd_workspace_bytes", "hg_bias_relu_ln_drop_bwd",
                "hg_gather_ln_reduce_drop_fwd", "hg_gather_ln_reduce_drop_bwd_workspace_bytes", "hg_gather_ln_reduce_drop_bwd",
                "hg_incidence_ln_reduce_drop_fwd", "hg_incidence_ln_reduce_drop_fwd_col",
                "hg_incidence_ln_reduce_drop_bwd_workspace_bytes", "hg_incidence_ln_reduce_drop_bwd")


def test_header_declares_and_library_exports_the_dropout_entry_points():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in hip.SIGNATURES, f"{name} is not declared in include/equihgnn_hip.h"
        assert hasattr(handle, name), f"{name} declared in the header but not exported"
    # every launching entry takes `float p, const int64_t* seed` side by side, as the faf_* entries do
    for name in ENTRY_POINTS:
        if name.endswith("_workspace_bytes"):
            assert hip.SIGNATURES[name] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32])
            continue
        res, args = hip.SIGNATURES[name]
        assert res is ctypes.c_int32
        at = [i for i in range(1, len(args) - 1) if args[i] is ctypes.c_float and args[i - 1] is ctypes.c_float
              and args[i + 1] is ctypes.c_void_p]
        assert len(at) == 1, name          # (eps, p, seed): the only place two floats meet a pointer


def test_dropout_entry_points_validate_before_launching():
    from equihgnn_amd import hip

    L = hip.lib()
    held = ctypes.create_string_buffer(64)
    a = ctypes.addressof(held)               # 16-byte alignment is not guaranteed: only used where a null is refused first
    assert L.hg_bias_relu_ln_drop_bwd_workspace_bytes(1000, 256) == L.hg_bias_relu_ln_bwd_workspace_bytes(1000, 256)
    assert L.hg_gather_ln_reduce_drop_bwd_workspace_bytes(1000, 256) == L.hg_gather_ln_reduce_bwd_workspace_bytes(1000, 256)
    # the per-incidence backward carries a d beta slab next to d gamma's
    assert L.hg_incidence_ln_reduce_drop_bwd_workspace_bytes(1000, 256) == 2 * L.hg_incidence_ln_reduce_bwd_workspace_bytes(1000, 256)
    assert L.hg_incidence_ln_reduce_drop_bwd_workspace_bytes(-1, 256) == 0
    fwd = lambda p, R=4, C=64: L.hg_bias_relu_ln_drop_fwd(None, 1.0, None, None, None, None, R, C, 1e-5, p, None, None, None)
    assert fwd(0.25, R=0) == hip.EQH_OK                        # nothing to do
    assert fwd(0.25) == hip.EQH_ERR_ARG                        # null pointers
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert fwd(p, R=0) == hip.EQH_ERR_ARG, p               # 0 <= p < 1, checked first
    assert fwd(0.25, R=0, C=66) == hip.EQH_ERR_ALIGN and fwd(0.25, R=0, C=1028) == hip.EQH_ERR_ALIGN
    assert fwd(0.25, R=2 ** 31) == hip.EQH_ERR_RANGE
    g = lambda p, R=4: L.hg_gather_ln_reduce_drop_fwd(None, None, None, None, None, None, R, 64, 1, 1e-5, p, None, None, None)
    assert g(0.5, 0) == hip.EQH_OK and g(0.5) == hip.EQH_ERR_ARG and g(1.0, 0) == hip.EQH_ERR_ARG
    i = lambda p, R=4: L.hg_incidence_ln_reduce_drop_fwd_col(None, None, None, None, None, 1, None, None, R, 64, 1, 1e-5, p, None,
                                                             None, None)
    assert i(0.5, 0) == hip.EQH_OK and i(0.5) == hip.EQH_ERR_ARG and i(-1.0, 0) == hip.EQH_ERR_ARG
    # backward without rows: the parameter gradients must still be named
    assert L.hg_incidence_ln_reduce_drop_bwd(None, None, None, None, None, None, 0, None, None, 0, None, None, None, a, 64, 1,
                                             1e-5, 0.5, None, None, None, None, None, 1, None, 0, None) == hip.EQH_ERR_ARG


def test_switch_is_forwarded_to_rows():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import rows

    assert ops.FUSED_DROPOUT is True and rows.FUSED_DROPOUT is True
    try:
        ops.FUSED_DROPOUT = False
        assert rows.FUSED_DROPOUT is False and ops.FUSED_DROPOUT is False
    finally:
        ops.FUSED_DROPOUT = True
    assert rows.FUSED_DROPOUT is True


def test_operators_reject_negative_p_and_route_p_of_one_to_zeros():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import CSR

    C = 8
    h = torch.randn(5, C, requires_grad=True)
    b, g, be = torch.zeros(C), torch.ones(C), torch.zeros(C, requires_grad=True)
    csr = CSR(rowptr=torch.zeros(4, dtype=torch.int32), perm=torch.zeros(1, dtype=torch.int32),
              col=torch.zeros(1, dtype=torch.int32), n_rows=3, nnz=0)
    i32 = torch.zeros(0, dtype=torch.int32)
    calls = {
        "bias_relu_ln": lambda p: ops.bias_relu_ln(h, b, g, be, p=p),
        "linear_add_relu_ln": lambda p: ops.linear_add_relu_ln(h, torch.randn(C, C), h, 0.5, b, g, be, p=p),
        "gather_ln_reduce": lambda p: ops.gather_ln_reduce(h, b, g, be, csr, csr, "mean", p=p),
        "incidence_ln_reduce": lambda p: ops.incidence_ln_reduce(h, h, g, be, i32, i32, csr, csr, csr, i32, "mean", p=p),
    }
    rows = {"bias_relu_ln": 5, "linear_add_relu_ln": 5, "gather_ln_reduce": 3, "incidence_ln_reduce": 3}
    for name, call in calls.items():
        for p in (-0.1, float("nan")):
            with pytest.raises(ValueError, match="between 0 and 1"):
                call(p)
        for p in (1.0, 1.5):                    # nn.Dropout(p = 1): zeros, and zero gradients
            out = call(p)
            assert out.shape == (rows[name], C) and float(out.detach().abs().max()) == 0.0, name
    out = calls["bias_relu_ln"](1.0)
    out.sum().backward()
    assert float(h.grad.abs().max()) == 0.0 and float(be.grad.abs().max()) == 0.0


def test_panel_and_stack_paths_keep_refusing_an_active_dropout():
    from common import golden_args

    from equihgnn_amd import models

    m = models.MODELS["mhnns"](1, golden_args("mhnns", 64, dropout=0.3))
    x = torch.zeros(4, 64)
    m.train()
    assert m.conv.W1.drop_p == 0.3 and m._drop_p == 0.3
    assert not m.conv.stack_supported(x, {"any": 0})
    m.eval()
    assert m.conv.W1.drop_p == 0.0 and m._drop_p == 0.0
