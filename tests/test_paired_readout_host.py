"""Host-side checks of the paired tail's one-launch read-out head (csrc/readout_pair.hip; no GPU): the four entries are declared
and exported, their derived signatures are hg_readout_mse_*'s with the added arguments, they validate before any launch, the
`supported` questions are answered without a device, the switch reaches its owner, and a paired model on the CPU never asks
for the launch."""
import ctypes

import pytest
import torch

ENTRIES = ("hg_readout_pair_mse_supported", "hg_readout_pair_mse_workspace_bytes", "hg_readout_pair_mse_f32",
           "hg_readout_pair_mse_drop_f32")
VP, I32 = ctypes.c_void_p, ctypes.c_int32


def test_header_declares_and_library_exports_the_four_entries():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name in hip.SIGNATURES, f"{name} is not declared in include/equihgnn_hip.h"
        assert hasattr(handle, name), f"{name} declared in the header but not exported"


def test_signatures_are_the_unpaired_ones_with_the_added_arguments():
    from equihgnn_amd import hip

    sig = hip.SIGNATURES
    assert sig["hg_readout_pair_mse_supported"] == sig["hg_readout_mse_supported"]
    assert sig["hg_readout_pair_mse_workspace_bytes"] == sig["hg_readout_mse_workspace_bytes"]
    res, args = sig["hg_readout_pair_mse_f32"]
    _, base = sig["hg_readout_mse_f32"]
    # (x, rowptr) then (e, e_rowptr, e_perm, e_order, n_e); ... dx then de; the rest as it was
    at_dx = 11
    assert base[at_dx] is VP and base[at_dx + 1] is VP          # dx, dweights
    expect = base[:2] + [VP, VP, VP, VP, I32] + base[2:at_dx + 1] + [VP] + base[at_dx + 1:]
    assert res is I32 and args == expect
    res_d, args_d = sig["hg_readout_pair_mse_drop_f32"]
    # ... then p_x, p_h and FOUR seeds (x, e, hidden 1, hidden 2) in front of the stream
    assert res_d is I32 and args_d == expect[:-1] + [ctypes.c_float, ctypes.c_float] + [VP] * 4 + expect[-1:]
    assert len(args_d) == len(sig["hg_readout_mse_drop_f32"][1]) + 7


def test_supported_is_true_for_exactly_the_six_shapes():
    from equihgnn_amd import hip

    L = hip.lib()
    ok = {(C, H) for C in (16, 32, 64, 96, 128, 192, 256, 512) for H in (32, 64, 96, 128, 192, 256, 512)
          if L.hg_readout_pair_mse_supported(C, H)}
    assert ok == {(C, H) for C in (64, 128, 256) for H in (128, 256)}
    for C, H in ok:
        floats = L.hg_readout_pair_mse_workspace_bytes(17, C, H) // 4
        assert floats >= 2 * (H * 2 * C + H * H + 6 * H + H + 4 + 1)          # two workgroups' slabs
    assert L.hg_readout_pair_mse_workspace_bytes(17, 64, 64) == 0 and L.hg_readout_pair_mse_workspace_bytes(0, 64, 128) == 0


def test_entries_validate_before_launching():
    from equihgnn_amd import hip

    L = hip.lib()
    held = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    s = [ctypes.addressof(held) + 8 * i for i in range(4)]
    none4 = (None, None, None, None)

    def plain(n_graphs=0, n_real=0, C=64, H=128, n_e=0):
        return L.hg_readout_pair_mse_f32(None, None, None, None, None, None, n_e, n_graphs, n_real, C, H, None, 1e-5, None, None,
                                         None, None, None, None, 0, None, 0, None, None)

    def drop(p_x, p_h, seeds=none4, n_graphs=0, n_real=0, C=64, H=128, n_e=0):
        return L.hg_readout_pair_mse_drop_f32(None, None, None, None, None, None, n_e, n_graphs, n_real, C, H, None, 1e-5, None,
                                              None, None, None, None, None, 0, None, 0, None, p_x, p_h, *seeds, None)

    assert plain() == hip.EQH_OK                                         # n_graphs = 0: nothing to do
    assert plain(n_graphs=4) == hip.EQH_ERR_ARG                          # null pointers
    assert plain(n_graphs=4, n_real=5) == hip.EQH_ERR_ARG                # n_real > n_graphs
    assert plain(n_real=1) == hip.EQH_ERR_ARG and plain(n_graphs=-1) == hip.EQH_ERR_ARG and plain(n_e=-1) == hip.EQH_ERR_ARG
    for C, H in ((64, 64), (96, 128), (512, 256), (128, 512)):
        assert plain(C=C, H=H) == hip.EQH_ERR_ARG, (C, H)                # unsupported (C, H)
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert drop(0.0, p, s) == hip.EQH_ERR_ARG and drop(p, 0.1, s) == hip.EQH_ERR_ARG, p      # 0 <= p < 1
    assert drop(0.3, 0.0, (None, s[1], None, None)) == hip.EQH_ERR_ARG   # an active site without its seed
    assert drop(0.3, 0.0, (s[0], None, None, None)) == hip.EQH_ERR_ARG
    assert drop(0.0, 0.3, (None, None, None, s[3])) == hip.EQH_ERR_ARG and drop(0.0, 0.3, (None, None, s[2], None)) == hip.EQH_ERR_ARG
    assert drop(0.0, 0.0, s) == hip.EQH_ERR_ARG                          # no active site: the plain entry's call
    assert drop(0.3, 0.1, s) == hip.EQH_OK                               # n_graphs = 0
    assert drop(0.3, 0.0, (s[0], s[1], None, None)) == hip.EQH_OK and drop(0.0, 0.1, (None, None, s[2], s[3])) == hip.EQH_OK
    assert drop(0.3, 0.1, s, n_graphs=4) == hip.EQH_ERR_ARG              # null pointers
    assert drop(0.3, 0.1, s, n_graphs=4, n_real=5) == hip.EQH_ERR_ARG and drop(0.3, 0.1, s, C=64, H=64) == hip.EQH_ERR_ARG
    # hyperedge rows without their pointers: x, rowptr, weights and y present, e missing
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    w = (ctypes.c_void_p * 10)(*[a] * 10)
    rc = L.hg_readout_pair_mse_f32(a, a, None, None, None, None, 3, 1, 1, 64, 128, w, 1e-5, None, a, None, None, None, None, 0, None,
                                   0, None, None)
    assert rc == hip.EQH_ERR_ARG
    rc = L.hg_readout_pair_mse_f32(a + 4, a, None, None, None, None, 0, 1, 1, 64, 128, w, 1e-5, None, a, None, None, None, None, 0,
                                   None, 0, None, None)
    assert rc == hip.EQH_ERR_ALIGN


def test_switch_is_forwarded_to_its_owner():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import readout

    before = ops.PAIRED_READOUT
    assert isinstance(before, bool) and readout.PAIRED_READOUT is before
    try:
        ops.PAIRED_READOUT = not before
        assert readout.PAIRED_READOUT is (not before) and ops.PAIRED_READOUT is (not before)
    finally:
        ops.PAIRED_READOUT = before
    assert readout.PAIRED_READOUT is before


def test_supported_predicates_answer_without_a_device():
    from equihgnn_amd import ops
    from equihgnn_amd.layers import MLP
    from equihgnn_amd.ops import readout

    x, e = torch.zeros(4, 64), torch.zeros(3, 64)
    good = MLP(128, 128, 1, 3, dropout=0.3, Normalization="ln", InputNorm=False)
    bad = (MLP(128, 128, 1, 2, dropout=0.3, Normalization="ln", InputNorm=False),   # a 2-Linear head
           MLP(128, 128, 1, 3, dropout=0.3, Normalization="bn", InputNorm=False),   # a BatchNorm head
           MLP(64, 128, 1, 3, dropout=0.3, Normalization="ln", InputNorm=False),    # first Linear on C, not 2C, inputs
           MLP(128, 64, 1, 3, dropout=0.3, Normalization="ln", InputNorm=False),    # a hidden width the kernel is not built for
           MLP(128, 128, 1, 3, dropout=0.3, Normalization="ln", InputNorm=True))
    # the head's side of the question needs no device: it is what separates `good` from the others
    assert readout._pair_mlp_ok(good, 64) and not readout._pair_mlp_ok(good, 128)
    for mlp in bad:
        assert not readout._pair_mlp_ok(mlp, 64)
    for mlp in (good, *bad):                                                        # CPU rows: never
        for mode in (mlp.train(), mlp.eval()):
            assert not ops.readout_pair_mse_supported(x, e, mode)
            assert not ops.readout_pair_mse_drop_supported(x, e, mode, 0.3)
    assert not ops.readout_pair_mse_drop_supported(x, e, good.train(), 1.0)
    assert not ops.readout_pair_mse_drop_supported(x, e, good.train(), -0.1)
    with pytest.raises(ValueError, match="one width"):
        ops.readout_pair_mse(x, torch.zeros(3, 32), None, None, None, good, torch.zeros(1))


@pytest.mark.parametrize("method", ["mhnn", "egnn_equihnn"])
def test_paired_models_on_the_cpu_never_call_the_entry(method, monkeypatch):
    """the tail's question is answered "no" for host rows with everything else in order, and a forward pass on the CPU (it stops
    at the index build: the package has no CPU path) has not reached either entry"""
    from common import fill_state_dict, golden_args, make_batch
    from equihgnn_amd import hip, models, ops

    lib, calls = hip.lib(), {"hg_readout_pair_mse_f32": 0, "hg_readout_pair_mse_drop_f32": 0}
    for n in calls:
        def counted(*a, _n=n, _inner=getattr(lib, n)):
            calls[_n] += 1
            return _inner(*a)
        monkeypatch.setattr(lib, n, counted, raising=True)
    monkeypatch.setattr(ops, "PAIRED_READOUT", True)
    m = models.MODELS[method](1, golden_args(method, 64, dropout=0.0, All_num_layers=2, output_hidden=64)).train()
    fill_state_dict(m, 13)
    data = make_batch(11, 3)
    head = (data.y.view(-1), None)
    assert isinstance(m, models._PairedBase) and m.mlp_out.lins[0].in_features == 128
    assert m._one_launch_head(torch.zeros(5, 64), torch.zeros(4, 64), None, head) is False
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        m(data, head=head)
    assert calls == {"hg_readout_pair_mse_f32": 0, "hg_readout_pair_mse_drop_f32": 0}
