"""Host-side checks of the fused read-out head's dropout form (no GPU): hg_readout_mse_drop_f32 is declared and exported and
validates its arguments before any launch, the package switch reaches its owner, the operator answers the `supported`
questions without a device -- and a numpy twin of csrc/drop_hash.h (drop_key, drop_hash, the threshold and the scale), which
tests/test_hip_readout_dropout.py checks against the device and uses to pick its cases on the host."""
import ctypes

import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1
M32 = np.uint64(0xFFFFFFFF)


def drop_key(seed: int):
    """(x, m, a) of csrc/drop_hash.h: index offset, odd multiplier, addend of the high index word"""
    def mix(z):                                            # splitmix64
        z = (z + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    z = mix(int(seed) & M64)
    y = mix(z)
    return z & 0xFFFFFFFF, (z >> 32) | 1, (y & 0xFFFFFFFF) | 1


def drop_hash(key, pair):
    """the 32-bit avalanche of the element PAIR index (numpy uint64 array) under ``key``"""
    x, m, a = (np.uint64(k) for k in key)
    pair = np.asarray(pair, dtype=np.uint64)
    h = (((pair & M32) ^ x) + (pair >> np.uint64(32)) * a) & M32
    h ^= h >> np.uint64(16)
    h = (h * m) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def drop_threshold16(p: float) -> int:
    """the high 16 bits of drop_threshold(p): the probability is a float in the C ABI"""
    if not p > 0:
        return 0
    return min(max(int(float(np.float32(p)) * 65536.0 + 0.5), 1), 65535)


def drop_inv_keep(p: float) -> np.float32:
    p32 = np.float32(p)
    if not p32 > 0:
        return np.float32(1.0)
    if p32 >= 1:
        return np.float32(0.0)
    return np.float32(65536.0) if float(p32) * 65536.0 + 0.5 >= 65536.0 else np.float32(1.0) / (np.float32(1.0) - p32)


def keep_matrix(rows: int, cols: int, p: float, seed: int, first: int = 0) -> np.ndarray:
    """[rows, cols] float32: 0 or 1 / (1 - p), the decisions of the flat elements first .. first + rows * cols - 1"""
    i = np.uint64(first) + np.arange(rows * cols, dtype=np.uint64)
    h = drop_hash(drop_key(seed), i >> np.uint64(1))
    half = np.where((i & np.uint64(1)).astype(bool), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return np.where(half >= np.uint64(drop_threshold16(p)), drop_inv_keep(p), np.float32(0.0)).astype(np.float32).reshape(rows, cols)


def test_header_declares_and_library_exports_the_entry_point():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    name = "hg_readout_mse_drop_f32"
    assert name in hip.SIGNATURES, f"{name} is not declared in include/equihgnn_hip.h"
    assert hasattr(handle, name), f"{name} declared in the header but not exported"
    res, args = hip.SIGNATURES[name]
    _, base = hip.SIGNATURES["hg_readout_mse_f32"]
    # the arguments of hg_readout_mse_f32, then p_x, p_h and the three seeds in front of the stream
    assert res is ctypes.c_int32 and args == base[:-1] + [ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 3 + base[-1:]


def test_entry_point_validates_before_launching():
    from equihgnn_amd import hip

    L = hip.lib()
    held = (ctypes.c_int64 * 3)(1, 2, 3)
    s = [ctypes.addressof(held) + 8 * i for i in range(3)]

    def call(p_x, p_h, seeds=(None, None, None), n_graphs=0, C=64, H=64):
        return L.hg_readout_mse_drop_f32(None, None, n_graphs, 0, C, H, None, 1e-5, None, None, None, None, None, 0, None, 0, None,
                                         p_x, p_h, *seeds, None)
    for p_h in (-0.1, 1.0, 1.5, float("nan")):
        assert call(0.0, p_h, s) == hip.EQH_ERR_ARG, p_h                 # 0 <= p < 1
    assert call(1.0, 0.1, s) == hip.EQH_ERR_ARG and call(-0.5, 0.1, s) == hip.EQH_ERR_ARG
    assert call(0.3, 0.0, (None, s[1], s[2])) == hip.EQH_ERR_ARG        # an active site without its seed
    assert call(0.0, 0.3, (s[0], None, s[2])) == hip.EQH_ERR_ARG and call(0.0, 0.3, (s[0], s[1], None)) == hip.EQH_ERR_ARG
    assert call(0.0, 0.0, s) == hip.EQH_ERR_ARG                          # no active site: hg_readout_mse_f32's call
    assert call(0.3, 0.1, s) == hip.EQH_OK                               # nothing to do
    assert call(0.3, 0.0, (s[0], None, None)) == hip.EQH_OK and call(0.0, 0.1, (None, s[1], s[2])) == hip.EQH_OK
    assert call(0.3, 0.1, s, n_graphs=4) == hip.EQH_ERR_ARG              # null pointers
    assert call(0.3, 0.1, s, C=96) == hip.EQH_ERR_ARG and call(0.3, 0.1, s, n_graphs=-1) == hip.EQH_ERR_ARG
    # the plain entry is as it was
    assert L.hg_readout_mse_f32(None, None, 0, 0, 64, 64, None, 1e-5, None, None, None, None, None, 0, None, 0, None,
                                None) == hip.EQH_OK


def test_switch_exists_is_on_by_default_and_is_forwarded_to_its_owner():
    from equihgnn_amd import ops
    from equihgnn_amd.ops import readout

    before = ops.READOUT_DROPOUT
    assert before is True and readout.READOUT_DROPOUT is True
    try:
        ops.READOUT_DROPOUT = False
        assert readout.READOUT_DROPOUT is False and ops.READOUT_DROPOUT is False
    finally:
        ops.READOUT_DROPOUT = before
    assert readout.READOUT_DROPOUT is before


def test_supported_answers_without_a_device_and_the_operator_rejects_probabilities_outside_the_range():
    from equihgnn_amd import ops
    from equihgnn_amd.layers import MLP

    mlp = MLP(64, 64, 1, 3, dropout=0.3, Normalization="ln", InputNorm=False).train()
    x = torch.zeros(4, 64)
    assert not ops.readout_mse_supported(x, mlp) and not ops.readout_mse_drop_supported(x, mlp, 0.3)      # host rows
    assert not ops.readout_mse_drop_supported(x, mlp, 1.0) and not ops.readout_mse_drop_supported(x, mlp, -0.1)
    mlp.eval()
    assert not ops.readout_mse_drop_supported(x, mlp, 0.0)              # no active site
    rowptr = torch.tensor([0, 4], dtype=torch.int32)
    mlp.train()
    for p_x in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"in \[0, 1\)"):
            ops.readout_mse(x, rowptr, mlp, torch.zeros(1), p_x=p_x)
    mlp.dropout = 1.0
    with pytest.raises(ValueError, match=r"in \[0, 1\)"):
        ops.readout_mse(x, rowptr, mlp, torch.zeros(1))


def test_numpy_twin_of_the_hash():
    """what can be said without a device: both elements of an aligned pair come from ONE hash, the realised keep rate is that of
    the 16-bit threshold, seeds and sites give different masks, and a window of a larger tensor is that tensor's mask"""
    key = drop_key(12345)
    assert all(0 <= k < 2 ** 32 for k in key) and key[1] & 1 and key[2] & 1 and drop_key(12346) != key
    h = drop_hash(key, np.arange(8, dtype=np.uint64))
    assert h.dtype == np.uint64 and int(h.max()) < 2 ** 32 and len(set(h.tolist())) == 8
    # the high index word enters: pair 2^32 is not pair 0
    assert int(drop_hash(key, np.array([1 << 32], dtype=np.uint64))[0]) != int(h[0])
    assert drop_threshold16(0.0) == 0 and drop_threshold16(1e-9) == 1 and drop_threshold16(0.5) == 32768
    assert drop_threshold16(0.1) == 6554 and float(drop_inv_keep(0.5)) == 2.0 and float(drop_inv_keep(0.0)) == 1.0
    for p in (0.1, 0.3, 0.5):
        k = keep_matrix(512, 256, p, 99)
        assert set(np.unique(k).tolist()) == {0.0, float(drop_inv_keep(p))}
        rate = float((k == 0).mean())
        assert abs(rate - p) < 4 * np.sqrt(p * (1 - p) / k.size) + 2.0 ** -16, (p, rate)
        assert not np.array_equal(k, keep_matrix(512, 256, p, 100))
    whole = keep_matrix(40, 64, 0.3, 7)
    assert np.array_equal(keep_matrix(8, 64, 0.3, 7, first=32 * 64), whole[32:])
    assert np.array_equal(keep_matrix(40, 64, 0.0, 7), np.ones((40, 64), np.float32))
