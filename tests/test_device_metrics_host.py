"""Device-resident epoch metrics, host side (no GPU): the Poisson(1) sampler that the bootstrap kernel and its host twin
share (distribution, independence of the copies, purity in (seed, position, copy), the quantised CDF), the argument checks
of the native entry points (which return before anything is launched), and ``Fitter``'s ``device_metrics`` switch on a CPU
model (off: today's rows; on: refused)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from equihgnn_amd import hip, ops

SEEDS = (0, 3, 2024)
THRESHOLDS = [1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
              4294966817, 4294967252, 4294967292, 4294967295]


@pytest.mark.parametrize("seed", SEEDS)
def test_weights_are_poisson_one_and_the_copies_are_uncorrelated(seed):
    n, copies = 4096, 50
    w = ops.bootstrap_weights_host(seed, 0, n, copies)
    assert w.shape == (copies, n) and w.dtype == np.int32
    m = w.size
    assert m == 204800
    p = [math.exp(-1.0) / math.factorial(k) for k in range(6)]
    p.append(1.0 - sum(p))
    counts = [int((w == k).sum()) for k in range(6)] + [int((w >= 6).sum())]
    for k, (c, pk) in enumerate(zip(counts, p)):
        sigmas = abs(c - m * pk) / math.sqrt(m * pk * (1.0 - pk))
        print(f"seed {seed}: value {k}{'+' if k == 6 else ''}: {c} draws, {sigmas:.2f} sigma from {m * pk:.1f}")
        assert sigmas <= 5.0, (k, c, m * pk)
    corr = np.corrcoef(w.astype(np.float64))
    np.fill_diagonal(corr, 0.0)
    print(f"seed {seed}: max |correlation| of two copies {np.abs(corr).max() * math.sqrt(n):.2f} / sqrt(n)")
    assert np.abs(corr).max() <= 5.0 / math.sqrt(n)
    assert 0 <= w.min() and w.max() <= 13


def test_weights_are_a_pure_function_of_seed_position_and_copy():
    seed, p0, n, copies = 5, 1000, 257, 50
    w = ops.bootstrap_weights_host(seed, p0, n, copies)
    assert np.array_equal(w, ops.bootstrap_weights_host(seed, p0, n, copies))
    for cut in (0, 1, 63, 64, 128, 256, 257):        # one call equals two calls split anywhere
        a = ops.bootstrap_weights_host(seed, p0, cut, copies)
        b = ops.bootstrap_weights_host(seed, p0 + cut, n - cut, copies)
        assert np.array_equal(np.concatenate((a, b), axis=1), w), cut
    # fewer copies: the same rows (a copy's stream does not depend on how many copies are drawn)
    assert np.array_equal(ops.bootstrap_weights_host(seed, p0, n, 7), w[:7])
    # another seed, another copy: another stream
    assert not np.array_equal(ops.bootstrap_weights_host(seed + 1, p0, n, copies), w)
    for c in range(1, copies):
        assert not np.array_equal(w[c], w[0]), c
    # a copy's stream is not a neighbour copy's stream moved by one position (position * 64 + copy is one index)
    assert not np.array_equal(w[1, :-1], w[0, 1:])


def test_window_where_the_stream_index_crosses_two_to_the_32():
    p0, n, copies = 2 ** 26 - 2, 5, 64
    w = ops.bootstrap_weights_host(9, p0, n, copies)
    one_by_one = np.concatenate([ops.bootstrap_weights_host(9, p0 + i, 1, copies) for i in range(n)], axis=1)
    assert np.array_equal(w, one_by_one)
    # a 32-bit index would give position 2^26 + j the draws of position j
    low = ops.bootstrap_weights_host(9, 0, 3, copies)
    assert not np.array_equal(w[:, 2:], low)


def test_thresholds_are_the_quantised_poisson_cdf():
    cdf, got = 0.0, []
    for k in range(13):
        cdf += math.exp(-1.0) / math.factorial(k)
        got.append(math.floor(2.0 ** 32 * cdf))
    assert got == THRESHOLDS
    # ... and they are the constants the sampler carries
    with open(hip.HEADER.replace("include/equihgnn_hip.h", "equihgnn_amd/csrc/poisson_hash.h")) as f:
        text = f.read()
    body = text.split("#define POISSON1_THRESHOLDS", 1)[1].split("}", 1)[0]
    assert [int(v.strip(" {\\\n").rstrip("u")) for v in body.split(",")] == THRESHOLDS


def test_native_entry_points_check_their_arguments_before_any_launch():
    L = hip.lib()
    for name in ("eqh_bootstrap_update", "eqh_loss_accumulate", "eqh_bootstrap_weights_host"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    held = ctypes.create_string_buffer(256)          # addresses that are never read: no call below gets as far as a launch
    ok = (ctypes.addressof(held) + 15) // 16 * 16

    def update(pred=ok, target=ok, n=4, copies=50, position0=0, acc=ok):
        return L.eqh_bootstrap_update(pred, target, n, 1.0, copies, 0, position0, acc, None)
    assert update(pred=None) == hip.EQH_ERR_ARG
    assert update(target=None) == hip.EQH_ERR_ARG
    assert update(acc=None) == hip.EQH_ERR_ARG
    assert update(n=-1) == hip.EQH_ERR_ARG
    for bad in (0, -1, 65):
        assert update(copies=bad) == hip.EQH_ERR_ARG, bad
    assert update(position0=-1) == hip.EQH_ERR_ARG
    assert update(acc=ok + 4) == hip.EQH_ERR_ALIGN
    assert update(n=0) == hip.EQH_OK                       # nothing to add, nothing launched
    assert update(n=0, acc=None) == hip.EQH_ERR_ARG        # (checked ahead of the empty-batch return)
    assert update(n=0, copies=65) == hip.EQH_ERR_ARG
    assert L.eqh_loss_accumulate(None, ok, None) == hip.EQH_ERR_ARG
    assert L.eqh_loss_accumulate(ok, None, None) == hip.EQH_ERR_ARG
    assert L.eqh_loss_accumulate(ok, ok + 4, None) == hip.EQH_ERR_ALIGN
    out = (ctypes.c_int32 * 8)()
    assert L.eqh_bootstrap_weights_host(0, 0, 4, 2, None) == hip.EQH_ERR_ARG
    assert L.eqh_bootstrap_weights_host(0, 0, -1, 2, out) == hip.EQH_ERR_ARG
    assert L.eqh_bootstrap_weights_host(0, -1, 4, 2, out) == hip.EQH_ERR_ARG
    assert L.eqh_bootstrap_weights_host(0, 0, 4, 0, out) == hip.EQH_ERR_ARG
    assert L.eqh_bootstrap_weights_host(0, 0, 4, 65, out) == hip.EQH_ERR_ARG
    assert L.eqh_bootstrap_weights_host(0, 0, 4, 2, out) == hip.EQH_OK


class _Net(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 1, bias=False)

    def forward(self, data):
        return self.b(torch.tanh(self.a(data.x))).squeeze(-1)


def _data(seed, n=9):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(x=torch.randn(n, 5, generator=g), y=3.0 * torch.randn(n, generator=g))


def test_fitter_option_off_is_todays_fit_and_on_needs_a_gpu_model():
    from equihgnn_amd.fit import DeviceBootstrapMetrics, Fitter
    train, valid = [_data(60 + t) for t in range(4)], [_data(70), _data(71)]
    plain = Fitter(_Net(4), lr=1e-2, std=2.5)
    off = Fitter(_Net(4), lr=1e-2, std=2.5, device_metrics=False)
    a, b = plain.fit(train, valid, epochs=2), off.fit(train, valid, epochs=2)
    assert a.history == b.history and len(a.history) == 2
    ta, tb = plain.test(valid), off.test(valid)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1])
    assert off.host_reads == 0 and off.step.loss_sum is None          # a CPU fit reads nothing from a device
    with pytest.raises(ValueError, match="device_metrics"):
        Fitter(_Net(4), lr=1e-2, device_metrics=True)
    # the device class refuses host tensors; the host class stays the CPU path
    m = DeviceBootstrapMetrics(50, 0)
    with pytest.raises(ValueError, match="GPU"):
        m.update(torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError):
        DeviceBootstrapMetrics(65)
