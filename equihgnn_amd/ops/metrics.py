"""An epoch's loss and bootstrap metrics kept on the device: the running sums of fit.DeviceBootstrapMetrics and of the
trainers' ``loss_readout`` (csrc/metrics.hip), and the host twin of their Poisson(1) weights.

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ._base import _c_void_p, _f32c, _ptr, _require_gpu, _stream

BOOTSTRAP_SLOTS = 64        # row length of a bootstrap accumulator: [3, 64] doubles


def _not_capturing(what: str, device) -> None:
    # the launch carries host-side state by value (the position of the batch's first element; one more step counted): a
    # replay would repeat it.  Capturing these updates needs a device-side counter.
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what}: the current stream is capturing; this update is an ordinary launch behind the replayed "
                           "graph, not a node of it")


def _acc(acc: torch.Tensor, numel: int, what: str) -> torch.Tensor:
    _require_gpu(acc, what)
    if acc.dtype != torch.float64 or acc.numel() != numel or not acc.is_contiguous():
        raise TypeError(f"{what}: the accumulator is {numel} contiguous float64 values on the device")
    return acc


def bootstrap_update(pred: torch.Tensor, target: torch.Tensor, scale: float, copies: int, seed: int, position0: int,
                     acc: torch.Tensor) -> None:
    """One batch into the bootstrap sums ``acc`` ([3, 64] float64: sum w |e|, sum w e^2, sum w per copy), with
    e = pred * scale - target * scale (the products in fp32, the rest in double) and w the Poisson(1) weight of
    (seed, position0 + i, copy).  No read, no allocation; the caller advances ``position0`` by ``pred.numel()``."""
    _require_gpu(pred, "bootstrap_update")
    _require_gpu(target, "bootstrap_update")
    _acc(acc, 3 * BOOTSTRAP_SLOTS, "bootstrap_update")
    if pred.numel() != target.numel():
        raise ValueError(f"bootstrap_update: {pred.numel()} predictions for {target.numel()} targets")
    _not_capturing("bootstrap_update", pred.device)
    p, t = _f32c(pred.detach().reshape(-1)), _f32c(target.detach().reshape(-1))
    hip.check(hip.lib().eqh_bootstrap_update(_ptr(p), _ptr(t), p.numel(), float(scale), int(copies), int(seed),
                                             int(position0), _ptr(acc), _stream(p.device)), "eqh_bootstrap_update")


def loss_accumulate(loss: torch.Tensor, acc: torch.Tensor) -> None:
    """``acc[0] += loss; acc[1] += 1`` in double, on the device (``acc``: 2 float64): one step's loss into the epoch's sum."""
    _require_gpu(loss, "loss_accumulate")
    _acc(acc, 2, "loss_accumulate")
    if loss.numel() != 1:
        raise ValueError(f"loss_accumulate: a scalar loss expected, got {tuple(loss.shape)}")
    _not_capturing("loss_accumulate", loss.device)
    ls = _f32c(loss.detach().reshape(1))
    hip.check(hip.lib().eqh_loss_accumulate(_ptr(ls), _ptr(acc), _stream(ls.device)), "eqh_loss_accumulate")


def bootstrap_weights_host(seed: int, position0: int, n: int, copies: int) -> np.ndarray:
    """The weights ``bootstrap_update`` gives the ``n`` elements from ``position0`` on: int32 [copies, n].  Host only."""
    out = np.empty((int(copies), int(n)), dtype=np.int32)
    hip.check(hip.lib().eqh_bootstrap_weights_host(int(seed), int(position0), int(n), int(copies),
                                                   _c_void_p(out.ctypes.data)), "eqh_bootstrap_weights_host")
    return out
