"""Readout heads (pool + output MLP + loss in one launch: the S / M tails' and the paired tail's), the paired node /
high-order-hyperedge pool and the fused losses: the MSE, and the L1 / smooth-L1 / Huber family (``loss_spec``).

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import ctypes
import math
import os

import torch
import torch.nn.functional as F

from .. import hip
from . import rows as _rows
from ._base import (ACC_PARAMS, LINEAR_PARAMS, _acc_target, _f32c, _hand_out, _ptr, _require_gpu, _stream, _workspace, timed)
from .frames import _dropout_seed

# An active training dropout stays on the fused read-out head (the DROP form of csrc/readout.hip: the dropout in front of the
# pool and the head's two hidden-layer dropouts inside the one launch).  False -- or ops.FUSED_DROPOUT False, or a probability
# >= 1: the head runs as separate launches (dropout_add, pool, three Linears, two bias_relu_ln, mse_loss), as it did before.
READOUT_DROPOUT = not os.environ.get("EQH_NO_READOUT_DROPOUT")

# The paired tail's head (models._PairedBase: [node pool | pool of the hyperedges of order > 2] -> MLP(2C -> H -> H -> 1) -> MSE)
# as ONE launch, csrc/readout_pair.hip, its dropout sites included.  False: the separate launches (the last application's two
# dropout_add passes, the pool, three Linears, two bias_relu_ln, mse_loss), as before.  On by default (DESIGN.md section 4.8:
# 0.18 ms of the mhnn / egnn_equihnn step); EQH_NO_PAIRED_READOUT switches it off, EQH_PAIRED_READOUT=0 does the same.
PAIRED_READOUT = not os.environ.get("EQH_NO_PAIRED_READOUT") and os.environ.get("EQH_PAIRED_READOUT", "1") != "0"


class _MseLoss(torch.autograd.Function):
    """F.mse_loss(pred, target) (mean) with forward value and gradient from ONE launch (eqh_mse_fwd_bwd)
    instead of six tiny elementwise / reduction launches."""

    @staticmethod
    def forward(ctx, pred, target):
        _require_gpu(pred, "mse_loss")
        pred, target = _f32c(pred), _f32c(target)
        n = pred.numel()
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        hip.check(hip.lib().eqh_mse_fwd_bwd(_ptr(pred), _ptr(target), n, _ptr(loss), _ptr(grad), _stream(pred.device)),
                  "eqh_mse_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return grad * dloss, None


def mse_loss(pred, target):
    """mean((pred - target)^2) for 1-D fp32 device tensors of up to 65 536 values (a batch of molecules)."""
    if pred.is_cuda and pred.dtype == torch.float32 and 0 < pred.numel() <= 65536 and not target.requires_grad:
        return _MseLoss.apply(pred.reshape(-1), target.reshape(-1))
    return F.mse_loss(pred, target)


LOSS_KINDS = ("mse", "l1", "smooth_l1", "huber")


def loss_spec(kind: str, beta: float = 1.0):
    """The training loss ``kind`` as the heads and ``regression_loss`` take it: None for "mse", else (beta, scale) of the family
    term(d) = scale * (|d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta) (csrc/loss_family.h):
    "l1" -> (0, 1), ``beta`` ignored; "smooth_l1" -> (beta, 1), F.smooth_l1_loss(beta=beta), beta >= 0;
    "huber" -> (delta, delta) with delta = ``beta`` > 0, F.huber_loss(delta=delta).  ValueError for anything else."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"loss_spec: unknown loss {kind!r}, expected one of {LOSS_KINDS}")
    if kind == "mse":
        return None
    if kind == "l1":
        return (0.0, 1.0)
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"loss_spec: beta must be a number, got {beta!r}") from None
    if not math.isfinite(b) or b < 0.0:
        raise ValueError(f"loss_spec: beta must be finite and >= 0, got {beta!r}")
    if kind == "huber":
        if b <= 0.0:
            raise ValueError(f"loss_spec: huber needs delta > 0, got {beta!r}")
        return (b, b)
    return (b, 1.0)


def _checked_spec(spec, who: str):
    """A spec handed to an operator directly: None, or two finite floats with beta >= 0 and scale > 0."""
    if spec is None:
        return None
    beta, scale = float(spec[0]), float(spec[1])
    if not (math.isfinite(beta) and math.isfinite(scale) and beta >= 0.0 and scale > 0.0):
        raise ValueError(f"{who}: loss spec (beta, scale) must be finite with beta >= 0 and scale > 0, got {spec!r}")
    return (beta, scale)


def torch_loss(pred, target, spec):
    """The spec's loss through torch.nn.functional (any tensor): what the fused launches are tested against."""
    if spec is None:
        return F.mse_loss(pred, target)
    beta, scale = spec
    if beta == 0.0:
        return F.l1_loss(pred, target) if scale == 1.0 else scale * F.l1_loss(pred, target)
    if scale == 1.0:
        return F.smooth_l1_loss(pred, target, beta=beta)
    if scale == beta:
        return F.huber_loss(pred, target, delta=beta)
    return scale * F.smooth_l1_loss(pred, target, beta=beta)


class _SmoothL1Loss(torch.autograd.Function):
    """The family's mean loss with forward value and gradient from ONE launch (eqh_smooth_l1_fwd_bwd): _MseLoss's twin."""

    @staticmethod
    def forward(ctx, pred, target, beta, scale):
        _require_gpu(pred, "regression_loss")
        pred, target = _f32c(pred), _f32c(target)
        n = pred.numel()
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        hip.check(hip.lib().eqh_smooth_l1_fwd_bwd(_ptr(pred), _ptr(target), n, beta, scale, _ptr(loss), _ptr(grad),
                                                  _stream(pred.device)), "eqh_smooth_l1_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (grad,) = ctx.saved_tensors
        return grad * dloss, None, None, None


def regression_loss(pred, target, spec=None):
    """The training loss of ``spec`` (``loss_spec``): None is ``mse_loss``, unchanged; otherwise the mean of the family's terms,
    from one launch under mse_loss's conditions (1-D fp32 device tensors of up to 65 536 values), else through torch."""
    if spec is None:
        return mse_loss(pred, target)
    beta, scale = _checked_spec(spec, "regression_loss")
    if (pred.is_cuda and pred.dtype == torch.float32 and 0 < pred.numel() <= 65536 and not target.requires_grad
            and pred.shape == target.shape):
        return _SmoothL1Loss.apply(pred.reshape(-1), target.reshape(-1), beta, scale)
    return torch_loss(pred, target, (beta, scale))


def pool_pair_bytes(N: int, M: int, B: int, C: int) -> tuple:
    """Algorithmic bytes of (hg_pool_pair_fwd, hg_pool_pair_bwd): forward 4C (N + M) rows (an upper bound: hyperedge rows of
    order <= 2 are skipped) + 4 (N + M) entries + 8 M orders + 8 (B + 1) row pointers + 8 C B output; backward 4C (N + M)
    rows written + 4 (N + M) molecule ids + 8 M orders + 8 C B read."""
    return (4 * C * (N + M) + 4 * (N + M) + 8 * M + 8 * (B + 1) + 8 * C * B, 4 * C * (N + M) + 4 * (N + M) + 8 * M + 8 * C * B)


class _PoolPair(torch.autograd.Function):
    """[global_add_pool(x, batch) | global_add_pool(e[e_order > 2], he_batch)] as ONE launch each way (hg_pool_pair_fwd/bwd):
    no mask tensor, no [M, C] product, no concatenation."""

    @staticmethod
    def forward(ctx, x, e, pool, x_mol, he_pool, e_mol, e_order):
        _require_gpu(x, "pool_pair")
        x, e = _f32c(x), _f32c(e)
        (N, C), M, B = x.shape, e.shape[0], pool.n_rows
        out = torch.empty((B, 2 * C), dtype=torch.float32, device=x.device)
        timed("k_pool_pair_fwd", pool_pair_bytes(N, M, B, C)[0],
              lambda: hip.check(hip.lib().hg_pool_pair_fwd(_ptr(x), _ptr(pool.rowptr), _ptr(pool.perm), N, _ptr(e),
                                                           _ptr(he_pool.rowptr), _ptr(he_pool.perm), _ptr(e_order), M,
                                                           _ptr(out), B, C, _stream(x.device)), "hg_pool_pair_fwd"))
        ctx.keys, ctx.sizes = (x_mol, e_mol, e_order), (N, M, B, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        x_mol, e_mol, e_order = ctx.keys
        N, M, B, C = ctx.sizes
        dout = _f32c(dout)
        dx = torch.empty((N, C), dtype=torch.float32, device=dout.device)
        de = torch.empty((M, C), dtype=torch.float32, device=dout.device)
        timed("k_pool_pair_bwd", pool_pair_bytes(N, M, B, C)[1],
              lambda: hip.check(hip.lib().hg_pool_pair_bwd(_ptr(dout), _ptr(x_mol), N, _ptr(e_mol), _ptr(e_order), M, _ptr(dx),
                                                           _ptr(de), B, C, _stream(dout.device)), "hg_pool_pair_bwd"))
        return dx, de, None, None, None, None, None


def pool_pair(x, e, index, n_e, e_order):
    """[B, 2C]: per molecule the sum of its node rows ``x`` [N, C] next to the sum of its hyperedge rows ``e`` [M, C] of order
    > 2 (equihnn_fa_former.py:99-101) -- zeros where a molecule has none.  ``index``: the batch's HyperIndex (its atom pool
    and, from ``n_e``, its hyperedge pool); ``e_order`` int64 [M]."""
    if x.dim() != 2 or e.dim() != 2 or x.shape[1] != e.shape[1]:
        raise ValueError(f"pool_pair: x [N, C] and e [M, C] of one width, got {tuple(x.shape)} and {tuple(e.shape)}")
    he_pool, e_mol = index.hyperedge_pool(n_e)
    if he_pool.n_rows != index.pool.n_rows or e_order.shape[0] != e.shape[0] or x.shape[0] != index.N:
        raise ValueError("pool_pair: x, e, n_e and e_order do not belong to this index's batch")
    if e_order.dtype != torch.int64:
        raise TypeError(f"pool_pair: e_order must be int64, got {e_order.dtype}")
    return _PoolPair.apply(x, e, index.pool, index.batch32, he_pool, e_mol, e_order.contiguous())


_READOUT_STATE = {}


def _readout_state(device):
    key = torch.device(device).index
    if key not in _READOUT_STATE:
        _READOUT_STATE[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _READOUT_STATE[key]


def _head_forward(ctx, entry, pools, rows, n_graphs, n_real, C, target, eps, unit_grad, params, drop, weights, loss_fam=None):
    """What the forward() of both heads does around its one launch, ``entry``_f32 or (``drop`` given) ``entry``_drop_f32 -- with
    ``loss_fam`` = (beta, scale) the ``sl1`` twin of either, the two floats in front of the stream:
    ``pools`` are the entry's leading arguments (the rows and their per-molecule lists), ``rows`` the fp32 row tensors that get a
    gradient.  The gradients are computed here; the parameter gradients go straight into their persistent accumulators when
    ``unit_grad`` says the incoming gradient is the implicit 1 of ``loss.backward()`` and every parameter has one.
    ``drop`` = (p_x, p_h, *seeds): the seeds are int64 device tensors the kernel reads, so nothing is kept for the backward."""
    dev = rows[0].device
    target = _f32c(target)
    ws_t = [_f32c(w.detach()) for w in weights]
    H = ws_t[0].shape[0]
    L = hip.lib()
    vp = ctypes.c_void_p * 10
    y = torch.empty(n_graphs, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d_rows = [torch.empty_like(r) for r in rows]
    ws_bytes = getattr(L, entry + "_workspace_bytes")(n_graphs, C, H)
    ws = _workspace(ws_bytes, dev)
    tg = [_acc_target(w) for w in params] if unit_grad else [None]
    in_place = all(t is not None for t in tg)
    grads = tg if in_place else [torch.empty_like(w) for w in ws_t]
    args = (*pools, n_graphs, n_real, C, H, vp(*[w.data_ptr() for w in ws_t]), float(eps), _ptr(target), _ptr(y), _ptr(loss),
            *[_ptr(d) for d in d_rows], vp(*[g.data_ptr() for g in grads]), 1 if in_place else 0, _ptr(ws), ws_bytes,
            _ptr(_readout_state(dev)))
    name = entry + "_f32"
    if drop is not None:
        name = entry + "_drop_f32"
        args += (drop[0], drop[1], *[_ptr(s) for s in drop[2:]])
    if loss_fam is not None:
        name = name.replace("_mse", "_sl1")
        args += (loss_fam[0], loss_fam[1])
    hip.check(getattr(L, name)(*args, _stream(dev)), name)
    ctx.unit_grad, ctx.in_place, ctx.n_rows = unit_grad, in_place, len(rows)
    ctx.targets = tg if (unit_grad and not in_place) else [None] * 10
    ctx.held = (*d_rows,) if in_place else (*d_rows, *grads)
    ctx.mark_non_differentiable(y)
    ctx.set_materialize_grads(False)        # (no zero-filled gradient tensor for the predictions: one launch per step)
    return loss, y


def _head_backward(ctx, dloss, n_other):
    """Hands out what _head_forward computed -- scaled by the incoming gradient unless ``unit_grad``.  ``n_other``: forward()'s
    arguments between the rows and the ten weights, which get no gradient."""
    held, n_rows = ctx.held, ctx.n_rows
    if dloss is None:
        return (None,) * (n_rows + n_other + 10)
    if not ctx.unit_grad:
        held = tuple(h * dloss for h in held)
    dws = (None,) * 10 if ctx.in_place else tuple(_hand_out([g.view_as(g) for g in held[n_rows:]], ctx.targets))
    return (*held[:n_rows], *(None,) * n_other, *dws)


class _ReadoutMse(torch.autograd.Function):
    """pool -> MLP(C -> H -> H -> 1, LN) -> MSE with loss, dx and all parameter gradients from ONE launch
    (hg_readout_mse_f32): _head_forward / _head_backward.
    ``drop`` = (p_x, p_h, seed_x, seed_h1, seed_h2) or None: the launch under training dropout (hg_readout_mse_drop_f32).
    ``loss_fam`` = (beta, scale) or None: the family of ``loss_spec`` in the place of the MSE (hg_readout_sl1_f32 / _drop_f32)."""

    @staticmethod
    def forward(ctx, x, rowptr, n_graphs, n_real, target, eps, unit_grad, params, drop, loss_fam, *weights):
        _require_gpu(x, "readout_mse")
        x = _f32c(x)
        return _head_forward(ctx, "hg_readout_mse", (_ptr(x), _ptr(rowptr)), (x,), n_graphs, n_real, weights[0].shape[1], target,
                             eps, unit_grad, params, drop, weights, loss_fam)

    @staticmethod
    def backward(ctx, dloss, _dy):
        return _head_backward(ctx, dloss, 9)


class _ReadoutPairMse(torch.autograd.Function):
    """[node pool | order > 2 hyperedge pool] -> MLP(2C -> H -> H -> 1, LN) -> MSE with loss, dx, de and all parameter gradients
    from ONE launch (hg_readout_pair_mse_f32): _ReadoutMse for the paired tail.
    ``drop`` = (p_x, p_h, seed_x, seed_e, seed_h1, seed_h2) or None (hg_readout_pair_mse_drop_f32); ``loss_fam`` = (beta, scale)
    or None (hg_readout_pair_sl1_f32 / _drop_f32)."""

    @staticmethod
    def forward(ctx, x, e, rowptr, he_pool, e_order, n_graphs, n_real, target, eps, unit_grad, params, drop, loss_fam, *weights):
        _require_gpu(x, "readout_pair_mse")
        x, e = _f32c(x), _f32c(e)
        pools = (_ptr(x), _ptr(rowptr), _ptr(e), _ptr(he_pool.rowptr), _ptr(he_pool.perm), _ptr(e_order), e.shape[0])
        return _head_forward(ctx, "hg_readout_pair_mse", pools, (x, e), n_graphs, n_real, x.shape[1], target, eps, unit_grad,
                             params, drop, weights, loss_fam)

    @staticmethod
    def backward(ctx, dloss, _dy):
        return _head_backward(ctx, dloss, 11)


def _head_drop_p(mlp) -> float:
    """The head's hidden-layer dropout probability in effect (mlp.py:97): 0 in eval mode."""
    return float(mlp.dropout) if (mlp.training and mlp.dropout > 0) else 0.0


def _mlp_ok(mlp, c_in: int, C: int, entry: str) -> bool:
    """The head's side of the question (no tensor, no device): three Linears c_in -> H -> H -> 1, LayerNorm behind both hidden
    layers with one eps, no InputNorm, (C, H) the kernel behind ``entry`` is built for."""
    lins = getattr(mlp, "lins", None)
    if lins is None or len(lins) != 3:
        return False
    norms = mlp.normalizations
    if mlp.InputNorm or not all(isinstance(n, torch.nn.LayerNorm) for n in norms[1:]):
        return False
    H = lins[0].weight.shape[0]
    if lins[0].weight.shape != (H, c_in) or lins[1].weight.shape != (H, H) or lins[2].weight.shape != (1, H):
        return False
    if norms[1].eps != norms[2].eps:
        return False
    return bool(getattr(hip.lib(), entry)(C, H))


def _rows_ok(*rows) -> bool:
    return all(t.is_cuda and t.dim() == 2 and t.dtype == torch.float32 and t.shape[1] == rows[0].shape[1] for t in rows)


def _drop_allowed(p_x: float, p_h: float) -> bool:
    """Whether a head may take its dropout form: ops.FUSED_DROPOUT and ops.READOUT_DROPOUT on, at least one probability above 0
    and both below 1."""
    return bool(_rows.FUSED_DROPOUT and READOUT_DROPOUT) and 0.0 <= p_x < 1.0 and p_h < 1.0 and (p_x > 0.0 or p_h > 0.0)


def _mlp_weights(mlp) -> tuple:
    """The ten weights of the head's MLP in the entries' order; its leaf parameters are registered for the in-place gradient
    accumulators."""
    lins, norms = mlp.lins, mlp.normalizations
    weights = (lins[0].weight, lins[0].bias, norms[1].weight, norms[1].bias, lins[1].weight, lins[1].bias,
               norms[2].weight, norms[2].bias, lins[2].weight, lins[2].bias)
    if torch.is_grad_enabled():
        for w in weights:
            if w.requires_grad and w.is_leaf:
                (LINEAR_PARAMS if w.dim() == 2 else ACC_PARAMS)[id(w)] = w
    return weights


def _head_drop(name: str, device, p_x: float, mlp, seeds, n_pre: int):
    """The ``drop`` argument of a head's Function: None without an active site, else (p_x, p_h, *seeds) with the seeds drawn
    through ``_dropout_seed`` in the order of the separate launches -- the ``n_pre`` pre-pool sites (only when ``p_x`` > 0),
    hidden layer 1, hidden layer 2 -- unless ``seeds`` gives them."""
    p_x, p_h = float(p_x), _head_drop_p(mlp)
    if not (0.0 <= p_x < 1.0 and p_h < 1.0):
        raise ValueError(f"{name}: dropout probabilities have to be in [0, 1), but got p_x = {p_x}, p_h = {p_h}")
    if p_x == 0.0 and p_h == 0.0:
        return None
    if seeds is None:
        seeds = [_dropout_seed(device, p) for p in (p_x,) * n_pre + (p_h, p_h)]
    return (p_x, p_h, *seeds)


def _head_shape_ok(x, mlp) -> bool:
    return _rows_ok(x) and _mlp_ok(mlp, x.shape[1], x.shape[1], "hg_readout_mse_supported")


def readout_mse_supported(x, mlp) -> bool:
    """Whether ops.readout_mse takes this pooled-MLP head without dropout: 2-D fp32 device rows, MLP of three Linears with
    LayerNorm hidden layers and one output, no active dropout, widths the kernel is built for."""
    return _head_drop_p(mlp) == 0.0 and _head_shape_ok(x, mlp)


def readout_mse_drop_supported(x, mlp, p_x: float = 0.0) -> bool:
    """Whether ops.readout_mse takes this head UNDER an active dropout -- ``p_x`` in front of the pool, the head's own behind
    its hidden layers: the shapes of readout_mse_supported and _drop_allowed."""
    return _drop_allowed(float(p_x), _head_drop_p(mlp)) and _head_shape_ok(x, mlp)


def readout_mse(x, pool_rowptr, mlp, target, n_real=None, unit_grad=False, p_x=0.0, seeds=None, loss=None):
    """(loss, predictions) of the readout head: x [N, C] node rows, pool_rowptr int32 [B+1] (sorted ``batch``),
    ``mlp`` the output MLP, ``target`` [>= n_real]; loss = mean over the first n_real molecules.
    Under training dropout (``p_x`` > 0: dropout of the node rows in front of the pool; the head's own probability when it is
    training) the launch is the dropout form, see readout_mse_drop_supported.  Its seeds are drawn through ``_dropout_seed`` in
    the order pre-pool (only when ``p_x`` > 0), hidden layer 1, hidden layer 2 -- the order of the separate launches -- unless
    ``seeds`` = (seed_x, seed_h1, seed_h2) gives them (int64 [1] device tensors; None for a site that is off).
    ``loss``: None for the MSE, or a ``loss_spec`` (beta, scale): the same launch with that loss (hg_readout_sl1_*)."""
    loss = _checked_spec(loss, "readout_mse")
    n_graphs = pool_rowptr.shape[0] - 1
    n_real = n_graphs if n_real is None else int(n_real)
    weights = _mlp_weights(mlp)
    drop = _head_drop("readout_mse", x.device, p_x, mlp, seeds, 1)
    return _ReadoutMse.apply(x, pool_rowptr, n_graphs, n_real, target, mlp.normalizations[1].eps, unit_grad, weights, drop,
                             loss, *weights)


def _pair_mlp_ok(mlp, C: int) -> bool:
    """_mlp_ok for the paired head: the first Linear on 2C inputs."""
    return _mlp_ok(mlp, 2 * C, C, "hg_readout_pair_mse_supported")


def readout_pair_mse_supported(x, e, mlp) -> bool:
    """Whether ops.readout_pair_mse takes this head without dropout: x [N, C] and e [M, C] 2-D fp32 device rows, MLP of three
    Linears (the first on 2C inputs) with LayerNorm hidden layers and one output, no active dropout, widths the kernel is built
    for (C in 64 / 128 / 256, hidden width 128 / 256)."""
    return _head_drop_p(mlp) == 0.0 and _rows_ok(x, e) and _pair_mlp_ok(mlp, x.shape[1])


def readout_pair_mse_drop_supported(x, e, mlp, p_x: float = 0.0) -> bool:
    """... UNDER an active dropout (``p_x`` on x and e in front of the pools, the head's own behind its hidden layers): the shapes
    of readout_pair_mse_supported and _drop_allowed."""
    return _drop_allowed(float(p_x), _head_drop_p(mlp)) and _rows_ok(x, e) and _pair_mlp_ok(mlp, x.shape[1])


def readout_pair_mse(x, e, index, n_e, e_order, mlp, target, n_real=None, unit_grad=False, p_x=0.0, seeds=None, loss=None):
    """(loss, predictions) of the paired tail's head: x [N, C] node rows and e [M, C] hyperedge rows of the batch of ``index``
    (its atom pool and, from ``n_e``, its hyperedge pool), ``e_order`` int64 [M] (only hyperedges of order > 2 are pooled),
    ``mlp`` the output MLP on [B, 2C], ``target`` [>= n_real]; loss = mean over the first n_real molecules.
    Under training dropout (``p_x`` > 0 on x and on e in front of the pools; the head's own probability when it is training)
    the launch is the dropout form.  Its seeds are drawn through ``_dropout_seed`` in the order x, e (both only when ``p_x`` >
    0), hidden layer 1, hidden layer 2 -- the order of the separate launches -- unless ``seeds`` = (seed_x, seed_e, seed_h1,
    seed_h2) gives them (int64 [1] device tensors; None for a site that is off).
    ``loss``: None for the MSE, or a ``loss_spec`` (beta, scale): the same launch with that loss (hg_readout_pair_sl1_*)."""
    loss = _checked_spec(loss, "readout_pair_mse")
    if x.dim() != 2 or e.dim() != 2 or x.shape[1] != e.shape[1]:
        raise ValueError(f"readout_pair_mse: x [N, C] and e [M, C] of one width, got {tuple(x.shape)} and {tuple(e.shape)}")
    he_pool, _ = index.hyperedge_pool(n_e)
    n_graphs = index.pool.n_rows
    if he_pool.n_rows != n_graphs or e_order.shape[0] != e.shape[0] or x.shape[0] != index.N:
        raise ValueError("readout_pair_mse: x, e, n_e and e_order do not belong to this index's batch")
    if e_order.dtype != torch.int64:
        raise TypeError(f"readout_pair_mse: e_order must be int64, got {e_order.dtype}")
    n_real = n_graphs if n_real is None else int(n_real)
    weights = _mlp_weights(mlp)
    drop = _head_drop("readout_pair_mse", x.device, p_x, mlp, seeds, 2)
    return _ReadoutPairMse.apply(x, e, index.pool.rowptr, he_pool, e_order.contiguous(), n_graphs, n_real, target,
                                 mlp.normalizations[1].eps, unit_grad, weights, drop, loss, *weights)
